"""Torus primitives on the GPU (RTC_TORUS, the torus kernels): every render of the fixture against the
checker (tests/cpp/torus_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no pixel masked - default
sampling, a sample grid with a lens, a later pass, the moving torus, both kernel forms, a close-up and a view from 1000
units away -, the torus kernels on handles without a torus against their ordinary renders, the kernel's name, a torus no
ray reaches, clones and band clones, Progressive, an adaptive run, rtch_scene_render and rtc_get_tile_costs.

Measured on an MI355X: see DESIGN.md section 18."""
import json

import numpy as np
import pytest

import bump_binding as bb
import camera_binding as cb
import test_table_limits_gpu as limits
import torus_binding as tb

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the project's bound for a render against its checker, sections 11-17)
FORCED_TOL = 1e-14  # (section 17's bound for a kernel family forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (tests/test_sampling_gpu.py: shares of a split frame's pixels added in another order)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
TORUS, TORUS_BIG = "rtc_render_kernel_torus", "rtc_render_kernel_torus_bigworld"


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, disp=None, light_seed=0):
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    if sample_pass:
        gpu.set_sample_pass(sample_pass)
    if disp is not None:
        gpu.set_motion(disp)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    return gpu


def check(rtc, hs, cam, smp=None, sample_pass=0, disp=None, depth=5, light_seed=0, kernel=TORUS):
    gpu = handle(rtc, hs, smp, sample_pass, disp, light_seed)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = tb.TorusScene(hs.desc, hs.lights, hs.bumps()).render(cam, depth, smp, hs.spots(), disp, sample_pass,
                                                                         light_seed=light_seed)
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    compare(got, want)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    assert st["overflow"] == 0
    return got, gpu


def static(hs):
    return np.zeros((hs.desc.n_roots, 3))


# ---- the fixture against the checker: 80 x 45, depth 5
def test_fixture_against_the_checker(rtc):
    hs = tb.mix(rtc)
    assert len(tb.tori_of(hs.desc)) == 10
    check(rtc, hs, hs.camera(80, 45), disp=static(hs), light_seed=3)


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = tb.mix(rtc)
    check(rtc, hs, hs.camera(80, 45), cb.sampling(2, True, aperture=0.08, focal_distance=7.0, seed=5), disp=static(hs), light_seed=3)


def test_fixture_at_sample_pass_3(rtc):
    hs = tb.mix(rtc)
    cam = hs.camera(80, 45)
    p0, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), disp=static(hs))
    p3, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), sample_pass=3, disp=static(hs))
    assert not np.array_equal(p0, p3)


def test_fixture_with_the_moving_torus(rtc):
    hs = tb.mix(rtc)
    disp = hs.motion()
    assert np.count_nonzero(np.abs(disp).sum(axis=1)) == 1   # the fixture's one moving torus
    moving, _ = check(rtc, hs, hs.camera(80, 45), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)
    still, _ = check(rtc, hs, hs.camera(80, 45), cb.sampling(2, True, seed=6), disp=static(hs), light_seed=11)
    assert not np.array_equal(moving, still)


def _with_many_lights(n):
    """torus_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_spot_lights_gpu.py's way)"""
    scene = json.loads(open(tb.TORUS_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra), tb.TORUS_DIR)
    assert hs.lights.n_lights == L_LIGHTS + extra
    check(rtc, hs, hs.camera(80, 45), disp=hs.motion(), light_seed=3, kernel=TORUS_BIG if extra else TORUS)


# ---- a close-up and a view from far away
def _one_torus(cam):
    objects = [{"type": {"plane": {}}, "transform": [{"translate": [0, -1.2, 0]}], "material": {"specular": 0, "reflective": 0.2}},
               {"type": {"torus": {"major-radius": 1.0, "minor-radius": 0.4}}, "transform": [{"rotate-x": 0.9}, {"rotate-z": 0.3}],
                "material": {"pattern": {"type": {"solid": [0.8, 0.5, 0.3]}}, "reflective": 0.3, "transparency": 0.5,
                             "refractive-index": 1.3}}]
    lights = [{"point-light": {"position": [-5, 8, -6], "intensity": [1, 1, 1]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": objects})


def test_close_up_where_the_torus_fills_the_frame(rtc):
    cam = {"width": 80, "height": 45, "field-of-view": 1.2, "from": [0.2, 0.3, -1.15], "to": [0.6, 0, 0], "up": [0, 1, 0]}
    hs = rtc.HostScene(_one_torus(cam))
    got, _ = check(rtc, hs, hs.camera())
    assert got.std() > 0.01


def test_view_from_1000_units_with_a_narrow_field_of_view(rtc):
    """The re-centring step at work: the coefficients of a ray that starts 1000 units away, taken about its origin,
    cancel to nothing; about the point nearest the centre they do not."""
    cam = {"width": 80, "height": 45, "field-of-view": 0.004, "from": [300, 500, -812.4], "to": [0, 0, 0], "up": [0, 1, 0]}
    hs = rtc.HostScene(_one_torus(cam))
    got, _ = check(rtc, hs, hs.camera())
    assert got.std() > 0.01          # the torus is in the picture


# ---- the torus kernels on a handle without a torus; the kernel's name
@pytest.mark.parametrize("name", ["cover.json", "bump_mix", "teapot.json"])
def test_torus_kernels_without_a_torus_are_the_ordinary_render(rtc, name):
    hs = bb.mix(rtc) if name == "bump_mix" else rtc.HostScene.from_file(name)
    cam = hs.camera(128, 72)
    gpu = handle(rtc, hs)
    ordinary = gpu.render(cam, 5)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_torus" not in old_name
    rtc.set_option("torus_kernels", 1)
    try:
        forced = gpu.render(cam, 5)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == TORUS
    finally:
        rtc.set_option("torus_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {TORUS}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, 5)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert "_torus" not in gpu.last_kernel_name()


def test_a_world_with_a_torus_runs_the_torus_kernels_whatever_else_it_has(rtc):
    cam = {"width": 64, "height": 36, "field-of-view": 0.8, "from": [0, 1.5, -6], "to": [0, 0.5, 0], "up": [0, 1, 0]}
    lights = [{"point-light": {"position": [-4, 8, -4], "intensity": [1, 1, 1]}}]
    spheres = [{"type": {"sphere": {}}}, {"type": {"plane": {}}, "transform": [{"translate": [0, -1, 0]}]}]
    plain = rtc.HostScene(json.dumps({"camera": cam, "lights": lights, "objects": spheres}))
    gpu = rtc.GpuScene(plain.desc, lights=plain.lights)
    gpu.render(plain.camera(), 5)
    assert "simple" in gpu.last_kernel_name()
    hs = rtc.HostScene(json.dumps({"camera": cam, "lights": lights, "objects": spheres + [{"type": {"torus": {}},
                                                                                            "transform": [{"translate": [2, 0, 0]}]}]}))
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)    # (no sampling, motion, spots or bumps set)
    got = gpu.render(hs.camera(), 5)
    assert gpu.last_kernel_name() == TORUS
    want, _ = tb.TorusScene(hs.desc, hs.lights).render(hs.camera(), 5)
    compare(got, want)


def test_a_torus_no_ray_reaches_leaves_every_bit(rtc):
    """The torus lies behind the camera of a scene without reflection and casts no shadow: the image is the one of the
    scene without it, which another kernel renders."""
    cam = {"width": 64, "height": 36, "field-of-view": 0.8, "from": [0, 1.5, -6], "to": [0, 1, 0], "up": [0, 1, 0]}
    objects = [{"type": {"plane": {}}, "material": {"specular": 0, "pattern": {"type": {"checkers": [{"type": {"solid": [1, 1, 1]}},
                                                                                                  {"type": {"solid": [0.2, 0.2, 0.2]}}]}}}},
               {"type": {"cube": {}}, "transform": [{"rotate-y": 0.5}, {"translate": [0, 1, 0]}], "material": {"diffuse": 0.6}}]
    torus = {"type": {"torus": {}}, "transform": [{"translate": [0, 1, -40]}], "casts-shadow": False}
    lights = [{"point-light": {"position": [-4, 8, -4], "intensity": [1, 1, 1]}}]
    without = rtc.HostScene(json.dumps({"camera": cam, "lights": lights, "objects": objects}))
    plain = rtc.GpuScene(without.desc, lights=without.lights)
    flat = plain.render(without.camera(), 5)
    assert "_torus" not in plain.last_kernel_name()
    hs = rtc.HostScene(json.dumps({"camera": cam, "lights": lights, "objects": objects + [torus]}))
    got, _ = check(rtc, hs, hs.camera())
    assert np.array_equal(got, flat)


# ---- a clone, band clones
def test_a_clone_and_band_clones_follow(rtc):
    hs = tb.mix(rtc)
    cam = hs.camera(160, 96)
    gpu = handle(rtc, hs, disp=hs.motion())
    rtc.set_option("host_bands", 3)
    try:
        banded = gpu.render(cam, 5)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = tb.TorusScene(hs.desc, hs.lights, hs.bumps()).render(cam, 5, spots=hs.spots(), disp=hs.motion())
    compare(banded, want)
    assert st["primary"] == counters["primary"] and st["shadow_calls"] == counters["shadow_calls"]
    whole = gpu.render(cam, 5)
    assert float(np.abs(whole - banded).max()) <= SPLIT_TOL
    clone = gpu.clone()
    assert float(np.abs(clone.render(cam, 5) - whole).max()) <= SPLIT_TOL
    assert clone.last_kernel_name() == TORUS


# ---- Progressive, an adaptive run, rtch_scene_render, rtc_get_tile_costs
def _pass_images(hs, cam, smp, n):
    ck = tb.TorusScene(hs.desc, hs.lights, hs.bumps())
    return [ck.render(cam, 5, smp, hs.spots(), hs.motion(), sample_pass=p)[0] for p in range(n)]


def test_progressive_mean_is_the_checkers(rtc):
    import torch
    hs = tb.mix(rtc)
    cam = hs.camera(64, 36)
    smp = cb.sampling(1, True, seed=4)
    gpu = handle(rtc, hs, smp, disp=hs.motion())
    prog = rtc.Progressive(gpu, cam, 5)
    for _ in range(4):
        prog.step()
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == TORUS
    compare(mean, np.mean(_pass_images(hs, cam, smp, 4), axis=0))


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(tb.TORUS_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 6,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene), tb.TORUS_DIR)
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, 5, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling(), disp=hs.motion())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == TORUS
    assert np.array_equal(out, rgb)
    assert passes.min() >= 2 and passes.max() <= 6
    images = _pass_images(hs, hs.camera(), hs.sampling(), 6)
    want = np.zeros_like(rgb)
    tiles_x = 80 // 16
    for t, k in enumerate(passes):
        ty, tx = divmod(t, tiles_x)
        want[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = np.mean([im[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] for im in images[:k]], axis=0)
    compare(rgb, want)
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the moving torus included
    plain = tb.mix(rtc)
    out1 = np.zeros((45, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, 80, 45, 5, out1.ctypes.data))
    want1, _ = tb.TorusScene(plain.desc, plain.lights, plain.bumps()).render(plain.camera(80, 45), 5, spots=plain.spots(), disp=plain.motion())
    compare(out1, want1)


def test_tile_costs_of_the_fixture_are_finite_and_positive(rtc):
    torch = pytest.importorskip("torch")
    hs = tb.mix(rtc)
    cam = hs.camera(160, 96)
    T = 32
    n_tiles = (160 // T) * (96 // T)
    gpu = handle(rtc, hs, disp=hs.motion())
    stream = torch.cuda.Stream()
    buf = torch.zeros((n_tiles, T, T, 3), dtype=torch.float64, device="cuda")
    gpu.render_tiles_device(cam, buf.data_ptr(), T, T, 0, 1, n_tiles, 5, stream.cuda_stream)
    costs = np.asarray(gpu.tile_costs(n_tiles))
    stream.synchronize()
    assert gpu.last_kernel_name() == TORUS
    assert costs.shape == (n_tiles,) and np.isfinite(costs).all() and (costs > 0).all()
