"""Ambient occlusion on the GPU (rtc_scene_set_occlusion, the occlusion kernels): every render of the
fixture against the checker (tests/cpp/occlusion_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no pixel
masked - default sampling, a sample grid with a lens, a later pass, a moving root, 1, 4 and 64 samples, both kernel forms,
band clones, a shuffled tile list, Progressive, an adaptive run, rtch_scene_render -, a deep ray tree whose path codes reach
17 bits, occlusion against none, the occlusion kernels forced on handles without a radius, the derived mean of the parallel
planes, the setter's refusals, and the seed.  80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 21."""
import json

import numpy as np
import pytest

import camera_binding as cb
import gloss_binding as gb
import meshuv_binding as mb
import occlusion_binding as ob
import test_table_limits_gpu as limits
import torus_binding as tb

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the issue's bound for a render against its checker: test_gloss_gpu.py's)
FORCED_TOL = 1e-14  # (the issue's bound for the occlusion kernels forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
OCCL, OCCL_BIG = "rtc_render_kernel_occl", "rtc_render_kernel_occl_bigworld"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, disp=None, light_seed=0, occlusion="scene"):
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
    gpu.set_mesh_uvs(hs.mesh_uvs())
    gpu.set_gloss(hs.gloss())
    gpu.set_occlusion(hs.occlusion() if isinstance(occlusion, str) else occlusion)
    return gpu


def checker(hs, occlusion="scene"):
    return ob.OcclScene(hs.desc, hs.lights, hs.bumps(), hs.mesh_uvs(), hs.gloss(), hs.occlusion() if isinstance(occlusion, str) else occlusion)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, disp=None, light_seed=0, kernel=OCCL, occlusion="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, disp, light_seed, occlusion)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(hs, occlusion).render(cam, depth, smp, hs.spots(), disp, sample_pass, light_seed=light_seed)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = ob.mix(rtc)
    o = hs.occlusion()
    assert sorted(set(o["radius"])) == [0.0, 0.3, 3.0, 1e3] and o["samples"] == 4 and len(tb.tori_of(hs.desc)) == 1
    got, _, c = check(rtc, hs, hs.camera(W, H), light_seed=3)
    n = c["occluded"] + c["unoccluded"]
    assert c["occluded"] >= 0.1 * n and c["unoccluded"] >= 0.1 * n and c["skipped"] > 0 and c["deep"] > 0
    assert got.std() > 0.05


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = ob.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=7.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc):
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    p0, _, _ = check(rtc, hs, cam, cb.sampling(1, False))   # (occlusion is sampled even without jitter)
    p3, _, _ = check(rtc, hs, cam, cb.sampling(1, False), sample_pass=3)
    assert not np.array_equal(p0, p3)


def test_fixture_with_a_moving_root(rtc):
    hs = ob.mix(rtc)
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[2] = (0.5, 0.0, 0.3)
    moving, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)
    still, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), light_seed=11)
    assert not np.array_equal(moving, still)


@pytest.mark.parametrize("samples", [1, 4, 64])
def test_fixture_at_1_4_and_64_samples(rtc, samples):
    hs = ob.mix(rtc)
    o = dict(hs.occlusion(), samples=samples)
    _, gpu, c = check(rtc, hs, hs.camera(W, H), occlusion=o)
    assert (c["occluded"] + c["unoccluded"]) % samples == 0
    # every occlusion sample is a call of isShadowed and is traced
    _, c0 = checker(hs, None).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    assert c["shadow_calls"] - c0["shadow_calls"] == c["occluded"] + c["unoccluded"]
    gpu0 = handle(rtc, hs, occlusion=None)
    gpu0.render(hs.camera(W, H), DEPTH)
    assert gpu.stats()["shadow_traced"] - gpu0.stats()["shadow_traced"] == c["occluded"] + c["unoccluded"]


def _with_many_lights(n):
    """occlusion_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_torus_gpu.py's way)"""
    scene = json.loads(open(ob.OCCL_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra), ob.OCCL_DIR)
    assert hs.lights.n_lights == L_LIGHTS + extra
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=OCCL_BIG if extra else OCCL)


# ---- band clones, a clone, a shuffled tile list
def test_a_clone_and_band_clones_follow(rtc):
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    rtc.set_option("host_bands", 3)
    try:
        banded = gpu.render(cam, DEPTH)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = checker(hs).render(cam, DEPTH, spots=hs.spots())
    compare(banded, want)
    same_counts(st, counters)   # (the bands' counts, summed)
    whole = gpu.render(cam, DEPTH)
    assert float(np.abs(whole - banded).max()) <= SPLIT_TOL
    clone = gpu.clone()
    assert np.array_equal(clone.render(cam, DEPTH), whole)   # a clone starts with its source's table
    assert clone.last_kernel_name() == OCCL
    # the setter after the band clones exist: they follow
    other = dict(hs.occlusion(), seed=9)
    gpu.set_occlusion(other)
    rtc.set_option("host_bands", 3)
    try:
        banded9 = gpu.render(cam, DEPTH)
    finally:
        rtc.set_option("host_bands", 0)
    want9, _ = checker(hs, other).render(cam, DEPTH, spots=hs.spots())
    compare(banded9, want9)
    assert not np.array_equal(banded9, banded)


def test_a_shuffled_tile_list(rtc):
    import torch
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    tw, th = 16, 16
    tiles_x, tiles_y = -(-W // tw), -(-H // th)
    n_tiles = tiles_x * tiles_y
    tiles = np.random.default_rng(5).permutation(n_tiles).astype(np.uint32)
    buf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_tile_list_device(cam, buf.data_ptr(), tw, th, tiles, DEPTH)
    gpu.synchronize()
    st = gpu.stats()
    assert gpu.last_kernel_name() == OCCL
    want, counters = checker(hs).render(cam, DEPTH, spots=hs.spots())
    b = buf.cpu().numpy()
    got = np.zeros((H, W, 3))
    for k, t in enumerate(tiles):
        ty, tx = divmod(int(t), tiles_x)
        h, w = min(th, H - ty * th), min(tw, W - tx * tw)
        got[ty * th:ty * th + h, tx * tw:tx * tw + w] = b[k, :h, :w]
    compare(got, want)
    same_counts(st, counters)


# ---- Progressive, an adaptive run, rtch_scene_render
def test_progressive_mean_is_the_checkers(rtc):
    import torch
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    smp = cb.sampling(1, True, seed=4)
    gpu = handle(rtc, hs, smp)
    ck = checker(hs)
    want = [ck.render(cam, DEPTH, smp, hs.spots(), sample_pass=p) for p in range(4)]
    prog = rtc.Progressive(gpu, cam, DEPTH)
    for p in range(4):
        prog.step()
        same_counts(gpu.stats(), want[p][1])                    # (the handle's counts are its last launch's: pass p)
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == OCCL
    compare(mean, np.mean([im for im, _ in want], axis=0))


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(ob.OCCL_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "occlusion-seed": 7,
                                                          "occlusion-samples": 2,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene), ob.OCCL_DIR)
    assert hs.occlusion()["seed"] == 7 and hs.occlusion()["samples"] == 2
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == OCCL
    assert np.array_equal(out, rgb)
    assert passes.min() >= 2 and passes.max() <= 5
    ck = checker(hs)
    images = [ck.render(hs.camera(), DEPTH, hs.sampling(), hs.spots(), sample_pass=p)[0] for p in range(5)]
    want = np.zeros_like(rgb)
    tiles_x = 80 // 16
    for t, k in enumerate(passes):
        ty, tx = divmod(t, tiles_x)
        want[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = np.mean([im[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] for im in images[:k]], axis=0)
    compare(rgb, want)
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the radius rows applied.  (Its handle lives
    # and dies inside the call, so of the host render the image alone is held to the checker.)
    plain = ob.mix(rtc)
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    want1, _ = checker(plain).render(plain.camera(W, H), DEPTH, spots=plain.spots())
    compare(out1, want1)
    # ... and its corners are darker than the same file's without the key
    bare = checker(plain, None).render(plain.camera(W, H), DEPTH, spots=plain.spots())[0]
    assert out1.mean() < bare.mean()


# ---- a deep ray tree
def _mirror_hall():
    """Two facing rough mirrors with a rough glass pane between them, every material with an occlusion radius, seen at a
    slant: every level of the tree has a reflection and a refraction, and every hit its occlusion rays."""
    cam = {"width": 16, "height": 9, "field-of-view": 0.9, "from": [0.4, 0.3, -1.6], "to": [0, 0, 2], "up": [0, 1, 0],
           "sampling": {"occlusion-samples": 2}}
    mirror = {"pattern": {"type": {"solid": [0.1, 0.12, 0.1]}}, "diffuse": 0.3, "specular": 0.2, "reflective": 0.9,
              "roughness": {"reflection": 0.04}, "ambient-occlusion": 2.5}
    glass = {"pattern": {"type": {"solid": [0.05, 0.05, 0.1]}}, "diffuse": 0.1, "reflective": 0.6, "transparency": 0.9,
             "refractive-index": 1.3, "roughness": {"reflection": 0.03, "transmission": 0.05}, "ambient-occlusion": 2.5}
    objects = [{"type": {"cube": {}}, "transform": [{"scale": [3, 3, 0.05]}, {"translate": [0, 0, 2]}], "material": mirror},
               {"type": {"cube": {}}, "transform": [{"scale": [3, 3, 0.05]}, {"translate": [0, 0, -2]}], "material": mirror},
               {"type": {"cube": {}}, "transform": [{"scale": [3, 3, 0.05]}, {"rotate-y": 0.2}], "material": glass}]
    lights = [{"point-light": {"position": [0.5, 2, -1], "intensity": [0.9, 0.9, 0.9]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": objects})


def test_a_deep_tree_at_max_depth_16(rtc):
    hs = rtc.HostScene(_mirror_hall(), ob.OCCL_DIR)
    _, _, counters = check(rtc, hs, hs.camera(), depth=16)
    print("secondary per primary", counters["secondary"] / counters["primary"])
    assert counters["secondary"] > 16 * counters["primary"]      # levels with both children: codes of 17 bits, k << 17 above them
    assert counters["deep"] > counters["primary"] and counters["occluded"] > 0 and counters["unoccluded"] > 0


# ---- occlusion against none
def test_occlusion_only_scales_ambient_terms_down(rtc):
    """Every colour and intensity of the fixture is non-negative, and the gloss draws do not depend on the occlusion table:
    every channel of the occluded render is at most the unoccluded one's."""
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    occluded, gpu, _ = check(rtc, hs, cam, light_seed=3)
    gpu.set_occlusion(None)
    bare = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() != OCCL
    assert (occluded <= bare + 1e-12).all()
    assert not np.array_equal(occluded, bare)


# ---- which kernel; the occlusion kernels on a handle without a radius
def test_an_all_zero_table_restores_the_gloss_kernel(rtc):
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, occlusion=None)
    bare = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == "rtc_render_kernel_gloss"
    gpu.set_occlusion(hs.occlusion())
    assert not np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == OCCL
    gpu.set_occlusion({"radius": np.zeros(hs.desc.n_materials), "samples": 8, "seed": 5})
    assert np.array_equal(gpu.render(cam, DEPTH), bare)
    assert gpu.last_kernel_name() == "rtc_render_kernel_gloss"


@pytest.mark.parametrize("name", ["cover.json", "gloss_mix", "torus_mix", "mesh_mix", "teapot.json"])
def test_occlusion_kernels_without_a_radius_are_the_ordinary_render(rtc, name):
    hs = gb.mix(rtc) if name == "gloss_mix" else mb.mix(rtc) if name == "mesh_mix" else tb.mix(rtc) if name == "torus_mix" \
        else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    gpu.set_mesh_uvs(hs.mesh_uvs())
    gpu.set_gloss(hs.gloss())
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_occl" not in old_name
    rtc.set_option("occlusion_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == OCCL
    finally:
        rtc.set_option("occlusion_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {OCCL}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- the distribution, derived
def parallel_planes(radius):
    """A pure-ambient white floor under a shadow-casting plane at height 1, seen from between them: a pixel of a pass is the
    visibility of its one occlusion ray.  A cosine-weighted ray meets the ceiling within R exactly when cos(theta) > 1 / R:
    E[vis] = 1 / R^2 for R >= 1, and 1 below."""
    cam = {"width": 8, "height": 8, "field-of-view": 0.5, "from": [0, 0.5, 0], "to": [0, 0, 1], "up": [0, 1, 0]}
    floor = {"type": {"plane": {}}, "material": {"pattern": {"type": {"solid": [1, 1, 1]}}, "ambient": 1, "diffuse": 0, "specular": 0,
                                                 "ambient-occlusion": radius}}
    ceiling = {"type": {"plane": {}}, "transform": [{"translate": [0, 1, 0]}]}
    lights = [{"point-light": {"position": [0, 0.5, 0], "intensity": [1, 1, 1]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": [floor, ceiling]})


def test_parallel_planes_mean_is_a_quarter(rtc):
    import torch
    hs = rtc.HostScene(parallel_planes(2), ob.OCCL_DIR)
    cam = hs.camera()
    gpu = handle(rtc, hs, cb.sampling(1, True, seed=1))
    prog = rtc.Progressive(gpu, cam, DEPTH, noise=False)
    for _ in range(256):
        prog.step()
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == OCCL
    m = float(mean.mean())
    bound = 4.0 * np.sqrt(0.1875 / 16384)
    print(f"mean {m:.5f}, |mean - 0.25| {abs(m - 0.25):.5f}, bound {bound:.5f}")
    assert abs(m - 0.25) <= bound


# ---- rtc_scene_set_occlusion
def _status_name(rtc, code):
    return rtc.hip_lib().rtc_status_name(code).decode()


def test_selection_refusals_and_reset(rtc):
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    o = hs.occlusion()
    n = hs.desc.n_materials
    gpu = handle(rtc, hs, occlusion=None)
    bare = gpu.render(cam, DEPTH)
    old_name = gpu.last_kernel_name()
    assert old_name == "rtc_render_kernel_gloss"         # (the fixture has a rough mirror)
    gpu.set_occlusion(o)
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == OCCL and not np.array_equal(first, bare)
    clone = gpu.clone()
    bad = [dict(o, radius=o["radius"][:-1]),
           dict(o, radius=np.where(np.arange(n) == 2, np.nan, o["radius"])),
           dict(o, radius=np.where(np.arange(n) == 2, np.inf, o["radius"])),
           dict(o, radius=np.where(np.arange(n) == 0, -1e-9, o["radius"])),
           dict(o, samples=0), dict(o, samples=65)]
    for target in (gpu, clone):
        for b in bad:
            with pytest.raises(rtc.RtcError) as e:
                target.set_occlusion(b)
            assert e.value.name == _status_name(rtc, 1)                   # RTC_ERR_INVALID_ARGUMENT
            assert np.array_equal(target.render(cam, DEPTH), first)       # a refused table changes nothing
            assert target.last_kernel_name() == OCCL
    # NULL restores the previous kernel and its bits; the clone keeps its own table
    gpu.set_occlusion(None)
    assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == old_name
    assert np.array_equal(clone.render(cam, DEPTH), first) and clone.last_kernel_name() == OCCL
    clone.set_occlusion(None)
    assert np.array_equal(clone.render(cam, DEPTH), bare) and clone.last_kernel_name() == old_name


def test_two_seeds_differ_on_occluded_pixels_only(rtc):
    hs = ob.mix(rtc)
    cam = hs.camera(W, H)
    o = hs.occlusion()
    a, gpu, _ = check(rtc, hs, cam, occlusion=dict(o, seed=1))
    b, _, _ = check(rtc, hs, cam, occlusion=dict(o, seed=2))
    assert not np.array_equal(a, b)
    gpu.set_occlusion(None)
    bare = gpu.render(cam, DEPTH)
    gpu.set_occlusion(dict(o, seed=1))
    assert np.array_equal(gpu.render(cam, DEPTH), a)      # the table set again: the same bits
    # a pixel whose tree meets no material with a radius and an ambient term has the bits of the render without a table
    untouched = (a == bare).all(axis=2) & (b == bare).all(axis=2)
    assert untouched.any() and not untouched.all()
