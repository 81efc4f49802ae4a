"""Spot lights on the GPU (rtc_scene_set_spots, the spot kernels): every spot-lit render against the checker
(tests/cpp/spot_oracle.cpp) within 1e-12 with equal ray counts and no overflow, the pixels where a hard edge meets a
rounding masked - sampling, a later pass, a moving root, a jittered area light beside the spots, the light table's edge
in both kernel forms -, the render entry points, clones and band clones, the setter's refusals and the reset, the spot
kernels on a handle without cones against the motion kernels, the shadow rays a narrow spot saves, Progressive, an
adaptive run and rtch_scene_render."""
import json
import math
import os

import numpy as np
import pytest

import camera_binding as cb
import spot_binding as sb
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12
SPLIT_TOL = 1e-14   # (tests/test_sampling_gpu.py: shares of a split frame's pixels added in another order)
HERE = os.path.dirname(os.path.abspath(__file__))
SPOT_MIX = os.path.join(HERE, "golden", "spot_scenes", "spot_mix.json")
SOFT_SHADOWS = os.path.join(HERE, "golden", "area_scenes", "soft_shadows.json")
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]


def compare(got, want, edge):
    keep = ~edge
    assert keep.mean() > 0.98
    delta = float(np.abs(got[keep] - want[keep]).max())
    assert delta <= TOL, f"max |delta| {delta}"


def check(rtc, desc, lights, cam, spots, smp=None, sample_pass=0, disp=None, depth=5, light_seed=0, kernel="rtc_render_kernel_spot"):
    gpu = rtc.GpuScene(desc, lights=lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    if sample_pass:
        gpu.set_sample_pass(sample_pass)
    if disp is not None:
        gpu.set_motion(disp)
    gpu.set_spots(spots)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    if kernel is not None:
        assert gpu.last_kernel_name() == kernel
    want, counters, edge = sb.SpotScene(desc, lights).render(cam, depth, smp, spots, disp, sample_pass, light_seed=light_seed)
    compare(got, want, edge)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    assert st["overflow"] == 0
    assert st["shadow_traced"] <= st["shadow_calls"]
    return got, gpu


def _mix(rtc):
    return rtc.HostScene.from_file(SPOT_MIX)


# ---- sampling forms, passes, motion, the jittered area light
@pytest.mark.parametrize("smp", [None, cb.sampling(2, True, aperture=0.08, focal_distance=6.0, seed=5)], ids=["default", "grid2-lens"])
def test_fixture_against_the_checker(rtc, smp):
    hs = _mix(rtc)
    check(rtc, hs.desc, hs.lights, hs.camera(96, 54), hs.spots(), smp, light_seed=3)


def test_later_pass(rtc):
    hs = _mix(rtc)
    cam = hs.camera(64, 36)
    p0, _ = check(rtc, hs.desc, hs.lights, cam, hs.spots(), cb.sampling(1, True, seed=2))
    p3, _ = check(rtc, hs.desc, hs.lights, cam, hs.spots(), cb.sampling(1, True, seed=2), sample_pass=3)
    assert not np.array_equal(p0, p3)


def test_moving_root_under_spots(rtc):
    hs = _mix(rtc)
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[1] = (0.6, 0.0, 0.3)      # the striped sphere, under the hard spot
    check(rtc, hs.desc, hs.lights, hs.camera(80, 45), hs.spots(), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)


def test_jittered_area_light_beside_spots(rtc):
    """soft_shadows' area light with a spot added before it, aimed at the red sphere"""
    with open(SOFT_SHADOWS) as f:
        scene = json.load(f)
    scene["lights"].insert(0, {"spot-light": {"position": [-3, 5, -3], "intensity": [0.6, 0.6, 0.6], "to": [0, 0.5, 0],
                                              "inner-angle": 0.2, "outer-angle": 0.35}})
    hs = rtc.HostScene(json.dumps(scene))
    assert list(hs.spots()["cone"]) == [1] + [0] * (hs.lights.n_lights - 1)
    check(rtc, hs.desc, hs.lights, hs.camera(64, 26), hs.spots(), cb.sampling(2, True, seed=4), light_seed=9)


# ---- the light table's edge: RTC_LDS_LIGHTS lights in LDS, one more in memory; the last light a spot
def _many_lights(n):
    lights = []
    for i in range(n - 1):
        a = 2 * math.pi * i / (n - 1)
        lights.append({"point-light": {"position": [6 * math.cos(a), 6 + i % 3, 6 * math.sin(a)], "intensity": [0.05, 0.05, 0.06]}})
    lights.append({"spot-light": {"position": [0, 6, -2], "intensity": [0.8, 0.7, 0.6], "to": [0.3, 0, 0.5],
                                  "inner-angle": 0.15, "outer-angle": 0.3}})
    objects = [{"type": {"plane": {}}, "material": {"pattern": {"type": {"solid": [0.9, 0.9, 0.9]}}, "specular": 0}},
               {"type": {"sphere": {}}, "transform": [{"translate": [0, 1, 0.5]}],
                "material": {"pattern": {"type": {"solid": [0.8, 0.3, 0.2]}}, "reflective": 0.2}}]
    cam = {"width": 48, "height": 32, "field-of-view": 1.0, "from": [0, 3, -6], "to": [0, 0.5, 0.5], "up": [0, 1, 0]}
    return json.dumps({"camera": cam, "lights": lights, "objects": objects})


@pytest.mark.parametrize("extra", [0, 1])
def test_table_edge_lights(rtc, extra):
    hs = rtc.HostScene(_many_lights(L_LIGHTS + extra))
    assert hs.lights.n_lights == L_LIGHTS + extra and hs.spots()["cone"][-1] == 1
    kernel = "rtc_render_kernel_spot" + ("_bigworld" if extra else "")
    check(rtc, hs.desc, hs.lights, hs.camera(), hs.spots(), cb.sampling(2, True, seed=8), kernel=kernel)


# ---- the entry points, a clone, band clones
def test_entry_points_and_a_clone_give_the_same_image(rtc):
    import torch
    hs = _mix(rtc)
    cam = hs.camera(160, 96)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    whole = gpu.render(cam, 5)
    assert gpu.last_kernel_name() == "rtc_render_kernel_spot"
    want, _, edge = sb.SpotScene(hs.desc, hs.lights).render(cam, 5, spots=hs.spots())
    compare(whole, want, edge)

    def same(a, b):
        assert float(np.abs(a - b).max()) <= SPLIT_TOL
    d = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_device(cam, d.data_ptr(), 5)
    gpu.synchronize()
    same(d.cpu().numpy(), whole)
    tw, th = 48, 32
    tiles_x, tiles_y = -(-cam.hsize // tw), -(-cam.vsize // th)
    tiles = list(range(tiles_x * tiles_y))[::-1]
    lbuf = torch.zeros((len(tiles), th, tw, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_tile_list_device(cam, lbuf.data_ptr(), tw, th, tiles, 5)
    gpu.synchronize()
    lb = lbuf.cpu().numpy()
    for k, t in enumerate(tiles):
        ty, tx = divmod(t, tiles_x)
        h, w = min(th, cam.vsize - ty * th), min(tw, cam.hsize - tx * tw)
        same(lb[k, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
    clone = gpu.clone()            # a clone starts with its source's spots
    same(clone.render(cam, 5), whole)
    assert clone.last_kernel_name() == "rtc_render_kernel_spot"
    rtc.set_option("host_bands", 3)
    try:
        same(gpu.render(cam, 5), whole)
    finally:
        rtc.set_option("host_bands", 0)


def test_setter_reaches_existing_band_clones(rtc):
    hs = _mix(rtc)
    cam = hs.camera(160, 96)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    rtc.set_option("host_bands", 3)
    try:
        first = gpu.render(cam, 5)          # makes the band clones, without cones
        gpu.set_spots(hs.spots())
        got = gpu.render(cam, 5)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters, edge = sb.SpotScene(hs.desc, hs.lights).render(cam, 5, spots=hs.spots())
    compare(got, want, edge)
    assert st["primary"] == counters["primary"] and st["shadow_calls"] == counters["shadow_calls"]
    assert not np.array_equal(first, got)


# ---- refusals change nothing; NULL (or every flag 0) is the old handle again, bit for bit
def test_refused_settings_and_reset(rtc):
    """(soft_shadows has no material both transparent and reflective: every comparison is bitwise)"""
    with open(SOFT_SHADOWS) as f:
        scene = json.load(f)
    scene["lights"].insert(0, {"spot-light": {"position": [-3, 5, -3], "intensity": [0.6, 0.6, 0.6], "to": [0, 0.5, 0],
                                              "outer-angle": 0.35}})
    hs = rtc.HostScene(json.dumps(scene))
    cam = hs.camera(96, 40)
    plain = rtc.GpuScene(hs.desc, lights=hs.lights)
    old = plain.render(cam, 5)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    spots = hs.spots()
    gpu.set_spots(spots)
    lit = gpu.render(cam, 5)
    assert gpu.last_kernel_name() == "rtc_render_kernel_spot"
    assert not np.array_equal(lit, old)
    n = hs.lights.n_lights
    bad = []
    a = [i for i in range(n) if hs.lights.kind[i] == rtc.RTC_LIGHT_AREA][0]
    area = {k: np.array(v) for k, v in sb.no_cones(n).items()}
    area["cone"][a], area["axis"][a] = 1, (0, -1, 0)          # a cone on the area light
    bad.append(area)
    for k, v in (("cone", 2), ("cos_inner", np.nan), ("cos_outer", 1.5)):
        b = {kk: np.array(vv) for kk, vv in spots.items()}
        b[k][0] = v
        bad.append(b)
    short = {k: np.array(v)[:n - 1] for k, v in spots.items()}
    bad.append(short)
    for b in bad:
        with pytest.raises(rtc.RtcError) as e:
            gpu.set_spots(b)
        assert e.value.name == "InvalidArgument"
    assert np.array_equal(gpu.render(cam, 5), lit)
    assert gpu.last_kernel_name() == "rtc_render_kernel_spot"
    gpu.set_spots(None)
    assert np.array_equal(gpu.render(cam, 5), old)
    assert gpu.last_kernel_name() == plain.last_kernel_name()
    gpu.set_spots(spots)
    gpu.set_spots(sb.no_cones(n))
    assert np.array_equal(gpu.render(cam, 5), old)
    assert gpu.last_kernel_name() == plain.last_kernel_name()


# ---- the spot kernels with every flag zero are the motion kernels' image
@pytest.mark.parametrize("name", ["cover.json", SOFT_SHADOWS])
def test_spot_kernels_without_cones_are_the_motion_kernels(rtc, name):
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(128, 72)
    smp = cb.sampling(1, True, seed=3)
    images, stats = [], []
    for option, kernel in (("motion_kernels", "rtc_render_kernel_motion"), ("spot_kernels", "rtc_render_kernel_spot")):
        rtc.set_option(option, 1)
        try:
            gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
            gpu.set_sampling(smp)
            images.append(gpu.render(cam, 5))
            stats.append(gpu.stats())
            assert gpu.last_kernel_name() == kernel
        finally:
            rtc.set_option(option, 0)
    assert np.array_equal(images[0], images[1])
    for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow"):
        assert stats[0][k] == stats[1][k], k


# ---- the skip: a narrow spot traces fewer shadow rays than the same point light
def test_narrow_spot_traces_fewer_shadow_rays(rtc):
    hs = rtc.HostScene.from_file("cover.json")
    cam = hs.camera(128, 72)
    n = hs.lights.n_lights
    pos = np.array([hs.lights.corner[k] for k in range(3)])
    spots = sb.no_cones(n)
    spots["cone"][0], spots["axis"][0] = 1, -pos        # aimed at the origin
    spots["cos_inner"][0], spots["cos_outer"][0] = math.cos(0.1), math.cos(0.12)
    got, gpu = check(rtc, hs.desc, hs.lights, cam, spots)
    plain = rtc.GpuScene(hs.desc, lights=hs.lights)
    plain.render(cam, 5)
    p, s = plain.stats(), gpu.stats()
    assert s["primary"] == p["primary"] and s["secondary"] == p["secondary"]
    assert s["shadow_calls"] < p["shadow_calls"] and s["shadow_traced"] < p["shadow_traced"]


# ---- Progressive, an adaptive run, rtch_scene_render
def test_progressive_noise_falls_on_a_spot_lit_scene(rtc):
    import torch
    hs = _mix(rtc)
    cam = hs.camera(96, 54)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(cb.sampling(1, True, seed=4))
    gpu.set_spots(hs.spots())
    prog = rtc.Progressive(gpu, cam, 5)
    noise = {}
    for _ in range(64):
        v = prog.step()
        if prog.passes in (4, 16, 64):
            noise[prog.passes] = v
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == "rtc_render_kernel_spot"
    for a, b in ((4, 16), (16, 64)):
        assert 0.35 < noise[b] / noise[a] < 0.7, (a, b, noise)


def test_adaptive_and_host_render_of_the_fixture(rtc):
    with open(SPOT_MIX) as f:
        scene = json.load(f)
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 6,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene))
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, 5, out.ctypes.data))
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(hs.sampling())
    gpu.set_spots(hs.spots())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == "rtc_render_kernel_spot"
    run = rtc.AdaptiveProgressive(gpu, hs.camera(), 5, a)
    run.run()
    mean = run.mean().cpu().numpy()
    assert np.array_equal(out, rgb) and np.array_equal(rgb, mean)
    assert passes.min() >= 2 and passes.max() <= 6
    # without "adaptive": rtch_scene_render is one rtc_render of the spot-lit handle
    plain = rtc.HostScene.from_file(SPOT_MIX)
    out1 = np.zeros((45, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, 80, 45, 5, out1.ctypes.data))
    g1 = rtc.GpuScene(plain.desc, lights=plain.lights)
    g1.set_spots(plain.spots())
    assert float(np.abs(out1 - g1.render(plain.camera(80, 45), 5)).max()) <= SPLIT_TOL
