"""Motion blur on the GPU (rtc_scene_set_motion, the motion kernels): every moving render against the checker
(tests/cpp/motion_oracle.cpp) within 1e-12 with equal ray counts and no overflow - grids, a lens, an area light, every
kind of root, the root table's edge in both kernel forms, splits, clones, band clones, rgba8, passes and Progressive -,
the setter's refusals, the reset to static, the motion kernels on a static handle against the sampling kernels, and a
check that needs no checker: a small sphere's path across black."""
import json
import os

import numpy as np
import pytest

import camera_binding as cb
import motion_binding as mb
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12
SPLIT_TOL = 1e-14   # (tests/test_sampling_gpu.py: shares of a split frame's pixels added in another order)
HERE = os.path.dirname(os.path.abspath(__file__))
MOTION_MIX = os.path.join(HERE, "golden", "motion_scenes", "motion_mix.json")
SOFT_SHADOWS = os.path.join(HERE, "golden", "area_scenes", "soft_shadows.json")
L_ROOTS = limits.LIMITS["LDS"]["ROOTS"]


def check(rtc, desc, lights, cam, disp, smp=None, sample_pass=0, depth=5, light_seed=0, kernel="rtc_render_kernel_motion"):
    gpu = rtc.GpuScene(desc, lights=lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    if sample_pass:
        gpu.set_sample_pass(sample_pass)
    gpu.set_motion(disp)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    if kernel is not None:
        assert gpu.last_kernel_name() == kernel
    want, counters = mb.MotionScene(desc, lights).render(cam, depth, smp, disp, sample_pass, light_seed=light_seed)
    delta = float(np.abs(got - want).max())
    assert delta <= TOL, f"max |delta| {delta}"
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    assert st["overflow"] == 0
    return got, gpu


def one_moving(n_roots, r, d):
    disp = np.zeros((n_roots, 3))
    disp[r] = d
    return disp


# ---- sampling forms
@pytest.mark.parametrize("smp", [None, cb.sampling(2, True, seed=3), cb.sampling(2, True, aperture=0.08, focal_distance=6.0, seed=5)],
                         ids=["grid1", "grid2", "lens"])
def test_fixture_against_the_checker(rtc, smp):
    hs = rtc.HostScene.from_file(MOTION_MIX)
    check(rtc, hs.desc, hs.lights, hs.camera(96, 54), hs.motion(), smp)


def test_area_light_with_motion(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[2] = (0.4, 0.2, 0.0)      # the red sphere
    disp[3] = (-0.3, 0.0, 0.5)     # the blue sphere
    check(rtc, hs.desc, hs.lights, hs.camera(64, 26), disp, cb.sampling(2, True, seed=4), light_seed=9)


# ---- every kind of root
@pytest.mark.parametrize("name, root, d", [
    (MOTION_MIX, 0, (0.0, 0.3, 0.2)),                 # a plane
    (MOTION_MIX, 1, (0.9, 0.0, 0.0)),                 # a striped sphere (the pattern's point)
    (MOTION_MIX, 2, (0.0, 0.5, 0.4)),                 # a group
    (MOTION_MIX, 3, (-0.7, 0.0, 0.5)),                # a csg unit
    (SOFT_SHADOWS, 0, (0.5, -0.5, 0.0)),              # a cube (its "room" flag, if it had one, is cleared)
    ("teapot.json", 1, (0.0, 2.0, 1.0)),              # a teapot-sized group
    ("texture_demo.json", 1, (0.2, 0.1, -0.2)),       # a textured object
    ("csg_demo.json", 1, (0.3, 0.0, 0.2)),
])
def test_each_kind_of_root(rtc, name, root, d):
    hs = rtc.HostScene.from_file(name)
    assert hs.desc.n_roots > root
    _, gpu = check(rtc, hs.desc, hs.lights, hs.camera(64, 36), one_moving(hs.desc.n_roots, root, d), cb.sampling(2, True, seed=root + 1),
                   kernel=None)
    assert gpu.last_kernel_name().startswith("rtc_render_kernel_motion")


def test_point_lights_through_the_motion_kernel_without_sampling(rtc):
    """A point-only light table (zero area rows), the default sampling, pass 0: the image still depends on the time."""
    hs = rtc.HostScene.from_file("cover.json")
    cam = hs.camera(80, 45)
    disp = one_moving(hs.desc.n_roots, 2, (0.3, 0.0, 0.0))
    got, _ = check(rtc, hs.desc, hs.lights, cam, disp)
    assert not np.array_equal(got, rtc.GpuScene(hs.desc).render(cam, 5))


# ---- the root table's edge: RTC_LDS_ROOTS roots in LDS, one more in memory
@pytest.mark.parametrize("extra", [0, 1])
def test_table_edge_roots(rtc, extra):
    hs = rtc.HostScene(limits._class_world("groups", L_ROOTS + extra).scene())
    n = hs.desc.n_roots
    assert n == L_ROOTS + extra
    rng = np.random.default_rng(5)
    disp = np.where(rng.random((n, 1)) < 0.5, rng.uniform(-0.5, 0.5, (n, 3)), 0.0)
    disp[-1] = (0.3, 0.1, -0.2)    # (the last root of the table moves)
    kernel = "rtc_render_kernel_motion" + ("_bigworld" if extra else "")
    check(rtc, hs.desc, hs.lights, hs.camera(48, 32), disp, cb.sampling(2, True, seed=8), kernel=kernel)


# ---- splitting the frame changes nothing
def test_splits_render_the_same_image(rtc):
    import torch
    hs = rtc.HostScene.from_file(MOTION_MIX)
    cam = hs.camera(200, 120)
    smp = cb.sampling(2, True, seed=12)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(smp)
    gpu.set_motion(hs.motion())
    d = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_device(cam, d.data_ptr(), 5)
    gpu.synchronize()
    whole = d.cpu().numpy()
    want, _ = mb.MotionScene(hs.desc, hs.lights).render(cam, 5, smp, hs.motion())
    assert float(np.abs(whole - want).max()) <= TOL

    def same(a, b):
        assert float(np.abs(a - b).max()) <= SPLIT_TOL
    rtc.set_option("host_bands", 3)   # rtc_render's bands, on the handle and its band clones
    try:
        same(gpu.render(cam, 5), whole)
        assert gpu.last_kernel_name() == "rtc_render_kernel_motion"
    finally:
        rtc.set_option("host_bands", 0)
    r = torch.zeros((40, 64, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_device(cam, r.data_ptr(), 5, tile=(30, 50, 64, 40))
    gpu.synchronize()
    same(r.cpu().numpy(), whole[50:90, 30:94])
    tw, th = 48, 32
    tiles_x, tiles_y = -(-cam.hsize // tw), -(-cam.vsize // th)
    n_tiles = tiles_x * tiles_y
    buf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    lbuf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_tiles_device(cam, buf.data_ptr(), tw, th, 1, 2, n_tiles // 2, 5)
    gpu.synchronize()
    tiles = list(range(n_tiles))[::-1]
    gpu.render_tile_list_device(cam, lbuf.data_ptr(), tw, th, tiles, 5)
    gpu.synchronize()
    b, lb = buf.cpu().numpy(), lbuf.cpu().numpy()
    for k, t in enumerate(tiles):
        ty, tx = divmod(t, tiles_x)
        h, w = min(th, cam.vsize - ty * th), min(tw, cam.hsize - tx * tw)
        same(lb[k, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
        if t % 2 == 1:
            same(b[(t - 1) // 2, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
    # a clone starts with its source's motion
    clone = gpu.clone()
    same(clone.render(cam, 5), whole)
    assert clone.last_kernel_name() == "rtc_render_kernel_motion"
    # rgba8 is the clamp of the canvas
    assert np.array_equal(gpu.render_rgba8(cam, 5), rtc.canvas_rgba8(gpu.render(cam, 5)))


def test_setter_reaches_existing_band_clones(rtc):
    hs = rtc.HostScene.from_file(MOTION_MIX)
    cam = hs.camera(160, 96)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    rtc.set_option("host_bands", 3)
    try:
        first = gpu.render(cam, 5)          # makes the band clones, static
        gpu.set_motion(hs.motion())
        got = gpu.render(cam, 5)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = mb.MotionScene(hs.desc, hs.lights).render(cam, 5, None, hs.motion())
    assert float(np.abs(got - want).max()) <= TOL
    assert st["primary"] == counters["primary"] and st["shadow_calls"] == counters["shadow_calls"]
    assert not np.array_equal(first, got)


# ---- refusals change nothing; NULL (or all zeros) is static again, bit for bit
def test_refused_settings_and_reset(rtc):
    """(soft_shadows has no material both transparent and reflective: no pixel's shares are added in a schedule's order,
    so every comparison is bitwise)"""
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(96, 40)
    plain = rtc.GpuScene(hs.desc, lights=hs.lights)
    static = plain.render(cam, 5)
    n = hs.desc.n_roots
    motion = one_moving(n, 2, (0.4, 0.2, 0.0))
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_motion(motion)
    moving = gpu.render(cam, 5)
    assert gpu.last_kernel_name() == "rtc_render_kernel_motion"
    assert not np.array_equal(moving, static)
    for bad in (np.full((n, 3), np.nan), np.full((n, 3), np.inf), np.zeros((n + 1, 3)), np.zeros((n - 1, 3))):
        with pytest.raises(rtc.RtcError) as e:
            gpu.set_motion(bad)
        assert e.value.name == "InvalidArgument"
    bad = motion.copy()
    bad[2, 1] = -np.inf
    with pytest.raises(rtc.RtcError):
        gpu.set_motion(bad)
    assert np.array_equal(gpu.render(cam, 5), moving)
    assert gpu.last_kernel_name() == "rtc_render_kernel_motion"
    gpu.set_motion(None)
    assert np.array_equal(gpu.render(cam, 5), static)
    assert gpu.last_kernel_name() == plain.last_kernel_name()
    gpu.set_motion(np.zeros((n, 3)))
    assert np.array_equal(gpu.render(cam, 5), static)
    assert gpu.last_kernel_name() == plain.last_kernel_name()


# ---- passes draw new times
def test_later_pass_draws_new_times(rtc):
    hs = rtc.HostScene.from_file(MOTION_MIX)
    cam = hs.camera(64, 36)
    p0, _ = check(rtc, hs.desc, hs.lights, cam, hs.motion(), cb.sampling(1, True, seed=2), sample_pass=0)
    p3, _ = check(rtc, hs.desc, hs.lights, cam, hs.motion(), cb.sampling(1, True, seed=2), sample_pass=3)
    assert not np.array_equal(p0, p3)


def test_progressive_noise_falls_on_a_moving_scene(rtc):
    import torch
    hs = rtc.HostScene.from_file(MOTION_MIX)
    cam = hs.camera(96, 54)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_motion(hs.motion())
    prog = rtc.Progressive(gpu, cam, 5)
    noise = {}
    for i in range(64):
        v = prog.step()
        if prog.passes in (4, 16, 64):
            noise[prog.passes] = v
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == "rtc_render_kernel_motion"
    # the standard error of the mean halves for every fourfold number of passes (roughly)
    for a, b in ((4, 16), (16, 64)):
        ratio = noise[b] / noise[a]
        assert 0.35 < ratio < 0.7, (a, b, noise)


# ---- the motion kernels with every displacement zero are the sampling kernels' image
@pytest.mark.parametrize("name, kernel", [("teapot.json", "rtc_render_kernel_motion"), ("cover.json", "rtc_render_kernel_motion"),
                                          (SOFT_SHADOWS, "rtc_render_kernel_motion")])
def test_motion_kernels_on_a_static_handle(rtc, name, kernel):
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(128, 72)
    ms = rtc.GpuScene(hs.desc, lights=hs.lights)
    ms.set_sampling(cb.sampling(1, True, seed=3))
    want = ms.render(cam, 5)
    assert ms.last_kernel_name().endswith("_ms")
    rtc.set_option("motion_kernels", 1)
    try:
        gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
        gpu.set_sampling(cb.sampling(1, True, seed=3))
        got = gpu.render(cam, 5)
        st = gpu.stats()
        assert gpu.last_kernel_name() == kernel
    finally:
        rtc.set_option("motion_kernels", 0)
    assert float(np.abs(got - want).max()) <= TOL
    assert st["primary"] == cam.hsize * cam.vsize and st["overflow"] == 0
    assert st["secondary"] == ms.stats()["secondary"] and st["shadow_calls"] == ms.stats()["shadow_calls"]


# ---- without the checker: a small sphere moving across black
def test_swept_sphere_is_partly_lit_along_its_path_only(rtc):
    """A white, purely ambient sphere of radius 0.3 moves from x = -1.5 to x = 1.5 in front of nothing.  After 64 passes
    of 4 jittered samples, pixels the sphere covers at neither end of the shutter but crosses mid-way are lit at a
    fraction strictly between 0 and 1; pixels outside the swept region are exactly black."""
    import torch
    scene = {"camera": {"width": 80, "height": 40, "field-of-view": 1.0, "from": [0, 1, -5], "to": [0, 1, 0], "up": [0, 1, 0]},
             "lights": [{"point-light": {"position": [-10, 10, -10], "intensity": [1, 1, 1]}}],
             "objects": [{"type": {"sphere": {}}, "transform": [{"scale": [0.3, 0.3, 0.3]}, {"translate": [-1.5, 1, 0]}],
                          "motion": [3, 0, 0],
                          "material": {"pattern": {"type": {"solid": [1, 1, 1]}}, "ambient": 1, "diffuse": 0, "specular": 0}}]}
    hs = rtc.HostScene(json.dumps(scene))
    cam = hs.camera()
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(cb.sampling(2, True, seed=17))
    gpu.set_motion(hs.motion())
    prog = rtc.Progressive(gpu, cam, 5, noise=False)
    for _ in range(64):
        prog.step()
    torch.cuda.synchronize()
    img = prog.mean().cpu().numpy()[..., 0]
    # the centre of the frame: x = 0 at the sphere's height, crossed only in the middle of the shutter
    cy, cx = cam.vsize // 2, cam.hsize // 2
    mid = img[cy - 1:cy + 1, cx - 2:cx + 2]
    assert np.all((mid > 0.0) & (mid < 1.0)), mid
    # outside the swept capsule (|y - 1| > 0.3 in the object's plane, with a pixel of slack): black to the bit
    half = np.tan(0.5) * 5.0                # half the view's width at the sphere's distance
    px = 2 * half / cam.hsize
    ys = 1.0 + half * (cam.vsize / cam.hsize) - (np.arange(cam.vsize) + 0.5) * px
    outside = np.abs(ys - 1.0) > 0.3 + 3 * px
    assert outside.any() and np.all(img[outside] == 0.0)
    assert img.max() <= 1.0
