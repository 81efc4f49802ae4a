"""Camera samples per pixel on the GPU (rtc_scene_set_sampling; rtc_render_kernel_ms / _ms_bigworld / _area_ms /
_area_ms_bigworld), every case against the checker (tests/cpp/camera_oracle.cpp): max |delta| <= 1e-12 on every pixel,
primary, secondary and shadow_calls equal, no overflow."""
import os

import numpy as np
import pytest

import camera_binding as cb
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12
SPLIT_TOL = 1e-14   # a split frame hands other sub-trees to other lanes: shares added in another order
HERE = os.path.dirname(os.path.abspath(__file__))
SOFT_SHADOWS = os.path.join(HERE, "golden", "area_scenes", "soft_shadows.json")
L_LIGHTS, L_ROOTS = limits.LIMITS["LDS"]["LIGHTS"], limits.LIMITS["LDS"]["ROOTS"]


def area_light(corner, uvec, vvec, steps, intensity=(1, 1, 1), jitter=True):
    return {"kind": "area", "corner": corner, "uvec": uvec, "usteps": steps, "vvec": vvec, "vsteps": steps,
            "intensity": intensity, "jitter": jitter}


def check(rtc, desc, lights, cam, smp, depth=5, light_seed=0, kernel=None):
    gpu = rtc.GpuScene(desc, lights=lights)
    gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    if kernel is not None:
        assert gpu.last_kernel_name() == kernel
    want, counters = cb.CameraScene(desc, lights).render(cam, depth, smp, light_seed=light_seed)
    delta = float(np.abs(got - want).max())
    assert delta <= TOL, f"max |delta| {delta}"
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["primary"] == cam.hsize * cam.vsize * smp.grid * smp.grid
    assert st["overflow"] == 0
    return got, gpu


@pytest.mark.parametrize("grid", [2, 4])
@pytest.mark.parametrize("jitter", [False, True])
def test_grids(rtc, grid, jitter):
    hs = rtc.HostScene.from_file("cover.json")
    got, _ = check(rtc, hs.desc, hs.lights, hs.camera(96, 54), cb.sampling(grid, jitter, seed=7), kernel="rtc_render_kernel_ms")
    one = rtc.GpuScene(hs.desc).render(hs.camera(96, 54), 5)
    assert not np.array_equal(got, one)   # (the edges are smoothed: not the one-sample image)


def test_focal_blur(rtc):
    hs = rtc.HostScene.from_file("cover.json")
    check(rtc, hs.desc, hs.lights, hs.camera(96, 54), cb.sampling(2, True, aperture=0.15, focal_distance=6.0, seed=3),
          kernel="rtc_render_kernel_ms")


def test_area_light_with_a_jittered_grid(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    check(rtc, hs.desc, hs.lights, hs.camera(100, 40), cb.sampling(2, True, seed=1), light_seed=9,
          kernel="rtc_render_kernel_area_ms")


@pytest.mark.parametrize("name", ["csg_demo.json", "texture_demo.json"])
def test_csg_and_texture_worlds(rtc, name):
    hs = rtc.HostScene.from_file(name)
    check(rtc, hs.desc, hs.lights, hs.camera(64, 40), cb.sampling(2, True, seed=2), kernel="rtc_render_kernel_ms")


def test_bigworld(rtc):
    hs = rtc.HostScene(limits._class_world("groups", L_ROOTS + 40).scene())
    assert hs.desc.n_roots > L_ROOTS
    check(rtc, hs.desc, hs.lights, hs.camera(64, 48), cb.sampling(2, True, seed=4), kernel="rtc_render_kernel_ms_bigworld")


# ---- the L / L + 1 table edges of lights and roots, point and area forms
@pytest.mark.parametrize("n, kernel", [(L_LIGHTS, "rtc_render_kernel_ms"), (L_LIGHTS + 1, "rtc_render_kernel_ms_bigworld")])
def test_table_edge_point_lights(rtc, n, kernel):
    hs = rtc.HostScene(limits.World(spheres=3, cubes=2, planes=1, lights=n, size=(48, 32)).scene())
    assert hs.desc.n_lights == n
    check(rtc, hs.desc, hs.lights, hs.camera(48, 32), cb.sampling(2, True, seed=5), kernel=kernel)


@pytest.mark.parametrize("n, kernel", [(L_LIGHTS, "rtc_render_kernel_area_ms"), (L_LIGHTS + 1, "rtc_render_kernel_area_ms_bigworld")])
def test_table_edge_area_lights(rtc, n, kernel):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    lights = [area_light((-1 + 0.1 * i, 2, 4), (2, 0, 0), (0, 2, 0), 2, (0.1, 0.1, 0.1)) for i in range(n)]
    check(rtc, hs.desc, rtc.LightDesc.make(lights), hs.camera(48, 27), cb.sampling(2, True, seed=6), kernel=kernel)


@pytest.mark.parametrize("area", [False, True])
@pytest.mark.parametrize("extra", [0, 1])
def test_table_edge_roots(rtc, area, extra):
    hs = rtc.HostScene(limits._class_world("groups", L_ROOTS + extra).scene())
    assert hs.desc.n_roots == L_ROOTS + extra
    lights = hs.lights
    if area:
        lights = rtc.LightDesc.make(hs.lights.to_list()[:1] + [area_light((-2, 6, -6), (2, 0, 0), (0, 0, 2), 2, (0.5, 0.5, 0.5))])
    kernel = "rtc_render_kernel_" + ("area_" if area else "") + "ms" + ("_bigworld" if extra else "")
    check(rtc, hs.desc, lights, hs.camera(48, 32), cb.sampling(2, True, seed=8), kernel=kernel)


# ---- splitting the frame changes nothing
@pytest.mark.parametrize("name, tol", [("cover.json", SPLIT_TOL), (SOFT_SHADOWS, 0.0)])
def test_splits_render_the_same_image(rtc, name, tol):
    """cover has glass that reflects (sub-trees handed to other lanes: shares added in another order); soft_shadows has no
    transparent reflective material, so every split is bitwise."""
    import torch
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(200, 120)
    smp = cb.sampling(2, True, aperture=0.05, focal_distance=4.0, seed=12)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(smp)
    gpu.set_light_seed(3)
    d = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.float64, device="cuda")
    gpu.render_device(cam, d.data_ptr(), 5)
    gpu.synchronize()
    whole = d.cpu().numpy()
    want, _ = cb.CameraScene(hs.desc, hs.lights).render(cam, 5, smp, light_seed=3)
    assert float(np.abs(whole - want).max()) <= TOL

    def same(a, b):
        assert float(np.abs(a - b).max()) <= tol
    rtc.set_option("host_bands", 3)   # rtc_render's bands, on the handle and its band clones
    try:
        same(gpu.render(cam, 5), whole)
        assert gpu.last_kernel_name().endswith("ms")
    finally:
        rtc.set_option("host_bands", 0)
    # a rectangle of the image
    r = torch.zeros((40, 64, 3), dtype=torch.float64, device="cuda")
    gpu.render_device(cam, r.data_ptr(), 5, tile=(30, 50, 64, 40))
    gpu.synchronize()
    same(r.cpu().numpy(), whole[50:90, 30:94])
    # interleaved tiles and a tile list, un-permuted
    tw, th = 48, 32
    tiles_x, tiles_y = -(-cam.hsize // tw), -(-cam.vsize // th)
    n_tiles = tiles_x * tiles_y
    buf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    gpu.render_tiles_device(cam, buf.data_ptr(), tw, th, 1, 2, n_tiles // 2, 5)
    gpu.synchronize()
    tiles = list(range(n_tiles))[::-1]
    lbuf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    gpu.render_tile_list_device(cam, lbuf.data_ptr(), tw, th, tiles, 5)
    gpu.synchronize()
    b, lb = buf.cpu().numpy(), lbuf.cpu().numpy()
    for k, t in enumerate(tiles):
        ty, tx = divmod(t, tiles_x)
        h, w = min(th, cam.vsize - ty * th), min(tw, cam.hsize - tx * tw)
        same(lb[k, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
        if t % 2 == 1:
            same(b[(t - 1) // 2, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
    # a clone starts with its source's sampling (and light seed)
    clone = gpu.clone()
    same(clone.render(cam, 5), whole)
    assert clone.last_kernel_name() == gpu.last_kernel_name()


def test_rgba8_is_the_clamp_of_the_canvas(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(120, 60)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(cb.sampling(3, True, seed=2))
    assert np.array_equal(gpu.render_rgba8(cam, 5), rtc.canvas_rgba8(gpu.render(cam, 5)))


def test_setter_reaches_existing_band_clones(rtc):
    hs = rtc.HostScene.from_file("cover.json")
    cam = hs.camera(160, 96)
    gpu = rtc.GpuScene(hs.desc)
    smp = cb.sampling(2, True, seed=21)
    rtc.set_option("host_bands", 3)
    try:
        first = gpu.render(cam, 5)          # makes the band clones, one sample per pixel
        gpu.set_sampling(smp)
        got = gpu.render(cam, 5)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = cb.CameraScene(hs.desc, hs.lights).render(cam, 5, smp)
    assert float(np.abs(got - want).max()) <= TOL
    assert st["primary"] == counters["primary"] == 4 * cam.hsize * cam.vsize
    assert not np.array_equal(first, got)
    # an invalid setting changes nothing
    with pytest.raises(rtc.RtcError):
        gpu.set_sampling(0)
    assert float(np.abs(gpu.render(cam, 5) - want).max()) <= TOL


@pytest.mark.parametrize("name, tol", [("teapot.json", 0.0), ("cover.json", SPLIT_TOL), (SOFT_SHADOWS, 0.0)])
def test_sampling_kernel_with_one_sample_is_the_old_image(rtc, name, tol):
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(128, 72)
    old = rtc.GpuScene(hs.desc, lights=hs.lights)
    want = old.render(cam, 5)
    assert "ms" not in old.last_kernel_name()
    rtc.set_option("sampling_kernels", 1)
    try:
        gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
        got = gpu.render(cam, 5)
        st = gpu.stats()
        assert gpu.last_kernel_name() == ("rtc_render_kernel_area_ms" if name == SOFT_SHADOWS else "rtc_render_kernel_ms")
    finally:
        rtc.set_option("sampling_kernels", 0)
    assert float(np.abs(got - want).max()) <= tol
    assert st["primary"] == cam.hsize * cam.vsize and st["overflow"] == 0
    assert st["secondary"] == old.stats()["secondary"] and st["shadow_calls"] == old.stats()["shadow_calls"]


def test_reset_to_default_is_the_old_kernel(rtc):
    hs = rtc.HostScene.from_file("teapot.json")
    cam = hs.camera(128, 72)
    plain = rtc.GpuScene(hs.desc)
    want = plain.render(cam, 5)
    gpu = rtc.GpuScene(hs.desc)
    gpu.set_sampling(cb.sampling(2, True, aperture=0.1, focal_distance=5.0))
    gpu.render(cam, 5)
    assert gpu.last_kernel_name() == "rtc_render_kernel_ms"
    gpu.set_sampling(None)
    assert np.array_equal(gpu.render(cam, 5), want)
    assert gpu.last_kernel_name() == plain.last_kernel_name()
    assert gpu.stats()["primary"] == cam.hsize * cam.vsize


def test_host_render_applies_the_files_sampling(rtc):
    import json
    with open(SOFT_SHADOWS) as f:
        scene = json.load(f)
    scene["camera"].update(width=80, height=32, sampling={"grid": 2, "jitter": True, "seed": 4})
    hs = rtc.HostScene(json.dumps(scene))
    smp = hs.sampling()
    out = np.zeros((32, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, 5, out.ctypes.data))
    want, _ = cb.CameraScene(hs.desc, hs.lights).render(hs.camera(), 5, smp)
    assert float(np.abs(out - want).max()) <= TOL
