"""Area lights on the GPU (rtc_scene_create_with_lights, rtc_render_kernel_area / _area_bigworld), every case against
the checker (tests/cpp/area_oracle.cpp): max |delta| <= 1e-12 on every pixel, shadow_calls equal, no overflow.  One flipped
shadow sample of an 8x8 light moves a pixel by ~1/64."""
import ctypes as C
import os

import numpy as np
import pytest

import area_binding as ab
import oracle_binding as ob

pytestmark = pytest.mark.gpu

TOL = 1e-12
# (beside the point-light scenes, not among them: the oracle's own scene parser, which every scene there is checked
# against, knows point lights only)
SOFT_SHADOWS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "area_scenes", "soft_shadows.json")


def area_light(corner, uvec, vvec, steps, intensity=(1, 1, 1), jitter=True):
    return {"kind": "area", "corner": corner, "uvec": uvec, "usteps": steps, "vvec": vvec, "vsteps": steps,
            "intensity": intensity, "jitter": jitter}


def check(rtc, desc, lights, cam, depth=5, seed=None, kernel=None):
    gpu = rtc.GpuScene(desc, lights=lights)
    if seed is not None:
        gpu.set_light_seed(seed)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    if kernel is not None:
        assert gpu.last_kernel_name() == kernel
    want, counters = ab.AreaScene(desc, lights).render(cam, depth, seed=seed or 0)
    delta = float(np.abs(got - want).max())
    assert delta <= TOL, f"max |delta| {delta}"
    assert st["shadow_calls"] == counters["shadow_calls"] and st["secondary"] == counters["secondary"]
    assert st["overflow"] == 0
    return got, gpu


@pytest.mark.parametrize("jitter", [True, False])
def test_soft_shadows(rtc, jitter):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    lights = hs.lights.to_list()
    lights[0]["jitter"] = jitter
    got, gpu = check(rtc, hs.desc, rtc.LightDesc.make(lights), hs.camera(160, 90), kernel="rtc_render_kernel_area")
    assert gpu.stats()["shadow_traced"] <= gpu.stats()["shadow_calls"]
    assert gpu.stats()["shadow_traced"] > 0


def test_one_sample_equals_a_point_light(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(160, 90)
    lights = rtc.LightDesc.make([area_light((-1, 2, 4), (2, 0, 0), (0, 2, 0), 1, (1.5, 1.5, 1.5), jitter=False)])
    got, _ = check(rtc, hs.desc, lights, cam)
    desc = rtc.SceneDesc.from_buffer_copy(hs.desc)
    pos = (C.c_double * 3)(0.0, 3.0, 4.0)
    rgb = (C.c_double * 3)(1.5, 1.5, 1.5)
    desc.n_lights, desc.light_pos, desc.light_rgb = 1, pos, rgb
    want, _ = ob.OracleScene(desc).render(cam, 5)
    assert float(np.abs(got - want).max()) <= TOL


def test_mixed_lights(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    lights = rtc.LightDesc.make([{"kind": "point", "position": (-10, 10, -10), "intensity": (0.3, 0.3, 0.3)},
                                 area_light((-1, 2, 4), (2, 0, 0), (0, 2, 0), 4),
                                 {"kind": "point", "position": (5, 5, -5), "intensity": (0.2, 0.1, 0.3)}])
    check(rtc, hs.desc, lights, hs.camera(96, 54), seed=3)


@pytest.mark.parametrize("name", ["teapot.json", "csg_demo.json"])
def test_other_worlds_with_an_area_light(rtc, name):
    hs = rtc.HostScene.from_file(name)
    p = hs.array("light_pos", hs.desc.n_lights, 3)[0]
    rgb = hs.array("light_rgb", hs.desc.n_lights, 3)[0]
    lights = rtc.LightDesc.make([area_light((p[0] - 0.5, p[1], p[2] - 0.5), (1, 0, 0), (0, 0, 1), 4, tuple(rgb))])
    check(rtc, hs.desc, lights, hs.camera(64, 48), kernel="rtc_render_kernel_area")


@pytest.mark.parametrize("n, kernel", [(16, "rtc_render_kernel_area"), (17, "rtc_render_kernel_area_bigworld")])
def test_table_edge(rtc, n, kernel):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    lights = [area_light((-1 + 0.1 * i, 2, 4), (2, 0, 0), (0, 2, 0), 2, (0.1, 0.1, 0.1)) for i in range(n)]
    check(rtc, hs.desc, rtc.LightDesc.make(lights), hs.camera(48, 27), kernel=kernel)


def test_every_entry_point_renders_the_same_bits(rtc):
    import torch
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    lights = hs.lights
    cam = hs.camera(200, 120)
    gpu = rtc.GpuScene(hs.desc, lights=lights)
    gpu.set_light_seed(11)
    whole = gpu.render(cam, 5)
    rtc.set_option("host_bands", 3)
    try:
        banded = gpu.render(cam, 5)
    finally:
        rtc.set_option("host_bands", 0)
    assert np.array_equal(banded, whole)
    # rgba8
    assert np.array_equal(gpu.render_rgba8(cam, 5), rtc.canvas_rgba8(whole))
    # a tile of the image, on the device
    d = torch.zeros((40, 64, 3), dtype=torch.float64, device="cuda")
    gpu.render_device(cam, d.data_ptr(), 5, tile=(30, 50, 64, 40))
    gpu.synchronize()
    assert np.array_equal(d.cpu().numpy(), whole[50:90, 30:94])
    # tiles, interleaved and listed
    tw, th = 48, 32
    tiles_x, tiles_y = -(-cam.hsize // tw), -(-cam.vsize // th)
    n_tiles = tiles_x * tiles_y
    buf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    gpu.render_tiles_device(cam, buf.data_ptr(), tw, th, 1, 2, (n_tiles - 1 + 1) // 2, 5)
    gpu.synchronize()
    tiles = list(range(n_tiles))[::-1]
    lbuf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    gpu.render_tile_list_device(cam, lbuf.data_ptr(), tw, th, tiles, 5)
    gpu.synchronize()
    b, lb = buf.cpu().numpy(), lbuf.cpu().numpy()
    for k, t in enumerate(tiles):
        ty, tx = divmod(t, tiles_x)
        h, w = min(th, cam.vsize - ty * th), min(tw, cam.hsize - tx * tw)
        assert np.array_equal(lb[k, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
        if t % 2 == 1:
            assert np.array_equal(b[(t - 1) // 2, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
    # a clone starts with its source's seed
    assert np.array_equal(gpu.clone().render(cam, 5), whole)


def test_seeds(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(120, 68)
    a, b = rtc.GpuScene(hs.desc, lights=hs.lights), rtc.GpuScene(hs.desc, lights=hs.lights)
    a.set_light_seed(5)
    b.set_light_seed(5)
    img5 = a.render(cam, 5)
    assert np.array_equal(img5, b.render(cam, 5))
    b.set_light_seed(6)
    img6 = b.render(cam, 5)
    assert not np.array_equal(img5, img6)
    chk = ab.AreaScene(hs.desc, hs.lights)
    for seed, img in ((5, img5), (6, img6)):
        assert float(np.abs(img - chk.render(cam, 5, seed=seed)[0]).max()) <= TOL
    # jitter off: the seed does not matter
    lights = hs.lights.to_list()
    lights[0]["jitter"] = False
    off = rtc.LightDesc.make(lights)
    c = rtc.GpuScene(hs.desc, lights=off)
    c.set_light_seed(1)
    one = c.render(cam, 5)
    c.set_light_seed(2)
    assert np.array_equal(one, c.render(cam, 5))


@pytest.mark.parametrize("name", ["cover.json", "teapot.json"])
def test_point_only_table_is_the_old_path(rtc, name):
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(160, 90)
    a = rtc.GpuScene(hs.desc)
    b = rtc.GpuScene(hs.desc, lights=hs.lights)
    ia, ib = a.render(cam, 5), b.render(cam, 5)
    assert a.last_kernel_name() == b.last_kernel_name()
    assert "area" not in b.last_kernel_name()
    assert np.array_equal(ia, ib)
