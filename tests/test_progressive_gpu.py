"""Progressive rendering on the GPU (rtc_scene_set_sample_pass, rtc_scene_accumulate_device, Progressive): every later pass
against the checker (tests/cpp/progressive_oracle.cpp) within 1e-12 with equal ray counts and no overflow, pass 0 as
the renders before, the accumulation's sums, mean, rgba and noise bit for bit against their host restatement, splits,
clones, band clones, the limit on a real handle and rtch_scene_render's passes."""
import json
import os

import numpy as np
import pytest

import camera_binding as cb
import progressive_binding as pb
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12
SPLIT_TOL = 1e-14   # (tests/test_sampling_gpu.py: shares of a split frame's pixels added in another order)
HERE = os.path.dirname(os.path.abspath(__file__))
SOFT_SHADOWS = os.path.join(HERE, "golden", "area_scenes", "soft_shadows.json")
L_LIGHTS, L_ROOTS = limits.LIMITS["LDS"]["LIGHTS"], limits.LIMITS["LDS"]["ROOTS"]


def area_light(corner, uvec, vvec, steps, intensity=(1, 1, 1), jitter=True):
    return {"kind": "area", "corner": corner, "uvec": uvec, "usteps": steps, "vvec": vvec, "vsteps": steps,
            "intensity": intensity, "jitter": jitter}


def check(rtc, desc, lights, cam, smp, sample_pass, depth=5, light_seed=0, kernel=None):
    gpu = rtc.GpuScene(desc, lights=lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    gpu.set_sample_pass(sample_pass)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    if kernel is not None:
        assert gpu.last_kernel_name() == kernel
    want, counters = pb.PassScene(desc, lights).render(cam, depth, smp, sample_pass, light_seed=light_seed)
    delta = float(np.abs(got - want).max())
    assert delta <= TOL, f"max |delta| {delta}"
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    assert st["overflow"] == 0
    return got, gpu


# ---- later passes against the checker
PASSES = [1, 3]


@pytest.mark.parametrize("p", PASSES)
def test_grid_one_jittered(rtc, p):
    hs = rtc.HostScene.from_file("cover.json")
    check(rtc, hs.desc, hs.lights, hs.camera(96, 54), cb.sampling(1, True, seed=7), p, kernel="rtc_render_kernel_ms")


@pytest.mark.parametrize("p", PASSES)
def test_grid_two_with_a_lens(rtc, p):
    hs = rtc.HostScene.from_file("cover.json")
    check(rtc, hs.desc, hs.lights, hs.camera(96, 54), cb.sampling(2, True, aperture=0.15, focal_distance=6.0, seed=3), p,
          kernel="rtc_render_kernel_ms")


@pytest.mark.parametrize("p", PASSES)
def test_soft_shadows(rtc, p):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    check(rtc, hs.desc, hs.lights, hs.camera(100, 40), cb.sampling(2, True, seed=1), p, light_seed=9,
          kernel="rtc_render_kernel_area_ms")


@pytest.mark.parametrize("p", PASSES)
def test_default_sampling_with_a_jittered_area_light(rtc, p):
    """A later pass runs the sampling kernel under the default sampling: the area light gets new samples, the camera does not."""
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(100, 40)
    got, _ = check(rtc, hs.desc, hs.lights, cam, None, p, light_seed=4, kernel="rtc_render_kernel_area_ms")
    first = rtc.GpuScene(hs.desc, lights=hs.lights)
    first.set_light_seed(4)
    assert not np.array_equal(first.render(cam, 5), got)
    assert first.last_kernel_name() == "rtc_render_kernel_area"


@pytest.mark.parametrize("p", PASSES)
@pytest.mark.parametrize("name", ["csg_demo.json", "texture_demo.json"])
def test_csg_and_texture_worlds(rtc, name, p):
    hs = rtc.HostScene.from_file(name)
    check(rtc, hs.desc, hs.lights, hs.camera(64, 40), cb.sampling(1, True, seed=2), p, kernel="rtc_render_kernel_ms")


@pytest.mark.parametrize("p", PASSES)
def test_bigworld(rtc, p):
    hs = rtc.HostScene(limits._class_world("groups", L_ROOTS + 40).scene())
    assert hs.desc.n_roots > L_ROOTS
    check(rtc, hs.desc, hs.lights, hs.camera(64, 48), cb.sampling(2, True, seed=4), p, kernel="rtc_render_kernel_ms_bigworld")


# ---- the L / L + 1 table edges of lights and roots, point and area forms, at a later pass
@pytest.mark.parametrize("n, kernel", [(L_LIGHTS, "rtc_render_kernel_ms"), (L_LIGHTS + 1, "rtc_render_kernel_ms_bigworld")])
def test_table_edge_point_lights(rtc, n, kernel):
    hs = rtc.HostScene(limits.World(spheres=3, cubes=2, planes=1, lights=n, size=(48, 32)).scene())
    assert hs.desc.n_lights == n
    check(rtc, hs.desc, hs.lights, hs.camera(48, 32), cb.sampling(2, True, seed=5), 2, kernel=kernel)


@pytest.mark.parametrize("n, kernel", [(L_LIGHTS, "rtc_render_kernel_area_ms"), (L_LIGHTS + 1, "rtc_render_kernel_area_ms_bigworld")])
def test_table_edge_area_lights(rtc, n, kernel):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    lights = [area_light((-1 + 0.1 * i, 2, 4), (2, 0, 0), (0, 2, 0), 2, (0.1, 0.1, 0.1)) for i in range(n)]
    check(rtc, hs.desc, rtc.LightDesc.make(lights), hs.camera(48, 27), None, 2, light_seed=6, kernel=kernel)


@pytest.mark.parametrize("area", [False, True])
@pytest.mark.parametrize("extra", [0, 1])
def test_table_edge_roots(rtc, area, extra):
    hs = rtc.HostScene(limits._class_world("groups", L_ROOTS + extra).scene())
    assert hs.desc.n_roots == L_ROOTS + extra
    lights = hs.lights
    if area:
        lights = rtc.LightDesc.make(hs.lights.to_list()[:1] + [area_light((-2, 6, -6), (2, 0, 0), (0, 0, 2), 2, (0.5, 0.5, 0.5))])
    kernel = "rtc_render_kernel_" + ("area_" if area else "") + "ms" + ("_bigworld" if extra else "")
    check(rtc, hs.desc, lights, hs.camera(48, 32), cb.sampling(1, True, seed=8), 3, light_seed=2, kernel=kernel)


# ---- pass 0 through the accumulation is the render of before
@pytest.mark.parametrize("name, smp, kernel", [
    ("cover.json", None, None),                          # a simple world
    ("teapot.json", None, "rtc_render_kernel"),          # the general kernel
    (SOFT_SHADOWS, None, "rtc_render_kernel_area"),
    ("cover.json", cb.sampling(2, True, seed=3), "rtc_render_kernel_ms"),
])
def test_pass_zero_accumulated_is_render_device(rtc, name, smp, kernel):
    import torch
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(128, 72)
    plain = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        plain.set_sampling(smp)
    want = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()   # (torch fills it on its stream; the library writes it on the handle's)
    plain.render_device(cam, want.data_ptr(), 5)
    plain.synchronize()
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    prog = rtc.Progressive(gpu, cam, 5)
    assert prog.step() is None and prog.passes == 1
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == plain.last_kernel_name()
    if kernel is not None:
        assert gpu.last_kernel_name() == kernel
    w = want.cpu().numpy()
    assert np.array_equal(prog.mean().cpu().numpy(), w)
    assert np.array_equal(prog.sum.cpu().numpy(), w)
    assert np.array_equal(prog.rgba8().cpu().numpy(), rtc.canvas_rgba8(w))


# ---- the accumulation against its host restatement
def _noise(sumsq, mean, P):
    d = sumsq - P * ((mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2])
    return float(np.sqrt(np.maximum(d, 0.0).sum() / d.size / (3.0 * (P - 1) * P)))


def _rgba8_device(rtc, mean):
    import torch
    out = torch.zeros(mean.shape[:-1], dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()   # (rtc_rgba8_device takes a stream of its own, not the legacy default one)
    torch.cuda.synchronize()
    rtc.rgba8_device(mean.data_ptr(), mean.shape[0] * mean.shape[1], out.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint8).reshape(mean.shape[0], mean.shape[1], 4)


@pytest.mark.parametrize("name, size, smp", [
    ("cover.json", (96, 54), cb.sampling(1, True, seed=7)),
    (SOFT_SHADOWS, (95, 41), None),                       # (an odd pixel count: the wide form's last pixel alone)
])
def test_sums_mean_rgba_and_noise_bitwise(rtc, name, size, smp):
    import torch
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(*size)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    gpu.set_light_seed(11)
    prog = rtc.Progressive(gpu, cam, 5)
    P = 6
    frames, noises = [], []
    for i in range(P):
        noises.append(prog.step())
        torch.cuda.synchronize()
        frames.append(prog.frame.cpu().numpy().copy())
        assert gpu.last_kernel_name().endswith("ms") or i == 0
    assert noises[0] is None
    s = frames[0].copy()
    sq = (frames[0][..., 0] * frames[0][..., 0] + frames[0][..., 1] * frames[0][..., 1]) + frames[0][..., 2] * frames[0][..., 2]
    for f in frames[1:]:
        s = s + f
        sq = sq + ((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2])
    assert not np.array_equal(frames[1], frames[2])      # (the passes differ)
    assert np.array_equal(prog.sum.cpu().numpy(), s)
    assert np.array_equal(prog.sumsq.cpu().numpy(), sq)
    mean = s / P
    assert np.array_equal(prog.mean().cpu().numpy(), mean)
    assert np.array_equal(prog.rgba8().cpu().numpy(), _rgba8_device(rtc, prog.mean()))
    assert np.array_equal(prog.rgba8().cpu().numpy(), rtc.canvas_rgba8(mean))
    want = _noise(sq, mean, P)
    assert want > 0.0
    assert abs(noises[-1] - want) <= 1e-12 * want, (noises[-1], want)
    # a second call on the same inputs: the same bits; and the narrow form (8-byte aligned buffers) agrees to the bit
    n = cam.hsize * cam.vsize
    base_sum = torch.from_numpy(s - frames[-1]).cuda()   # (not the bits of the sum after P - 1 passes: any inputs will do)
    base_sq = torch.from_numpy(sq).cuda()
    frame = prog.frame
    outs = []
    for offset in (0, 0, 1):
        buf = torch.zeros(offset + 3 * n * 3 + n * 2 + 1, dtype=torch.float64, device="cuda")
        fr = buf[offset:offset + 3 * n]
        sm = buf[offset + 3 * n:offset + 6 * n]
        mn = buf[offset + 6 * n:offset + 9 * n]
        sqs = buf[offset + 9 * n:offset + 10 * n]
        noise = buf[offset + 10 * n:offset + 10 * n + 1]
        fr.copy_(frame.reshape(-1))
        sm.copy_(base_sum.reshape(-1))
        sqs.copy_(base_sq.reshape(-1))
        rgba = torch.zeros(n + 1, dtype=torch.int32, device="cuda")[offset:offset + n]
        a = rtc.Accum(fr.data_ptr(), n, P, sm.data_ptr(), sqs.data_ptr(), mn.data_ptr(), rgba.data_ptr(), noise.data_ptr())
        torch.cuda.synchronize()   # (the copies above ran on torch's stream; the call runs on the handle's)
        gpu.accumulate_device(a)
        gpu.synchronize()
        outs.append([t.cpu().numpy().copy() for t in (sm, sqs, mn, rgba, noise)])
    for x, y in zip(outs[0], outs[1]):                    # the same inputs twice: every output, the noise too
        assert x.tobytes() == y.tobytes()
    for x, y in zip(outs[0][:4], outs[2][:4]):            # the narrow form: the per-pixel outputs to the bit ...
        assert x.tobytes() == y.tobytes()
    assert abs(outs[2][4][0] - outs[0][4][0]) <= 1e-12 * outs[0][4][0]   # ... its noise partials cover other pixels


def test_tile_buffers_accumulate_as_a_length(rtc):
    """A rank accumulates its own tiles: n_pixels is only a length."""
    import torch
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(160, 96)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_light_seed(5)
    tw, th, n_tiles = 32, 32, 7
    tiles = [1, 4, 9, 2, 14, 0, 11]
    n = n_tiles * tw * th
    buf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    s = torch.zeros_like(buf)
    sq = torch.zeros((n_tiles, th, tw), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()   # (torch fills it on its stream; the library writes it on the handle's)
    frames = []
    for P in range(3):
        gpu.set_sample_pass(P)
        gpu.render_tile_list_device(cam, buf.data_ptr(), tw, th, tiles, 5)
        gpu.accumulate_device(rtc.Accum(buf.data_ptr(), n, P + 1, s.data_ptr(), sq.data_ptr(), None, None, None))
        gpu.synchronize()
        frames.append(buf.cpu().numpy().copy())
    assert np.array_equal(s.cpu().numpy(), (frames[0] + frames[1]) + frames[2])


# ---- splitting the frame at pass 2 changes nothing
@pytest.mark.parametrize("name, smp", [("cover.json", cb.sampling(2, True, seed=12)), (SOFT_SHADOWS, None)])
def test_splits_at_pass_two(rtc, name, smp):
    import torch
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(200, 120)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    gpu.set_light_seed(3)
    gpu.set_sample_pass(2)
    d = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()   # (torch fills it on its stream; the library writes it on the handle's)
    gpu.render_device(cam, d.data_ptr(), 5)
    gpu.synchronize()
    whole = d.cpu().numpy()
    want, _ = pb.PassScene(hs.desc, hs.lights).render(cam, 5, smp, 2, light_seed=3)
    assert float(np.abs(whole - want).max()) <= TOL

    def same(a, b):
        assert float(np.abs(a - b).max()) <= SPLIT_TOL
    rtc.set_option("host_bands", 3)
    try:
        same(gpu.render(cam, 5), whole)
    finally:
        rtc.set_option("host_bands", 0)
    tw, th = 48, 32
    tiles_x, tiles_y = -(-cam.hsize // tw), -(-cam.vsize // th)
    n_tiles = tiles_x * tiles_y
    buf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()   # (torch fills it on its stream; the library writes it on the handle's)
    gpu.render_tiles_device(cam, buf.data_ptr(), tw, th, 1, 2, n_tiles // 2, 5)
    gpu.synchronize()
    tiles = list(range(n_tiles))[::-1]
    lbuf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()   # (torch fills it on its stream; the library writes it on the handle's)
    gpu.render_tile_list_device(cam, lbuf.data_ptr(), tw, th, tiles, 5)
    gpu.synchronize()
    b, lb = buf.cpu().numpy(), lbuf.cpu().numpy()
    for k, t in enumerate(tiles):
        ty, tx = divmod(t, tiles_x)
        h, w = min(th, cam.vsize - ty * th), min(tw, cam.hsize - tx * tw)
        same(lb[k, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])
        if t % 2 == 1:
            same(b[(t - 1) // 2, :h, :w], whole[ty * th:ty * th + h, tx * tw:tx * tw + w])


# ---- clones, band clones, the limit
def test_clone_inherits_the_pass(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(96, 40)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_light_seed(8)
    gpu.set_sample_pass(5)
    clone = gpu.clone()
    want, _ = pb.PassScene(hs.desc, hs.lights).render(cam, 5, None, 5, light_seed=8)
    assert float(np.abs(clone.render(cam, 5) - want).max()) <= TOL
    assert clone.last_kernel_name() == "rtc_render_kernel_area_ms"


def test_setter_reaches_existing_band_clones(rtc):
    hs = rtc.HostScene.from_file("cover.json")
    cam = hs.camera(160, 96)
    gpu = rtc.GpuScene(hs.desc)
    smp = cb.sampling(1, True, seed=21)
    gpu.set_sampling(smp)
    rtc.set_option("host_bands", 3)
    try:
        first = gpu.render(cam, 5)          # makes the band clones, at pass 0
        gpu.set_sample_pass(4)
        got = gpu.render(cam, 5)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = pb.PassScene(hs.desc, hs.lights).render(cam, 5, smp, 4)
    assert float(np.abs(got - want).max()) <= TOL
    assert st["primary"] == counters["primary"] == cam.hsize * cam.vsize
    assert not np.array_equal(first, got)


def test_limit_on_a_real_handle(rtc):
    hs = rtc.HostScene.from_file("cover.json")
    gpu = rtc.GpuScene(hs.desc)
    gpu.set_sampling(cb.sampling(16, True))
    gpu.set_sample_pass(65535)                 # (65535 + 1) * 256 == 2^24
    with pytest.raises(rtc.RtcError):
        gpu.set_sample_pass(65536)
    gpu.set_sampling(cb.sampling(1, True))
    gpu.set_sample_pass(70000)
    with pytest.raises(rtc.RtcError):          # a grid that breaks the limit at the current pass
        gpu.set_sampling(cb.sampling(16, True))
    assert "sample pass" in rtc.hip_lib().rtc_last_error().decode()
    gpu.set_sampling(cb.sampling(2, True))     # (70001 * 4 fits)
    cam = hs.camera(32, 18)
    want, _ = pb.PassScene(hs.desc, hs.lights).render(cam, 5, cb.sampling(2, True), 70000)
    assert float(np.abs(gpu.render(cam, 5) - want).max()) <= TOL


# ---- rtch_scene_render's passes
def test_host_render_averages_the_files_passes(rtc):
    import torch
    with open(SOFT_SHADOWS) as f:
        scene = json.load(f)
    scene["camera"].update(width=80, height=32, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 4})
    hs = rtc.HostScene(json.dumps(scene))
    assert hs.passes() == 4
    out = np.zeros((32, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, 5, out.ctypes.data))
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(hs.sampling())
    prog = rtc.Progressive(gpu, hs.camera(), 5)
    noise = [prog.step() for _ in range(4)]
    torch.cuda.synchronize()
    assert noise[0] is None and all(v > 0.0 for v in noise[1:])
    assert np.array_equal(out, prog.mean().cpu().numpy())
