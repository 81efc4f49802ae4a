"""Adaptive sampling on the GPU (rtc_scene_adaptive_*, rtc_render_adaptive, AdaptiveProgressive): synthetic frames through
the accumulation bit for bit against the checker (tests/cpp/adaptive_oracle.cpp) - sums, mean, rgba, tile noise and
passes, the active list and the largest noise - on both memory paths, edge tiles, a 1x1 image and 130k tiles; the full
list against rtc_scene_accumulate_device; rendered runs against the checker within 1e-12 with the same passes per tile;
determinism, the handle's own pass, clones, the index limit on a real handle, rtc_render_adaptive and rtch_scene_render."""
import json
import os

import numpy as np
import pytest

import adaptive_binding as ab
import camera_binding as cb
import motion_binding as mb
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12
HERE = os.path.dirname(os.path.abspath(__file__))
SOFT_SHADOWS = os.path.join(HERE, "golden", "area_scenes", "soft_shadows.json")
MOTION_MIX = os.path.join(HERE, "golden", "motion_scenes", "motion_mix.json")
L_ROOTS = limits.LIMITS["LDS"]["ROOTS"]


class DeviceState:
    """rtc_adaptive_state in torch tensors; `offset` bytes into each buffer (8: every [n][3] array off 16-byte alignment)."""

    def __init__(self, rtc, hsize, vsize, adaptive, offset=0):
        import torch
        self.torch = torch
        n, T = hsize * vsize, ab.n_tiles(hsize, vsize, adaptive.tile_w, adaptive.tile_h)
        e = offset // 8
        self._keep = []

        def buf(count, dtype):
            words = count * (2 if dtype == torch.float64 else 1) + 2 * e
            raw = torch.zeros(words, dtype=torch.int32, device="cuda")
            self._keep.append(raw)
            return raw[2 * e:].view(dtype)[:count]

        self.sum, self.sumsq, self.mean = buf(3 * n, torch.float64), buf(n, torch.float64), buf(3 * n, torch.float64)
        self.rgba, self.tile_passes, self.tile_noise = buf(n, torch.int32), buf(T, torch.int32), buf(T, torch.float64)
        self.active, self.n_active, self.max_noise = buf(T, torch.int32), buf(1, torch.int32), buf(1, torch.float64)
        self.c = rtc.AdaptiveState(*[t.data_ptr() for t in (self.sum, self.sumsq, self.mean, self.rgba, self.tile_passes, self.tile_noise,
                                                           self.active, self.n_active, self.max_noise)], 0)
        self.hsize, self.vsize = hsize, vsize

    def host(self):
        self.torch.cuda.synchronize()
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        n = int(u32(self.n_active)[0])
        h, w = self.vsize, self.hsize
        return dict(sum=self.sum.cpu().numpy().reshape(h, w, 3), sumsq=self.sumsq.cpu().numpy().reshape(h, w),
                    mean=self.mean.cpu().numpy().reshape(h, w, 3), rgba=u32(self.rgba).reshape(h, w),
                    tile_passes=u32(self.tile_passes), tile_noise=self.tile_noise.cpu().numpy(), active=u32(self.active)[:n],
                    max_noise=float(self.max_noise.cpu().numpy()[0]))


def _compare(got, chk, where):
    assert np.array_equal(got["tile_passes"], chk.tile_passes), where
    assert np.array_equal(got["tile_noise"], chk.tile_noise), (where, np.abs(got["tile_noise"] - chk.tile_noise).max())
    assert np.array_equal(got["active"], chk.active), where
    assert got["max_noise"] == chk.max_noise, where
    touched = np.zeros((chk.vsize, chk.hsize), dtype=bool)   # (pixels of tiles never accumulated are unset on the device)
    for t in np.nonzero(chk.tile_passes)[0]:
        x0, y0, w, h = ab.tile_rect(int(t), chk.hsize, chk.vsize, chk.a.tile_w, chk.a.tile_h)
        touched[y0:y0 + h, x0:x0 + w] = True
    for k in ("sum", "sumsq", "mean", "rgba"):
        assert np.array_equal(got[k][touched], getattr(chk, k)[touched]), (where, k)


def _synthetic(rng, hsize, vsize, tile_amp):
    """A frame whose noise amplitude is a function of the tile: some tiles converge at once, some never."""
    base = rng.random((vsize, hsize, 3))
    return base + tile_amp * rng.standard_normal((vsize, hsize, 3))


def _amp(hsize, vsize, a, rng):
    T = ab.n_tiles(hsize, vsize, a.tile_w, a.tile_h)
    levels = rng.choice([0.0, 0.003, 0.03, 0.3], size=T)
    amp = np.zeros((vsize, hsize, 1))
    for t in range(T):
        x0, y0, w, h = ab.tile_rect(t, hsize, vsize, a.tile_w, a.tile_h)
        amp[y0:y0 + h, x0:x0 + w] = levels[t]
    return amp


@pytest.mark.parametrize("hsize, vsize, tile, offset", [
    (64, 48, (16, 16), 0),     # the 16-byte path, tiles that divide the image
    (64, 45, (10, 7), 0),      # the 16-byte path, edge tiles on both sides
    (61, 45, (16, 16), 0),     # an odd width: one pixel at a time
    (64, 48, (9, 8), 0),       # an odd tile width
    (64, 48, (16, 16), 8),     # buffers off 16-byte alignment
    (1, 1, (16, 16), 0),       # one pixel, one tile
    (33, 17, (1, 1), 0),       # one-pixel tiles
    (70, 40, (1024, 3), 0),    # a tile wider than the image, 1024 lanes
])
def test_synthetic_rounds_match_the_checker_bitwise(rtc, hsize, vsize, tile, offset):
    import torch
    rng = np.random.default_rng(hsize * 7 + vsize + offset)
    a = rtc.Adaptive(tile[0], tile[1], 2, 6, 0.01)
    gpu = rtc.GpuScene(rtc.HostScene.from_file("cover.json").desc)
    dev = DeviceState(rtc, hsize, vsize, a, offset)
    gpu.adaptive_begin(hsize, vsize, a, dev.c)
    chk = ab.State(hsize, vsize, a)
    amp = _amp(hsize, vsize, a, rng)
    frame_raw = torch.zeros(a.tile_w * a.tile_h * 3 * chk.tile_passes.size * 2 + 2, dtype=torch.int32, device="cuda")
    frame_off = offset // 4
    rounds = 0
    while True:
        tiles = chk.active
        if len(tiles) == 0:
            break
        if rounds == 2 and len(tiles) > 2:
            tiles = tiles[::2]     # (a list the stopping rule did not make: any distinct tiles, here every other one)
        frame = chk.compact(_synthetic(rng, hsize, vsize, amp), tiles)
        flat = torch.from_numpy(frame.reshape(-1)).cuda()
        dframe = frame_raw[frame_off:frame_off + 2 * flat.numel()].view(torch.float64)
        dframe.copy_(flat)
        dtiles = torch.from_numpy(tiles.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        gpu.adaptive_accumulate_device(hsize, vsize, a, dev.c, dframe.data_ptr(), dtiles.data_ptr(), len(tiles))
        chk.accumulate(frame, tiles)
        _compare(dev.host(), chk, f"round {rounds}")
        rounds += 1
    assert rounds >= 2 and chk.tile_passes.max() <= 6


def test_large_tile_count_matches_the_checker(rtc):
    """3840 x 2160 in 8 x 8 tiles: 129 600 tiles through the one-block scan."""
    import torch
    hsize, vsize = 3840, 2160
    a = rtc.Adaptive(8, 8, 2, 3, 0.05)
    T = ab.n_tiles(hsize, vsize, 8, 8)
    assert T == 129600
    rng = np.random.default_rng(5)
    gpu = rtc.GpuScene(rtc.HostScene.from_file("cover.json").desc)
    dev = DeviceState(rtc, hsize, vsize, a)
    gpu.adaptive_begin(hsize, vsize, a, dev.c)
    chk = ab.State(hsize, vsize, a)
    levels = np.where(rng.random((vsize // 8, hsize // 8)) < 0.3, 0.2, 0.0)
    amp = np.repeat(np.repeat(levels, 8, axis=0), 8, axis=1)[..., None]
    for r in range(3):
        tiles = chk.active
        if len(tiles) == 0:
            break
        img = rng.random((vsize, hsize, 3)) + amp * rng.standard_normal((vsize, hsize, 3))
        # (the compact frame of tiles in row-major order, built without a Python loop over 130k tiles)
        blocks = img.reshape(vsize // 8, 8, hsize // 8, 8, 3).transpose(0, 2, 1, 3, 4).reshape(T, 8, 8, 3)
        frame = np.ascontiguousarray(blocks[tiles])
        dframe = torch.from_numpy(frame.reshape(-1)).cuda()
        dtiles = torch.from_numpy(tiles.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        gpu.adaptive_accumulate_device(hsize, vsize, a, dev.c, dframe.data_ptr(), dtiles.data_ptr(), len(tiles))
        chk.accumulate(frame, tiles)
        got = dev.host()
        assert np.array_equal(got["tile_noise"], chk.tile_noise) and np.array_equal(got["active"], chk.active), r
        assert got["max_noise"] == chk.max_noise
        assert np.array_equal(got["sum"], chk.sum) and np.array_equal(got["rgba"], chk.rgba)
    assert 0 < len(chk.active) < T or r == 2


@pytest.mark.parametrize("hsize, vsize", [(64, 48), (61, 45)])
def test_the_full_list_is_the_progressive_accumulation(rtc, hsize, vsize):
    """Every tile every round: sum, mean and rgba are rtc_scene_accumulate_device's bits on the same frames."""
    import torch
    a = rtc.Adaptive(16, 16, 3, 3, 0.0)
    T = ab.n_tiles(hsize, vsize, 16, 16)
    gpu = rtc.GpuScene(rtc.HostScene.from_file("cover.json").desc)
    dev = DeviceState(rtc, hsize, vsize, a)
    gpu.adaptive_begin(hsize, vsize, a, dev.c)
    n = hsize * vsize
    acc = {k: torch.empty(s, dtype=d, device="cuda") for k, s, d in
           [("sum", 3 * n, torch.float64), ("sumsq", n, torch.float64), ("mean", 3 * n, torch.float64), ("rgba", n, torch.int32)]}
    rng = np.random.default_rng(3)
    chk = ab.State(hsize, vsize, a)
    tiles = np.arange(T, dtype=np.uint32)
    dtiles = torch.from_numpy(tiles.astype(np.int32)).cuda()
    for p in range(1, 4):
        img = rng.random((vsize, hsize, 3)) * 2
        whole = torch.from_numpy(img.reshape(-1)).cuda()
        compact = torch.from_numpy(chk.compact(img, tiles).reshape(-1)).cuda()
        torch.cuda.synchronize()
        gpu.accumulate_device(rtc.Accum(whole.data_ptr(), n, p, acc["sum"].data_ptr(), acc["sumsq"].data_ptr(), acc["mean"].data_ptr(),
                                        acc["rgba"].data_ptr(), None))
        gpu.adaptive_accumulate_device(hsize, vsize, a, dev.c, compact.data_ptr(), dtiles.data_ptr(), T)
        gpu.synchronize()
        got = dev.host()
        for k in ("sum", "sumsq", "mean"):
            assert np.array_equal(got[k].reshape(-1), acc[k].cpu().numpy()), (p, k)
        assert np.array_equal(got["rgba"].reshape(-1), acc["rgba"].cpu().numpy().view(np.uint32)), p
    assert len(got["active"]) == 0 and np.all(got["tile_passes"] == 3)


# ---- rendered runs against the checker
def _threshold(frames, hsize, vsize, a):
    """A threshold halfway between two neighbouring distinct tile noises (any tile, any pass count min .. max), near their
    median: no decision of the run sits on a tie."""
    values = []
    for t in range(ab.n_tiles(hsize, vsize, a.tile_w, a.tile_h)):
        x0, y0, w, h = ab.tile_rect(t, hsize, vsize, a.tile_w, a.tile_h)
        s, q = np.zeros((h, w, 3)), np.zeros((h, w))
        for p, f in enumerate(frames[:a.max_passes], start=1):
            c = f[y0:y0 + h, x0:x0 + w]
            s, q = s + c, q + (c ** 2).sum(axis=2)
            if p >= a.min_passes:
                m = s / p
                values.append(np.sqrt(np.maximum(0.0, q - p * (m ** 2).sum(axis=2)).sum() / (w * h) / (3 * (p - 1) * p)))
    v = np.unique(np.array(values))
    v = v[v > 0]
    assert len(v) >= 4, v
    gaps = [(v[i + 1] - v[i], i) for i in range(len(v) // 4, 3 * len(v) // 4 + 1) if i + 1 < len(v)]
    g, i = max(gaps)
    assert g > 1e-9 * v[i + 1]
    return float((v[i] + v[i + 1]) / 2)


def _rendered(rtc, gpu, cam, render_pass, min_passes=2, max_passes=6, tile=16, depth=5):
    a0 = rtc.Adaptive.make(0.0, max_passes, min_passes, tile)
    frames = [render_pass(R) for R in range(max_passes)]
    a = rtc.Adaptive.make(_threshold(frames, cam.hsize, cam.vsize, a0), max_passes, min_passes, tile)
    chk = ab.run(lambda R: frames[R], cam.hsize, cam.vsize, a)
    run = rtc.AdaptiveProgressive(gpu, cam, depth, a)
    rounds = run.run()
    mean = run.mean().cpu().numpy()
    passes = run.tile_passes().cpu().numpy().view(np.uint32)
    assert np.array_equal(passes, chk.tile_passes)
    delta = float(np.abs(mean - chk.mean).max())
    assert delta <= TOL, delta
    assert rounds == chk.rounds and len(set(passes.tolist())) >= 2, passes
    st = gpu.stats()
    assert st["overflow"] == 0
    return a, mean, passes


def test_soft_shadows_against_the_checker(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(100, 40)
    smp = cb.sampling(2, True, seed=1)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(smp)
    gpu.set_light_seed(9)
    chk = ab.PassScene(hs.desc, hs.lights)
    _rendered(rtc, gpu, cam, lambda R: chk.render(cam, 5, smp, R, light_seed=9), max_passes=8)


def test_cover_with_jitter_and_a_lens_against_the_checker(rtc):
    hs = rtc.HostScene.from_file("cover.json")
    cam = hs.camera(96, 54)
    smp = cb.sampling(2, True, aperture=0.15, focal_distance=6.0, seed=3)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(smp)
    chk = ab.PassScene(hs.desc, hs.lights)
    _rendered(rtc, gpu, cam, lambda R: chk.render(cam, 5, smp, R), min_passes=3, max_passes=7, tile=(16, 8))


def test_a_moving_scene_against_the_checker(rtc):
    hs = rtc.HostScene.from_file(MOTION_MIX)
    disp = hs.motion()
    assert np.any(disp != 0)
    cam = hs.camera(64, 40)
    smp = cb.sampling(1, True, seed=6)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(smp)
    gpu.set_motion(disp)
    chk = mb.MotionScene(hs.desc, hs.lights)
    _rendered(rtc, gpu, cam, lambda R: chk.render(cam, 5, smp, disp, R)[0], max_passes=6, tile=8)


def test_a_bigworld_scene_against_the_checker(rtc):
    hs = rtc.HostScene(limits._class_world("groups", L_ROOTS + 40).scene())
    assert hs.desc.n_roots > L_ROOTS
    cam = hs.camera(64, 48)
    smp = cb.sampling(2, True, seed=4)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(smp)
    chk = ab.PassScene(hs.desc, hs.lights)
    _rendered(rtc, gpu, cam, lambda R: chk.render(cam, 5, smp, R), max_passes=5, tile=16)


# ---- determinism, the handle's pass, clones, the limit
def _soft(rtc, w=80, h=32):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(cb.sampling(1, True, seed=2))
    gpu.set_light_seed(5)
    return hs, gpu, hs.camera(w, h)


def _run_bits(rtc, gpu, cam, a):
    run = rtc.AdaptiveProgressive(gpu, cam, 5, a)
    run.run()
    return (run.mean().cpu().numpy(), run.rgba8().cpu().numpy(), run.tile_passes().cpu().numpy(), run.tile_noise.cpu().numpy(),
            run.sum.cpu().numpy())


def test_two_runs_and_a_clone_give_the_same_bits(rtc):
    hs, gpu, cam = _soft(rtc)
    a = rtc.Adaptive.make(0.004, 8, 2, 16)
    first = _run_bits(rtc, gpu, cam, a)
    second = _run_bits(rtc, gpu, cam, a)
    clone = _run_bits(rtc, gpu.clone(), cam, a)
    for x, y, z in zip(first, second, clone):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert len(set(first[2].tolist())) >= 2, first[2]


def test_the_handle_s_own_pass_is_left_alone(rtc):
    hs, gpu, cam = _soft(rtc)
    gpu.set_sample_pass(3)
    before = gpu.render(cam, 5)
    _run_bits(rtc, gpu, cam, rtc.Adaptive.make(0.004, 6, 2, 16))
    assert np.array_equal(gpu.render(cam, 5), before)
    fresh = rtc.GpuScene(hs.desc, lights=hs.lights)
    fresh.set_sampling(cb.sampling(1, True, seed=2))
    fresh.set_light_seed(5)
    fresh.set_sample_pass(3)
    assert np.array_equal(fresh.render(cam, 5), before)
    # ... and a run does not depend on the pass the handle was left at
    gpu.set_sample_pass(0)
    a = rtc.Adaptive.make(0.004, 6, 2, 16)
    zero = _run_bits(rtc, gpu, cam, a)
    gpu.set_sample_pass(5)
    assert all(np.array_equal(x, y) for x, y in zip(zero, _run_bits(rtc, gpu, cam, a)))


def test_the_index_limit_on_a_real_handle(rtc):
    """grid 16 (256 samples): max_passes 65536 is accepted, 65537 refused with nothing changed."""
    import torch
    hs, gpu, cam = _soft(rtc, 32, 16)
    gpu.set_sampling(cb.sampling(16, True, seed=1))
    dev = DeviceState(rtc, 32, 16, rtc.Adaptive.make(0.1, 2, 2, 16))
    dev.n_active.fill_(-1)
    torch.cuda.synchronize()
    dev.c.round = 9
    with pytest.raises(rtc.RtcError) as e:
        gpu.adaptive_begin(32, 16, rtc.Adaptive.make(0.1, 65537, 2, 16), dev.c)
    assert "sample indices" in str(e.value)
    assert dev.c.round == 9 and int(dev.n_active.cpu()[0]) == -1
    gpu.adaptive_begin(32, 16, rtc.Adaptive.make(0.1, 65536, 2, 16), dev.c)
    gpu.synchronize()
    assert dev.c.round == 0 and int(dev.n_active.cpu()[0]) == 2


def test_a_finished_run_renders_nothing(rtc):
    hs, gpu, cam = _soft(rtc, 40, 16)
    run = rtc.AdaptiveProgressive(gpu, cam, 5, rtc.Adaptive.make(1e9, 3, 3, 16))
    assert [run.step() for _ in range(3)] == [3, 3, 0]
    gpu.synchronize()
    primary = gpu.stats()["primary"]
    assert run.step() == 0 and run.rounds == 3
    assert gpu.stats()["primary"] == primary
    assert np.all(run.tile_passes().cpu().numpy() == 3)


# ---- the synchronous driver and the host library
def test_render_adaptive_is_the_device_path(rtc):
    hs, gpu, cam = _soft(rtc)
    a = rtc.Adaptive.make(0.004, 8, 2, (16, 8))
    rgb, passes = gpu.render_adaptive(cam, a)
    mean, _, dev_passes, _, _ = _run_bits(rtc, gpu, cam, a)
    assert np.array_equal(rgb, mean) and np.array_equal(passes, dev_passes.view(np.uint32))


def test_host_render_applies_the_files_adaptive(rtc):
    with open(SOFT_SHADOWS) as f:
        scene = json.load(f)
    scene["camera"].update(width=80, height=32, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 8,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 8]}})
    hs = rtc.HostScene(json.dumps(scene))
    a = hs.adaptive()
    assert a.to_dict() == {"tile_w": 16, "tile_h": 8, "min_passes": 2, "max_passes": 8, "threshold": 0.004}
    out = np.zeros((32, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, 5, out.ctypes.data))
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert np.array_equal(out, rgb)
    assert passes.min() >= 2 and passes.max() <= 8
