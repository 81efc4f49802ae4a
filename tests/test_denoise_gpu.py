"""The denoiser on the GPU (rtc_denoise_device, the kernels of csrc/rtc_denoise.hip): both kernel forms -
the tiled one and, under option "denoise_naive", the literal one - against the checker (tests/cpp/denoise_oracle.cpp) within
1e-12 * max(1, |value|) per channel and against each other, `rgba` against rtc_rgba8_device of the result to the bit, at
sizes around the tile and with windows and halos larger than the image; an adaptive run's tile_passes with a tile at one
pass; Progressive.denoised() and AdaptiveProgressive.denoised() on the fixture emitters_mix.json against the checker and
against the mean of GPU passes 32 .. 159; rtc_render_denoised and rtch_scene_render of a file with the key; and the two forms
on a rendered 480 x 270 mean.

Figures: DESIGN.md section 29."""
import json

import numpy as np
import pytest

import denoise_binding as db
import emitters_binding as mb
import test_denoise_cpu as cpu
import test_emitters_gpu as eg

pytestmark = pytest.mark.gpu

SETTINGS = [(0, 0), (1, 0), (1, 1), (7, 2), (10, 3), (10, 0)]
SIZES = {"1x1": lambda tw, th: (1, 1), "3x2": lambda tw, th: (3, 2), "tile": lambda tw, th: (tw, th),
         "tile+1 x tile": lambda tw, th: (tw + 1, th), "tile x tile+1": lambda tw, th: (tw, th + 1),
         "2tile+1 x 2tile-1": lambda tw, th: (2 * tw + 1, 2 * th - 1), "47x35": lambda tw, th: (47, 35)}
W, H, DEPTH, PASSES = 80, 45, 5, 8


def random_case(w, h, passes, seed):
    """A seeded image in 0 .. 1 whose variances are exact zeros (sumsq is P |u|^2 as the kernel forms it, or below it), 1e30
    and values of 1e-4 .. 1e-2, a third of the pixels each"""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.0, 1.0, (h, w, 3))
    p = float(passes)
    base = p * ((mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2])
    kind = rng.integers(0, 3, (h, w))
    v = np.where(kind == 0, 0.0, np.where(kind == 1, 1e30, rng.uniform(1e-4, 1e-2, (h, w))))
    sumsq = base + 3.0 * ((p - 1.0) * p) * v
    below = (kind == 0) & (rng.uniform(0, 1, (h, w)) < 0.5)
    sumsq[below] = base[below] * 0.999                     # (a sum of squares below P |u|^2: the variance is cut to 0)
    return mean, sumsq


def run_gpu(rtc, mean, sumsq, naive, passes=0, tile_passes=None, tile=(0, 0), want_rgba=True, **setting):
    """-> (out [h][w][3] f64, rgba [h][w] u32 or None, rtc_rgba8_device(out) or None), host arrays"""
    import torch
    h, w = sumsq.shape
    stream = torch.cuda.Stream()
    d_mean, d_sumsq = torch.from_numpy(np.ascontiguousarray(mean)).cuda(), torch.from_numpy(np.ascontiguousarray(sumsq)).cuda()
    d_tp = torch.from_numpy(np.ascontiguousarray(tile_passes).astype(np.int32)).cuda() if tile_passes is not None else None
    d_out = torch.full((h, w, 3), -7.0, dtype=torch.float64, device="cuda")
    d_rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_rgba2 = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    rtc.set_option("denoise_naive", 1 if naive else 0)
    try:
        rtc.denoise_device(d_mean.data_ptr(), d_sumsq.data_ptr(), w, h, d_out.data_ptr(), stream.cuda_stream, passes=passes,
                           tile_passes_ptr=d_tp.data_ptr() if d_tp is not None else None, tile=tile,
                           setting=rtc.DenoiseSetting.make(**setting), rgba_ptr=d_rgba.data_ptr() if want_rgba else None)
    finally:
        rtc.set_option("denoise_naive", 0)
    if want_rgba:
        rtc.rgba8_device(d_out.data_ptr(), w * h, d_rgba2.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    out = d_out.cpu().numpy()
    return out, (d_rgba.cpu().numpy().view(np.uint32) if want_rgba else None), (d_rgba2.cpu().numpy().view(np.uint32) if want_rgba else None)


def both_forms(rtc, mean, sumsq, label, **kw):
    """Both forms against the checker and against each other; returns the tiled form's result."""
    want = db.denoise(mean, sumsq, **{k: v for k, v in kw.items() if k != "want_rgba"})
    got = {}
    for naive in (False, True):
        out, rgba, rgba2 = run_gpu(rtc, mean, sumsq, naive, **kw)
        err, ok = db.close(out, want)
        print(f"{label} {'naive' if naive else 'tiled'}: max |delta| / max(1, |value|) {err:.3e}")
        assert ok, (label, naive, err)
        if rgba is not None:
            assert np.array_equal(rgba, rgba2), (label, naive)
        got[naive] = out
    err, ok = db.close(got[False], got[True])
    print(f"{label} tiled against naive: {err:.3e} (0 is expected)")
    assert ok, (label, err)
    return got[False]


# ---- parity at sizes around the tile, windows and halos larger than the image among them
@pytest.mark.parametrize("size", list(SIZES))
def test_both_forms_against_the_checker(rtc, size):
    w, h = SIZES[size](*rtc.denoise_tile())
    mean, sumsq = random_case(w, h, PASSES, seed=w * 131 + h)
    for radius, patch in SETTINGS:
        out = both_forms(rtc, mean, sumsq, f"{w}x{h} ({radius}, {patch})", passes=PASSES, radius=radius, patch=patch)
        if radius == 0:
            assert np.array_equal(out, mean)


def test_other_strengths_and_pass_counts(rtc):
    mean, sumsq = random_case(37, 21, 2, seed=5)
    both_forms(rtc, mean, sumsq, "37x21 at 2 passes, strength 0.7, cancel 0", passes=2, radius=5, patch=1, strength=0.7, cancel=0.0)
    both_forms(rtc, mean, sumsq, "37x21 at 2 passes, strength 0.2, cancel 2", passes=2, radius=3, patch=3, strength=0.2, cancel=2.0, want_rgba=False)


def test_non_finite_inputs_propagate(rtc):
    mean, sumsq = random_case(47, 35, PASSES, seed=9)
    mean[3, 4, 1] = np.nan
    mean[20, 30, 0] = np.inf
    sumsq[10, 10] = np.inf
    sumsq[30, 40] = np.nan
    out = both_forms(rtc, mean, sumsq, "47x35 with NaN and inf", passes=PASSES)
    assert not np.isfinite(out).all() and np.isfinite(out).any()


# ---- an adaptive run's tile_passes
def test_tile_passes_and_a_tile_at_one_pass(rtc):
    mean, sumsq, tile_passes, tile, where = cpu.tiles_case()
    out = both_forms(rtc, mean, sumsq, "17x11 in 5x3 tiles", tile_passes=tile_passes, tile=tile)
    assert np.array_equal(out[where], mean[where])
    assert not np.array_equal(out, mean)                                       # (the other tiles are smoothed)


# ---- Progressive and AdaptiveProgressive on the fixture
@pytest.fixture(scope="module")
def fixture_reference(rtc):
    """emitters_mix.json at 80 x 45: the mean of GPU passes 32 .. 159, computed once and left unchanged"""
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = eg.handle(rtc, hs, hs.sampling())
    total = np.zeros((H, W, 3))
    for p in range(32, 160):
        gpu.set_sample_pass(p)
        total += gpu.render(cam, DEPTH)
    gpu.close()
    ref = total / 128.0
    ref.setflags(write=False)
    return hs, cam, ref


def test_progressive_denoised_is_the_checkers_and_gains(rtc, fixture_reference):
    import torch
    hs, cam, ref = fixture_reference
    prog = rtc.Progressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH)
    for _ in range(PASSES):
        prog.step()
    got = prog.denoised().cpu().numpy()
    mean, sumsq = prog.mean().cpu().numpy(), prog.sumsq.cpu().numpy()
    torch.cuda.synchronize()
    err, ok = db.close(got, db.denoise(mean, sumsq, PASSES))
    print(f"Progressive.denoised() against the checker: {err:.3e}")
    assert ok, err
    noisy, den = db.rmse(mean, ref), db.rmse(got, ref)
    print(f"RMSE noisy {noisy:.5f}, denoised {den:.5f}, ratio {noisy / den:.3f} (>= 1.2)")
    assert noisy / den >= 1.2
    small = prog.denoised(radius=2, patch=1, strength=0.3).cpu().numpy()
    assert db.close(small, db.denoise(mean, sumsq, PASSES, radius=2, patch=1, strength=0.3))[1]
    with pytest.raises(ValueError):
        rtc.Progressive(prog.gpu, cam, DEPTH, noise=False).denoised()


def test_adaptive_denoised_is_the_checkers_and_gains(rtc, fixture_reference):
    import torch
    hs, cam, ref = fixture_reference
    adaptive = rtc.Adaptive.make(0.03, PASSES, min_passes=2, tile=16)
    run = rtc.AdaptiveProgressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH, adaptive=adaptive)
    run.run()
    got = run.denoised().cpu().numpy()
    mean, sumsq, tile_passes = run.mean().cpu().numpy(), run.sumsq.cpu().numpy(), run.tile_passes().cpu().numpy().astype(np.uint32)
    torch.cuda.synchronize()
    print("tile passes", tile_passes.tolist())
    assert tile_passes.min() >= 2 and tile_passes.max() <= PASSES
    err, ok = db.close(got, db.denoise(mean, sumsq, tile_passes=tile_passes, tile=(16, 16)))
    print(f"AdaptiveProgressive.denoised() against the checker: {err:.3e}")
    assert ok, err
    noisy, den = db.rmse(mean, ref), db.rmse(got, ref)
    print(f"RMSE noisy {noisy:.5f}, denoised {den:.5f}, ratio {noisy / den:.3f} (>= 1.2)")
    assert noisy / den >= 1.2


# ---- the convenience calls
def test_render_denoised_is_progressive_denoised_and_restores_the_pass(rtc, fixture_reference):
    import torch
    hs, cam, _ = fixture_reference
    gpu = eg.handle(rtc, hs, hs.sampling(), sample_pass=3)
    before = gpu.render(cam, DEPTH)
    rgb, noisy = gpu.render_denoised(cam, PASSES, max_depth=DEPTH)
    assert np.array_equal(gpu.render(cam, DEPTH), before)                      # (the handle is still at pass 3 ...)
    gpu.set_sample_pass(0)
    assert not np.array_equal(gpu.render(cam, DEPTH), before)                  # (... which is not pass 0's image)
    prog = rtc.Progressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH)
    for _ in range(PASSES):
        prog.step()
    want, mean = prog.denoised().cpu().numpy(), prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(rgb, want) and np.array_equal(noisy, mean)
    # another setting, and an adaptive run
    setting = rtc.DenoiseSetting.make(radius=3, patch=1, strength=0.6, cancel=0.5)
    rgb2, _ = gpu.render_denoised(cam, PASSES, setting=setting, max_depth=DEPTH)
    assert np.array_equal(rgb2, prog.denoised(radius=3, patch=1, strength=0.6, cancel=0.5).cpu().numpy())
    adaptive = rtc.Adaptive.make(0.03, PASSES, min_passes=2, tile=16)
    rgb3, noisy3 = gpu.render_denoised(cam, 0, adaptive=adaptive, max_depth=DEPTH)
    run = rtc.AdaptiveProgressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH, adaptive=adaptive)
    run.run()
    assert np.array_equal(noisy3, run.mean().cpu().numpy()) and np.array_equal(rgb3, run.denoised().cpu().numpy())


def test_host_render_of_a_file_with_the_key(rtc):
    scene = json.loads(open(mb.EMITTERS_MIX).read())
    scene["camera"]["sampling"].update(passes=PASSES, denoise={"radius": 5, "strength": 0.5})
    hs = rtc.HostScene(json.dumps(scene))
    setting = hs.denoise()
    assert setting.to_dict() == {"radius": 5, "patch": 2, "strength": 0.5, "cancel": 1.0}
    out = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    rgb, noisy = eg.handle(rtc, hs, hs.sampling()).render_denoised(hs.camera(), hs.passes(), setting=setting, max_depth=DEPTH)
    assert np.array_equal(out, rgb) and not np.array_equal(out, noisy)
    # with "adaptive" beside it: the file's adaptive setting goes along
    scene["camera"]["sampling"].update(adaptive={"threshold": 0.03, "min-passes": 2}, denoise=True)
    hs = rtc.HostScene(json.dumps(scene))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    rgb, _ = eg.handle(rtc, hs, hs.sampling()).render_denoised(hs.camera(), 0, adaptive=hs.adaptive(), setting=hs.denoise(), max_depth=DEPTH)
    assert np.array_equal(out, rgb)


# ---- the two forms at a size no checker run is made at: one launch each
def test_the_two_forms_agree_on_a_rendered_mean_at_480x270(rtc):
    import torch
    hs = mb.mix(rtc)
    cam = hs.camera(480, 270)
    prog = rtc.Progressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH)
    for _ in range(4):
        prog.step()
    tiled = prog.denoised().cpu().numpy()
    rtc.set_option("denoise_naive", 1)
    try:
        naive = prog.denoised().cpu().numpy()
    finally:
        rtc.set_option("denoise_naive", 0)
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    err, ok = db.close(tiled, naive)
    print(f"480x270, 4 passes: tiled against naive {err:.3e} (0 is expected)")
    assert ok, err
    assert np.isfinite(tiled).all() and not np.array_equal(tiled, mean)
