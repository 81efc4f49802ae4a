"""Robust accumulation on the GPU (rtc_robust_device, the kernels of csrc/rtc_robust.hip): the register
forms - wide and, with pointers offset by one double or an odd pixel count, narrow - and, under option "robust_naive", the
literal form, against the checker (tests/cpp/robust_oracle.cpp) and against each other.  No library function is involved:
mean_out, sumsq_out and rejected_out are held to the checker's bits, rgba to rtc_rgba8_device(mean_out).

Then the chain on the fixture tests/golden/robust_scenes/robust_lamp.json: Progressive(robust=5), its buckets, robust(),
denoised(robust={}), filmed(denoise={}, robust={}), rtc_render_robust, rtch_scene_render, and the fixture's two measures on the
GPU's own passes.

Figures: DESIGN.md section 31."""
import numpy as np
import pytest

import denoise_binding as db
import film_binding as fb
import robust_binding as rb
import test_emitters_gpu as eg
from test_robust_cpu import LAMP_BOUND

pytestmark = pytest.mark.gpu

BUCKETS = (3, 5, 7, 9, 11, 13, 15)
SIZES = (1, 2, 3, 255, 256, 257, 513)
GAINS = (0.0, 0.5, 1.0, 4.0, 1e9)
KINDS = 8
W, H, DEPTH, PASSES = 80, 45, 5, 16


def passes_of(m):
    return (m, m + 1, 2 * m - 1, 2 * m, 3 * m + 2)


def seeded_sums(m, n, passes, seed, shift=0):
    """[M][n][3] bucket sums; pixel i is of kind (i + shift) % 8: ordinary, exact duplicates across buckets (the tie-break
    decides), all zeros, negatives, a 1e30 spike, one NaN, one +inf, NaN in the majority"""
    rng = np.random.default_rng(seed)
    frames = np.array([passes // m + (1 if j < passes % m else 0) for j in range(m)], dtype=np.float64)
    means = rng.uniform(0.0, 2.0, (m, n, 3))
    kind = (np.arange(n) + shift) % KINDS
    eighths = rng.integers(0, 4, (m, n, 1)) / 8.0                     # (few values, exact in every product and quotient: ties)
    means = np.where((kind == 1)[None, :, None], np.broadcast_to(eighths, means.shape), means)
    means[:, kind == 2] = 0.0
    means = np.where((kind == 3)[None, :, None], means - 1.0, means)
    sums = means * frames[:, None, None]
    pick = rng.integers(0, m, n)
    at = np.arange(n)
    sums[pick[kind == 4], at[kind == 4], rng.integers(0, 3)] = 1e30
    sums[pick[kind == 5], at[kind == 5], rng.integers(0, 3)] = np.nan
    sums[pick[kind == 6], at[kind == 6]] = np.inf
    start, channel = rng.integers(0, m, n), rng.integers(0, 3)
    for t in range(m // 2 + 1):
        sums[((start + t) % m)[kind == 7], at[kind == 7], channel] = np.nan
    return sums


class OnDevice:
    """Bucket sums on the device, 16-byte aligned and offset by one double, and outputs for both"""

    def __init__(self, sums):
        import torch
        self.m, self.n = sums.shape[0], sums.shape[1]
        self.stream = torch.cuda.Stream()
        flat = torch.zeros(sums.size + 1, dtype=torch.float64, device="cuda")
        host = torch.from_numpy(np.ascontiguousarray(sums).reshape(-1))
        flat[:-1].copy_(host)
        self.sums = {False: flat[:-1], True: torch.zeros_like(flat)[1:]}
        self.sums[True].copy_(host)
        self.mean = torch.zeros(self.n * 3 + 1, dtype=torch.float64, device="cuda")
        self.sumsq = torch.zeros(self.n + 1, dtype=torch.float64, device="cuda")
        self.rejected = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.rgba = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.rgba2 = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.stream.wait_stream(torch.cuda.current_stream())

    def run(self, rtc, passes, gain, naive=False, unaligned=False):
        """-> (mean [n][3], sumsq [n], rejected [n] u32, rgba [n] u32, rtc_rgba8_device(mean) [n] u32), host values"""
        mean = self.mean[1:] if unaligned else self.mean[:-1]
        sumsq = self.sumsq[1:] if unaligned else self.sumsq[:-1]
        sums = self.sums[unaligned]
        assert (sums.data_ptr() % 16 == 8) == unaligned and (mean.data_ptr() % 16 == 8) == unaligned
        self.mean.fill_(-7.0), self.sumsq.fill_(-7.0), self.rejected.fill_(-7), self.rgba.fill_(0)
        self.stream.wait_stream(__import__("torch").cuda.current_stream())
        rtc.set_option("robust_naive", 1 if naive else 0)
        try:
            rtc.robust_device(sums.data_ptr(), self.n, passes, mean.data_ptr(), self.stream.cuda_stream,
                              setting=rtc.RobustSetting.make(self.m, gain), sumsq_ptr=sumsq.data_ptr(), rejected_ptr=self.rejected.data_ptr(),
                              rgba_ptr=self.rgba.data_ptr())
        finally:
            rtc.set_option("robust_naive", 0)
        rtc.rgba8_device(mean.data_ptr(), self.n, self.rgba2.data_ptr(), self.stream.cuda_stream)
        self.stream.synchronize()
        return (mean.cpu().numpy().reshape(self.n, 3), sumsq.cpu().numpy(), self.rejected.cpu().numpy().view(np.uint32),
                self.rgba.cpu().numpy().view(np.uint32), self.rgba2.cpu().numpy().view(np.uint32))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


FORMS = [("register", False, False), ("register, offset pointers", False, True), ("literal", True, False)]


def hold(rtc, sums, passes, gains, label, forms=FORMS):
    dev = OnDevice(sums)
    for gain in gains:
        want = rb.robust(sums, passes, gain)
        for name, naive, unaligned in forms:
            mean, sumsq, rejected, rgba, rgba2 = dev.run(rtc, passes, gain, naive, unaligned)
            where = (label, gain, name)
            assert same_bits(mean, want["mean"]), where
            assert same_bits(sumsq, want["sumsq"]), where
            assert np.array_equal(rejected, want["rejected"]), where
            assert np.array_equal(rgba, rgba2) and np.array_equal(rgba, rb.rgba(want["mean"])), where


# ---- seeded bucket sums: both kernel forms and the checker, bit for bit
@pytest.mark.parametrize("m", BUCKETS)
def test_every_form_gives_the_checkers_bits(rtc, m):
    for passes in passes_of(m):
        for n in SIZES:
            # (fewer pixels than kinds of values: a run per kind)
            for shift in (range(KINDS) if n < KINDS else (0,)):
                sums = seeded_sums(m, n, passes, seed=1000 * m + 10 * passes + n, shift=shift)
                hold(rtc, sums, passes, GAINS, f"M {m} P {passes} n {n} shift {shift}")


def test_the_values_are_what_they_are_meant_to_be():
    """the seeded sums hold every kind the kernels are held on (no GPU needed, but it describes this file's inputs)"""
    sums = seeded_sums(5, 256, 12, seed=3)
    r = rb.robust(sums, 12)
    kind = np.arange(256) % KINDS
    assert (r["rejected"][kind == 2] == 0).all() and (r["mean"][kind == 2] == 0.0).all()
    assert np.isfinite(r["mean"][(kind == 4) | (kind == 5) | (kind == 6)]).all() and (r["rejected"][kind == 6] == 4).all()
    assert r["mean"][kind == 4].max() < 1e29 and not np.isfinite(r["mean"][kind == 7]).all(axis=1).any()
    assert r["mean"][kind == 3].min() < 0.0
    means = sums[:, kind == 1] / np.array([3, 3, 2, 2, 2.0])[:, None, None]
    assert (means[0] == means[1]).all(axis=1).any()                                            # (whole buckets tie)
    assert len({int(x) for x in r["rejected"]}) >= 2


def test_above_the_grids_cap_a_lane_takes_more_than_one_item(rtc):
    max_blocks, block = rtc.robust_grid()
    n = 2 * max_blocks * block + 2          # (wide: one pair more than one sweep holds; narrow and literal: two sweeps and more)
    sums = seeded_sums(3, n, 4, seed=11)
    hold(rtc, sums, 4, (1.0,), f"n {n}")


def test_an_odd_pixel_count_takes_the_narrow_form(rtc):
    """n * 24 bytes is a bucket's stride: with n odd the second bucket is not 16-byte aligned, whatever the pointers are"""
    sums = seeded_sums(7, 1001, 17, seed=5)
    hold(rtc, sums, 17, (1.0, 0.5), "n 1001", forms=FORMS[:1] + FORMS[2:])


def test_optional_outputs_may_be_absent(rtc):
    import torch
    sums = seeded_sums(5, 300, 16, seed=9)
    want = rb.robust(sums, 16)
    d_sums = torch.from_numpy(sums).cuda()
    d_mean = torch.zeros((300, 3), dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for naive in (0, 1):
        d_mean.fill_(-7.0)
        stream.wait_stream(torch.cuda.current_stream())
        rtc.set_option("robust_naive", naive)
        try:
            rtc.robust_device(d_sums.data_ptr(), 300, 16, d_mean.data_ptr(), stream.cuda_stream)      # (the default setting)
        finally:
            rtc.set_option("robust_naive", 0)
        stream.synchronize()
        assert same_bits(d_mean.cpu().numpy(), want["mean"])


# ---- the chain on the fixture
def _host(*tensors):
    import torch
    out = [t.cpu().numpy() for t in tensors]
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def lamp_run(rtc):
    """robust_lamp.json at 80 x 45, 16 passes: the Progressive objects with and without buckets, every frame, and what they
    leave, computed once and left unchanged"""
    hs = rtc.HostScene.from_file(rb.ROBUST_LAMP)
    cam = hs.camera()
    assert (cam.hsize, cam.vsize, hs.passes()) == (W, H, PASSES) and hs.robust().to_dict() == rb.DEFAULTS
    prog = rtc.Progressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH, robust=5)
    bare = rtc.Progressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH)
    frames = []
    for _ in range(PASSES):
        prog.step()
        bare.step()
        prog.stream.synchronize()
        frames.append(_host(prog.frame)[0].copy())
    mean, sumsq, buckets = _host(prog.mean(), prog.sumsq, prog.buckets)
    for a in frames + [mean, sumsq, buckets]:
        a.setflags(write=False)
    return hs, cam, prog, bare, frames, mean, sumsq, buckets


def test_the_buckets_are_the_in_order_sums_of_their_frames(rtc, lamp_run):
    hs, cam, prog, bare, frames, mean, sumsq, buckets = lamp_run
    assert buckets.shape == (5, H, W, 3) and same_bits(buckets, rb.bucket_sums(frames, 5))
    total = frames[0]
    for f in frames[1:]:
        total = total + f
    assert same_bits(mean, total / float(PASSES))


def test_a_progressive_without_buckets_gives_the_bits_of_before(rtc, lamp_run):
    hs, cam, prog, bare, frames, mean, sumsq, buckets = lamp_run
    assert bare.buckets is None and prog.passes == bare.passes == PASSES
    bare_mean, bare_sumsq, bare_rgba, rgba = _host(bare.mean(), bare.sumsq, bare.rgba8(), prog.rgba8())
    assert same_bits(bare_mean, mean) and same_bits(bare_sumsq, sumsq) and np.array_equal(bare_rgba, rgba)
    assert same_bits(_host(bare.denoised())[0], _host(prog.denoised())[0])
    with pytest.raises(ValueError):
        bare.robust()


def test_progressive_robust_is_the_checkers(rtc, lamp_run):
    hs, cam, prog, bare, frames, mean, sumsq, buckets = lamp_run
    for gain in (1.0, 0.0, 3.0):
        got_mean, got_sumsq, got_rejected = _host(*prog.robust(gain=gain))
        want = rb.robust(buckets, PASSES, gain)
        assert same_bits(got_mean, want["mean"]) and same_bits(got_sumsq, want["sumsq"])
        assert np.array_equal(got_rejected.view(np.uint32), want["rejected"])
    assert (rb.robust(buckets, PASSES)["rejected"] > 0).any()
    # the later stages over the robust pair, within the tolerances those stages have
    want = rb.robust(buckets, PASSES)
    denoised = _host(prog.denoised(robust={}))[0]
    err, ok = db.close(denoised, db.denoise(want["mean"], want["sumsq"], passes=PASSES))
    print(f"Progressive.denoised(robust={{}}) against the denoiser's checker on the robust pair: {err:.3e}")
    assert ok, err
    assert not same_bits(denoised, _host(prog.denoised())[0])
    small = dict(radius=2, patch=1, strength=0.3)
    err, ok = db.close(_host(prog.denoised(robust=dict(gain=0.5), **small))[0],
                       db.denoise(*[rb.robust(buckets, PASSES, 0.5)[k] for k in ("mean", "sumsq")], passes=PASSES, **small))
    assert ok, err
    film = dict(exposure=0.8, bloom_radius=6, bloom_sigma=2.0, bloom_threshold=1.0, bloom_intensity=0.2)
    out, rgba = _host(*prog.filmed(denoise={}, robust={}, **film))
    err, ok = fb.close(out, fb.film(denoised, **rtc.FilmSetting.make(**film).to_dict())[0])
    print(f"Progressive.filmed(denoise={{}}, robust={{}}) against the film checker on the denoised robust mean: {err:.3e}")
    assert ok, err
    assert np.array_equal(rgba, np.ascontiguousarray(fb.rgba(out)).view(np.uint8).reshape(H, W, 4))
    out2 = _host(prog.filmed(robust={}, **film)[0])[0]
    assert fb.close(out2, fb.film(want["mean"], **rtc.FilmSetting.make(**film).to_dict())[0])[1]


def test_render_robust_is_the_chain_and_restores_the_pass(rtc, lamp_run):
    hs, cam, prog, bare, frames, mean, sumsq, buckets = lamp_run
    gpu = eg.handle(rtc, hs, hs.sampling(), sample_pass=3)
    before = gpu.render(cam, DEPTH)
    rgb, rgba, robust_mean, plain, rejected = gpu.render_robust(cam, PASSES, max_depth=DEPTH)
    assert np.array_equal(gpu.render(cam, DEPTH), before)                      # (the handle is still at pass 3 ...)
    gpu.set_sample_pass(0)
    assert not np.array_equal(gpu.render(cam, DEPTH), before)                  # (... which is not pass 0's image)
    gpu.set_sample_pass(3)
    want_mean, _, want_rejected = _host(*prog.robust())
    assert same_bits(robust_mean, want_mean) and same_bits(rgb, want_mean) and np.array_equal(rejected, want_rejected.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(rgba).view(np.uint32)[..., 0], rb.rgba(want_mean))
    assert same_bits(plain, mean)
    assert same_bits(plain, gpu.render_denoised(cam, PASSES, max_depth=DEPTH)[1])     # (rtc_render_denoised's noisy_out)
    # another setting; then the denoiser and the film stage behind it
    rgb7 = gpu.render_robust(cam, PASSES, robust=rtc.RobustSetting.make(5, 0.0), max_depth=DEPTH)[0]
    assert same_bits(rgb7, _host(prog.robust(gain=0.0)[0])[0])
    dn = rtc.DenoiseSetting.make()
    rgb2, rgba2, robust2, plain2, _ = gpu.render_robust(cam, PASSES, denoise=dn, max_depth=DEPTH)
    assert same_bits(rgb2, _host(prog.denoised(robust={}))[0]) and same_bits(robust2, want_mean) and same_bits(plain2, mean)
    assert np.array_equal(np.ascontiguousarray(rgba2).view(np.uint32)[..., 0], rb.rgba(rgb2))
    film = dict(exposure=0.8, bloom_radius=6, bloom_sigma=2.0, bloom_threshold=1.0, bloom_intensity=0.2)
    rgb3, rgba3, robust3, _, _ = gpu.render_robust(cam, PASSES, denoise=dn, film=rtc.FilmSetting.make(**film), max_depth=DEPTH)
    want3, want_rgba3 = _host(*prog.filmed(denoise={}, robust={}, **film))
    assert same_bits(rgb3, want3) and np.array_equal(rgba3, want_rgba3) and same_bits(robust3, want_mean)
    rgb4 = gpu.render_robust(cam, PASSES, film=rtc.FilmSetting.make(**film), max_depth=DEPTH)[0]
    assert same_bits(rgb4, _host(prog.filmed(robust={}, **film)[0])[0])
    with pytest.raises(rtc.RtcError):
        gpu.render_robust(cam, 4, max_depth=DEPTH)


def test_host_render_of_the_fixture(rtc, lamp_run):
    """rtch_scene_render of a file with the key goes through rtc_render_robust"""
    hs, cam, prog, bare, frames, mean, sumsq, buckets = lamp_run
    out = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    rgb = eg.handle(rtc, hs, hs.sampling()).render_robust(cam, hs.passes(), robust=hs.robust(), denoise=hs.denoise(), film=hs.film(),
                                                          max_depth=DEPTH)[0]
    assert same_bits(out, rgb) and not same_bits(out, mean)


def test_the_fixtures_measures_hold_on_the_gpus_own_passes(rtc, lamp_run):
    hs, cam, prog, bare, frames, mean, sumsq, buckets = lamp_run
    gpu = eg.handle(rtc, hs, hs.sampling())
    total = np.zeros((H, W, 3))
    for p in range(32, 160):
        gpu.set_sample_pass(p)
        total = total + gpu.render(cam, DEPTH)
    reference = total / 128.0
    robust_mean = _host(prog.robust()[0])[0]
    a_plain, a_robust = rb.speck_share(mean), rb.speck_share(robust_mean)
    e_plain, e_robust = rb.rmse(mean, reference), rb.rmse(robust_mean, reference)
    print(f"speck share: plain {a_plain:.4f}, robust {a_robust:.4f}; RMSE against passes 32 .. 159: plain {e_plain:.4f}, "
          f"robust {e_robust:.4f}, ratio {e_plain / e_robust:.3f} (bound {LAMP_BOUND:.3f})")
    assert a_plain > 0.0 and a_robust < a_plain
    assert e_plain / e_robust >= LAMP_BOUND > 1.0
