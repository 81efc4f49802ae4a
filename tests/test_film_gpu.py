"""The film stage on the GPU (rtc_film_device, the kernels of csrc/rtc_film.hip): the point kernel in its
wide and its narrow form, the tiled bloom kernels and, under option "film_naive", the literal ones, against the checker
(tests/cpp/film_oracle.cpp) and against each other, at sizes around the tiles and with windows and halos larger than the
image, with every curve and every transfer.

With manual exposure and a LINEAR transfer no library function is involved: every form equals the checker to the bit.
Otherwise (pow, or the automatic exposure's exp and log) both forms are within 1e-12 * max(1, |value|) of the checker run with
the GPU's E, and equal to each other exactly; the GPU's E is within 1e-12, relatively, of the checker's own, whose sum T is
taken in long double.  Inputs for the automatic exposure have luminances of 1e-3 .. 1e2: every term of T is below 7 in
magnitude, a lane adds a few of them, the block and the final sum are trees of some 20 additions per path, so T / n carries
an error of a few 1e-15 at most and E of 2e-14, relatively.

Then Progressive.filmed(), AdaptiveProgressive.filmed(), rtc_render_filmed and rtch_scene_render of the fixture
tests/golden/film_scenes/film_lamp.json.

Figures: DESIGN.md section 30."""
import numpy as np
import pytest

import emitters_binding as mb
import film_binding as fb
import test_emitters_gpu as eg

pytestmark = pytest.mark.gpu

SIZES = {"1x1": lambda rw, cw, ch: (1, 1), "3x2": lambda rw, cw, ch: (3, 2), "row_w x 3": lambda rw, cw, ch: (rw, 3),
         "row_w+1 x 3": lambda rw, cw, ch: (rw + 1, 3), "7 x col_h": lambda rw, cw, ch: (7, ch), "7 x col_h+1": lambda rw, cw, ch: (7, ch + 1),
         "2col_w+1 x 2col_h-1": lambda rw, cw, ch: (2 * cw + 1, 2 * ch - 1), "65x5": lambda rw, cw, ch: (65, 5),
         "5x4": lambda rw, cw, ch: (5, 4), "70x67": lambda rw, cw, ch: (70, 67)}
# (radius, sigma, curve, transfer, exposure, auto_key): every radius of the issue, every curve and every transfer; the settings
# with manual exposure and a LINEAR transfer are held to the checker's bits
BLOOMS = [(1, 0.6, fb.LINEAR, fb.T_LINEAR, 1.0, 0.0), (2, 1.0, fb.REINHARD, fb.T_LINEAR, 0.7, 0.0), (12, 4.0, fb.HABLE, fb.T_LINEAR, 1.3, 0.0),
          (32, 9.0, fb.ACES, fb.T_LINEAR, 0.9, 0.0), (12, 4.0, fb.ACES, fb.T_SRGB, 1.0, 0.18), (32, 10.0, fb.HABLE, fb.T_GAMMA, 1.3, 0.0),
          (2, 0.7, fb.LINEAR, fb.T_SRGB, 2.0, 0.36)]
W, H, DEPTH, PASSES = 80, 45, 5, 8


def luminance(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def random_image(w, h, seed):
    """A seeded image in 0 .. 16 with a twentieth of its pixels at 1e3 (one at least)"""
    rng = np.random.default_rng(seed)
    image = rng.uniform(0.0, 16.0, (h, w, 3))
    hot = rng.uniform(0, 1, (h, w)) < 0.05
    hot[rng.integers(0, h), rng.integers(0, w)] = True
    image[hot] = 1e3
    return image


def auto_image(w, h, seed):
    """A seeded image whose luminances are 1e-3 .. 1e2, spread evenly in the logarithm"""
    rng = np.random.default_rng(seed)
    colour = rng.uniform(0.5, 1.5, (h, w, 3))
    lum = 10.0 ** rng.uniform(-3.0, 2.0, (h, w))
    return colour * (lum / luminance(colour))[..., None]


def run_gpu(rtc, image, naive=False, unaligned=False, **setting):
    """-> (out [h][w][3] f64, rgba [h][w] u32, rtc_rgba8_device(out), E from scale_out), host values"""
    import torch
    h, w, _ = image.shape
    s = rtc.FilmSetting(*[dict(fb.DEFAULTS, **setting)[name] for name, _ in rtc.FilmSetting._fields_])
    stream = torch.cuda.Stream()
    flat = torch.zeros(h * w * 3 + 1, dtype=torch.float64, device="cuda")      # (offset by one double: not 16-byte aligned)
    d_in = flat[1:] if unaligned else flat[:-1]
    d_in.copy_(torch.from_numpy(np.ascontiguousarray(image).reshape(-1)))
    assert (d_in.data_ptr() % 16 == 8) == unaligned
    d_out = torch.full((h, w, 3), -7.0, dtype=torch.float64, device="cuda")
    d_rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_rgba2 = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_scale = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    n = rtc.film_scratch_bytes(w, h, s)
    d_scratch = torch.zeros((n + 7) // 8, dtype=torch.float64, device="cuda") if n else None
    stream.wait_stream(torch.cuda.current_stream())
    rtc.set_option("film_naive", 1 if naive else 0)
    try:
        rtc.film_device(d_in.data_ptr(), w, h, d_out.data_ptr(), stream.cuda_stream, setting=s,
                        scratch_ptr=d_scratch.data_ptr() if d_scratch is not None else None, rgba_ptr=d_rgba.data_ptr(),
                        scale_ptr=d_scale.data_ptr())
    finally:
        rtc.set_option("film_naive", 0)
    rtc.rgba8_device(d_out.data_ptr(), w * h, d_rgba2.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return d_out.cpu().numpy(), d_rgba.cpu().numpy().view(np.uint32), d_rgba2.cpu().numpy().view(np.uint32), float(d_scale.item())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def hold(rtc, image, label, forms, **setting):
    """Every form of `forms` (pairs of run_gpu's naive, unaligned) against the checker and against each other; returns the
    first form's result and E."""
    s = dict(fb.DEFAULTS, **setting)
    exact = s["auto_key"] == 0.0 and s["transfer"] == fb.T_LINEAR
    own, own_E = fb.film(image, **setting)
    got = []
    for naive, unaligned in forms:
        out, rgba, rgba2, E = run_gpu(rtc, image, naive, unaligned, **setting)
        name = ("naive" if naive else "tiled") + (", unaligned" if unaligned else "")
        if s["auto_key"] == 0.0:
            assert E == s["exposure"], (label, name)
            want = own
        else:
            rel = abs(E - own_E) / own_E
            print(f"{label} {name}: E {E!r}, the checker's {own_E!r}, relative difference {rel:.3e}")
            assert rel <= 1e-12, (label, name, E, own_E)
            want, used = fb.film(image, E=E, **setting)
            assert used == E
        err, ok = fb.close(out, want)
        print(f"{label} {name}: max |delta| / max(1, |value|) {err:.3e}" + (" (0 is required)" if exact else ""))
        assert ok, (label, name, err)
        if exact:
            assert np.array_equal(out, want), (label, name)
        assert np.array_equal(rgba, rgba2), (label, name)
        got.append((out, E))
    for out, E in got[1:]:
        assert same_bits(out, got[0][0]) and E == got[0][1], label           # (the forms agree exactly; so do two runs' E)
    return got[0]


BOTH = [(False, False), (True, False)]          # the tiled and the literal bloom kernels
WIDE_NARROW = [(False, False), (False, True)]   # the point kernel's two forms


# ---- parity at sizes around the tiles, windows and halos larger than the image among them
@pytest.mark.parametrize("size", list(SIZES))
def test_bloom_in_both_forms_against_the_checker(rtc, size):
    w, h = SIZES[size](*rtc.film_tile())
    for radius, sigma, curve, transfer, exposure, key in BLOOMS:
        image = (auto_image if key else random_image)(w, h, seed=w * 131 + h + radius)
        hold(rtc, image, f"{w}x{h} R={radius} curve {curve} transfer {transfer}", BOTH, exposure=exposure, auto_key=key, bloom_radius=radius,
             bloom_sigma=sigma, bloom_threshold=1.0, bloom_intensity=0.15, curve=curve, transfer=transfer, white=4.0 + radius, gamma=2.2)


@pytest.mark.parametrize("size", list(SIZES))
def test_the_point_kernel_in_both_forms_against_the_checker(rtc, size):
    w, h = SIZES[size](*rtc.film_tile())
    image = random_image(w, h, seed=w * 17 + h)
    for curve in (fb.LINEAR, fb.REINHARD, fb.ACES, fb.HABLE):
        for transfer in (fb.T_LINEAR, fb.T_SRGB, fb.T_GAMMA):
            hold(rtc, image, f"{w}x{h} curve {curve} transfer {transfer}", WIDE_NARROW, exposure=0.8, curve=curve, transfer=transfer, white=6.0,
                 gamma=2.4)
    hold(rtc, auto_image(w, h, seed=w + h), f"{w}x{h} automatic", WIDE_NARROW, auto_key=0.18, exposure=1.5)


def test_other_thresholds_and_intensities(rtc):
    image = random_image(37, 21, seed=5)
    for threshold, intensity in ((0.0, 1.0), (8.0, 0.5), (2000.0, 0.3)):      # (everything blooms; the hot pixels and a few; nothing)
        out, _ = hold(rtc, image, f"37x21 threshold {threshold} intensity {intensity}", BOTH, bloom_radius=5, bloom_sigma=1.7, bloom_threshold=threshold,
                      bloom_intensity=intensity, curve=fb.REINHARD, transfer=fb.T_LINEAR)
    assert same_bits(out, fb.film(image, curve=fb.REINHARD, transfer=fb.T_LINEAR)[0])   # (above every luminance: B is +0.0 everywhere)
    # intensity 0, or radius 0, is no bloom: the point kernel, to the bit
    plain, _ = hold(rtc, image, "37x21 no bloom", WIDE_NARROW, curve=fb.ACES, transfer=fb.T_LINEAR)
    for off in (dict(bloom_radius=5, bloom_sigma=1.7, bloom_threshold=0.0, bloom_intensity=0.0), dict(bloom_radius=0, bloom_intensity=0.5)):
        out, _ = hold(rtc, image, f"37x21 {off}", BOTH, curve=fb.ACES, transfer=fb.T_LINEAR, **off)
        assert same_bits(out, plain)


def test_the_identity_setting_returns_the_inputs_bits(rtc):
    image = random_image(70, 67, seed=2)
    image[5, 6] = (-0.0, 1e-300, 1e300)
    for unaligned in (False, True):
        out, _, _, E = run_gpu(rtc, image, unaligned=unaligned, **fb.IDENTITY)
        assert E == 1.0 and same_bits(out, image)


def test_an_unaligned_image_takes_the_narrow_form_and_gives_the_same_bits(rtc):
    image = random_image(131, 9, seed=4)
    for setting in (dict(curve=fb.ACES, transfer=fb.T_SRGB), dict(curve=fb.HABLE, transfer=fb.T_GAMMA, auto_key=0.18),
                    dict(curve=fb.ACES, transfer=fb.T_SRGB, bloom_radius=12, bloom_intensity=0.15)):
        a = run_gpu(rtc, image, unaligned=False, **setting)
        b = run_gpu(rtc, image, unaligned=True, **setting)
        assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3], setting


def test_above_the_reductions_cap_a_lane_sums_more_than_one_pixel(rtc):
    """1024 x 513 is 525 312 pixels: one more row than 2048 blocks of 256 lanes hold, so the first 1024 lanes of the
    reduction take two pixels each and the point kernel's narrow form strides as well"""
    image = auto_image(1024, 513, seed=7)
    assert image.shape[0] * image.shape[1] > 2048 * 256
    out, E = hold(rtc, image, "1024x513 automatic", WIDE_NARROW, auto_key=0.18, curve=fb.ACES, transfer=fb.T_SRGB)
    assert np.isfinite(out).all() and 0.0 < E < 10.0


def test_non_finite_inputs_propagate_in_kind(rtc):
    image = random_image(47, 35, seed=9)
    image[3, 4, 1] = np.nan
    image[20, 30, 0] = np.inf
    image[30, 10, 2] = -np.inf
    cases = [(WIDE_NARROW, dict(curve=fb.LINEAR, transfer=fb.T_LINEAR)), (WIDE_NARROW, dict(curve=fb.REINHARD, transfer=fb.T_SRGB)),
             (BOTH, dict(curve=fb.LINEAR, transfer=fb.T_LINEAR, bloom_radius=3, bloom_sigma=1.0, bloom_intensity=0.2)),
             (BOTH, dict(curve=fb.ACES, transfer=fb.T_SRGB, bloom_radius=12, bloom_sigma=4.0, bloom_intensity=0.15))]
    for forms, setting in cases:
        want, _ = fb.film(image, **setting)
        assert np.isnan(want[3, 4, 1]) and not np.isfinite(want[20, 30, 0]) and not np.isfinite(want[30, 10, 2]) and np.isfinite(want).any()
        for naive, unaligned in forms:
            out, rgba, rgba2, _ = run_gpu(rtc, image, naive, unaligned, **setting)
            assert fb.close(out, want)[1], setting
            for kind in (np.isnan, np.isposinf, np.isneginf):
                assert np.array_equal(kind(out), kind(want)), (setting, kind.__name__)
            assert np.array_equal(rgba, rgba2)


# ---- Progressive and AdaptiveProgressive on the fixture emitters_mix.json
@pytest.fixture(scope="module")
def mix_run(rtc):
    """emitters_mix.json at 80 x 45, 8 passes: the Progressive object and what it and rtc_render_denoised leave, computed once
    and left unchanged"""
    import torch
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    prog = rtc.Progressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH)
    for _ in range(PASSES):
        prog.step()
    mean, denoised = prog.mean().cpu().numpy(), prog.denoised().cpu().numpy()
    torch.cuda.synchronize()
    for a in (mean, denoised):
        a.setflags(write=False)
    return hs, cam, prog, mean, denoised


LAMP = dict(exposure=0.8, bloom_radius=6, bloom_sigma=2.0, bloom_threshold=1.0, bloom_intensity=0.2)


def _tensors(pair):
    import torch
    out, rgba = pair[0].cpu().numpy(), pair[1].cpu().numpy()
    torch.cuda.synchronize()
    return out, rgba


def _rgba_bytes(px):
    return np.ascontiguousarray(px).view(np.uint8).reshape(px.shape + (4,))


def test_progressive_filmed_is_the_checkers(rtc, mix_run):
    hs, cam, prog, mean, denoised = mix_run
    for setting in ({}, LAMP, dict(LAMP, auto_key=0.18, curve="hable", transfer="gamma")):
        out, rgba = _tensors(prog.filmed(**setting))
        numbers = rtc.FilmSetting.make(**setting).to_dict()
        own, own_E = fb.film(mean, **numbers)
        err, ok = fb.close(out, own)           # (with the automatic exposure the checker's own E: some 1e-14 from the GPU's, and so is E * in)
        print(f"Progressive.filmed({setting}) against the checker: {err:.3e}")
        assert ok, err
        assert rgba.shape == (H, W, 4) and np.array_equal(rgba, _rgba_bytes(fb.rgba(out)))
    out, _ = _tensors(prog.filmed(denoise={}, **LAMP))
    err, ok = fb.close(out, fb.film(denoised, **rtc.FilmSetting.make(**LAMP).to_dict())[0])
    print(f"Progressive.filmed(denoise={{}}) against the checker on denoised(): {err:.3e}")
    assert ok, err
    small = dict(radius=2, patch=1, strength=0.3)
    out, _ = _tensors(prog.filmed(denoise=small))
    assert fb.close(out, fb.film(prog.denoised(**small).cpu().numpy())[0])[1]


def test_adaptive_filmed_is_the_checkers(rtc, mix_run):
    import torch
    hs, cam, _, _, _ = mix_run
    adaptive = rtc.Adaptive.make(0.03, PASSES, min_passes=2, tile=16)
    run = rtc.AdaptiveProgressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH, adaptive=adaptive)
    run.run()
    mean, denoised = run.mean().cpu().numpy(), run.denoised().cpu().numpy()
    torch.cuda.synchronize()
    numbers = rtc.FilmSetting.make(**LAMP).to_dict()
    out, rgba = _tensors(run.filmed(**LAMP))
    err, ok = fb.close(out, fb.film(mean, **numbers)[0])
    print(f"AdaptiveProgressive.filmed() against the checker: {err:.3e}")
    assert ok and np.array_equal(rgba, _rgba_bytes(fb.rgba(out))), err
    out, _ = _tensors(run.filmed(denoise={}, **LAMP))
    err, ok = fb.close(out, fb.film(denoised, **numbers)[0])
    print(f"AdaptiveProgressive.filmed(denoise={{}}) against the checker on denoised(): {err:.3e}")
    assert ok, err


# ---- the convenience calls
def test_render_filmed_is_progressive_filmed_and_restores_the_pass(rtc, mix_run):
    hs, cam, prog, mean, denoised = mix_run
    film = rtc.FilmSetting.make(**LAMP)
    gpu = eg.handle(rtc, hs, hs.sampling(), sample_pass=3)
    before = gpu.render(cam, DEPTH)
    rgb, rgba, linear = gpu.render_filmed(cam, PASSES, film=film, max_depth=DEPTH)
    assert np.array_equal(gpu.render(cam, DEPTH), before)                      # (the handle is still at pass 3 ...)
    gpu.set_sample_pass(0)
    assert not np.array_equal(gpu.render(cam, DEPTH), before)                  # (... which is not pass 0's image)
    gpu.set_sample_pass(3)
    want, want_rgba = _tensors(prog.filmed(**LAMP))
    assert same_bits(rgb, want) and np.array_equal(rgba, want_rgba) and same_bits(linear, mean)
    # the defaults, and one pass alone
    rgb0, _, linear0 = gpu.render_filmed(cam, PASSES, max_depth=DEPTH)
    assert same_bits(rgb0, _tensors(prog.filmed())[0]) and same_bits(linear0, mean)
    one, _, frame = gpu.render_filmed(cam, 1, film=film, max_depth=DEPTH)
    gpu.set_sample_pass(0)
    assert same_bits(frame, gpu.render(cam, DEPTH)) and not same_bits(one, rgb)
    # with the denoiser: linear_out is rtc_render_denoised's image, rgb_out the film over it
    dn = rtc.DenoiseSetting.make()
    den_rgb, den_noisy = gpu.render_denoised(cam, PASSES, max_depth=DEPTH)
    rgb2, rgba2, linear2 = gpu.render_filmed(cam, PASSES, denoise=dn, film=film, max_depth=DEPTH)
    assert same_bits(linear2, den_rgb) and same_bits(den_rgb, denoised) and same_bits(den_noisy, mean)
    want2, want_rgba2 = _tensors(prog.filmed(denoise={}, **LAMP))
    assert same_bits(rgb2, want2) and np.array_equal(rgba2, want_rgba2)
    # an adaptive run, with and without the denoiser
    adaptive = rtc.Adaptive.make(0.03, PASSES, min_passes=2, tile=16)
    run = rtc.AdaptiveProgressive(eg.handle(rtc, hs, hs.sampling()), cam, DEPTH, adaptive=adaptive)
    run.run()
    rgb3, _, linear3 = gpu.render_filmed(cam, 0, adaptive=adaptive, film=film, max_depth=DEPTH)
    assert same_bits(linear3, run.mean().cpu().numpy()) and same_bits(rgb3, _tensors(run.filmed(**LAMP))[0])
    rgb4, _, linear4 = gpu.render_filmed(cam, 0, adaptive=adaptive, denoise=dn, film=film, max_depth=DEPTH)
    assert same_bits(linear4, gpu.render_denoised(cam, 0, adaptive=adaptive, max_depth=DEPTH)[0])
    assert same_bits(rgb4, _tensors(run.filmed(denoise={}, **LAMP))[0])


def test_host_render_of_the_lamp_fixture(rtc):
    """rtch_scene_render of a file with the key goes through rtc_render_filmed; and the film keeps the highlights the plain
    clamp cuts flat (the two shares with the CPU checkers: tests/test_film_cpu.py)"""
    hs = rtc.HostScene.from_file(fb.FILM_LAMP)
    film = hs.film()
    assert film is not None and film.bloom_radius == 6 and hs.passes() == PASSES
    cam = hs.camera()
    out = np.zeros((cam.vsize, cam.hsize, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    rgb, rgba, linear = eg.handle(rtc, hs, hs.sampling()).render_filmed(cam, hs.passes(), film=film, max_depth=DEPTH)
    assert same_bits(out, rgb) and not np.array_equal(out, linear)
    err, ok = fb.close(rgb, fb.film(linear, **film.to_dict())[0])
    print(f"film_lamp.json against the checker on linear_out: {err:.3e}")
    assert ok, err
    filmed, clamped = fb.share_at_255(rgba.view(np.uint32)[..., 0]), fb.share_at_255(fb.rgba(linear))
    print(f"share of channels at 255: film {filmed:.4f}, plain clamp {clamped:.4f}")
    assert linear.max() >= 20.0 and filmed < clamped
