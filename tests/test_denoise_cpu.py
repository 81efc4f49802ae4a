"""The denoiser without a GPU: the symbols, the structs and the constants, every refusal of
rtc_denoise_device and rtc_render_denoised made with stand-in pointers, the loader's "denoise" key and rtch_scene_denoise, and
the checker (tests/cpp/denoise_oracle.cpp) - its exact properties, what it does to i.i.d. noise on a flat and on a step
image, and the fixture emitters_mix.json rendered by the emitter checker: 8 passes against the mean of passes 32 .. 159.

Measured with the checker (defaults 7, 2, 0.45, 1.0; the bounds are the issue's): flat 32 x 32, sigma 0.2, 8 passes: RMSE
ratio 9.2 (bound 4); step 0.2 / 0.8: 6.1 (bound 3), mean |error| of the four columns beside the edge at most 0.022 (bound
0.1); the fixture: 1.378 at 80 x 45 (bound 1.2) and 2.170 at 240 x 135 (bound 1.7).  The variant without the c3 term gives
1.9 on the flat image, 1.6 on the step, 1.10 and 1.37 on the fixture: it misses every ratio.  A variant whose variance is
not divided by 3 misses none of them (12.9, 8.0, 1.70, 2.35: it only smooths more), so the checker carries no such variant:
these bounds cannot tell that mistake, the parity of the GPU with the checker does."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import denoise_binding as db
import emitters_binding as mb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
FAKE = 0x7F0000001000   # (never dereferenced: validation comes first)
NEW = ["rtc_denoise_device", "rtc_render_denoised"]
DEPTH = 5


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


# ---- ABI
def test_symbols_structs_and_constants(rtc):
    assert set(NEW) <= set(rtc.RTC_SYMBOLS) and "rtch_scene_denoise" in rtc.HOST_SYMBOLS and "rtc_diag_denoise_tile" in rtc.RTC_DIAG_SYMBOLS
    for n in NEW + ["rtc_diag_denoise_tile"]:
        assert getattr(rtc.hip_lib(), n) is not None
    assert rtc.host_lib().rtch_scene_denoise is not None
    S, D = rtc.DenoiseSetting, rtc.Denoise
    assert C.sizeof(S) == 24 and (S.radius.offset, S.patch.offset, S.strength.offset, S.cancel.offset) == (0, 4, 8, 16)
    assert C.sizeof(D) == 88
    assert (D.mean.offset, D.sumsq.offset, D.hsize.offset, D.vsize.offset, D.passes.offset, D.tile_passes.offset, D.tile_w.offset,
            D.tile_h.offset, D.setting.offset, D.out.offset, D.rgba.offset) == (0, 8, 16, 20, 24, 32, 40, 44, 48, 72, 80)
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("#define RTC_DENOISE_MAX_RADIUS 10u", "#define RTC_DENOISE_MAX_PATCH 3u", "#define RTC_DENOISE_EPS 1e-10",
                 "#define RTC_ABI_VERSION 3u", "typedef struct rtc_denoise_setting {", "typedef struct rtc_denoise {",
                 "int rtc_denoise_device(const rtc_denoise *d, void *hip_stream);"):
        assert line in header, line
    assert (rtc.DENOISE_MAX_RADIUS, rtc.DENOISE_MAX_PATCH, rtc.DENOISE_EPS) == (10, 3, 1e-10)
    assert rtc.DenoiseSetting.make().to_dict() == db.DEFAULTS
    assert "denoise_naive" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "rtch_scene_denoise" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    assert "rtc_denoise" not in open(os.path.join(REPO, "include", "rtc_multi.h")).read()   # (librtc_multi does not get it)
    rtc.set_option("denoise_naive", 1)
    rtc.set_option("denoise_naive", 0)
    tw, th = rtc.denoise_tile()
    assert tw >= 1 and th >= 1
    zig = open(os.path.join(REPO, "integration", "gpu.zig")).read()
    assert "rtc_denoise_device" in zig and "rtc_render_denoised" in zig and "RtcDenoise" in zig and "RtcDenoiseSetting" in zig


def test_headers_are_still_strict_c99_and_the_binding_matches():
    import test_abi
    test_abi.test_headers_are_valid_c()
    test_abi.test_zig_binding_matches_the_header()


def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("v(x, y) = P < 2 ? 0.0 : max(0, s - P * ((u.r * u.r + u.g * u.g) + u.b * u.b)) / (3.0 * ((P - 1.0) * P))",
                 "t   = ((D.r * D.r + D.g * D.g) + D.b * D.b) - c3 * (v(a) + min(v(a), v(b)))",
                 "S   = S + t / (RTC_DENOISE_EPS + k2 * (v(a) + v(b)));   n = n + 1",
                 "w = exp(-max(0, S / (3.0 * n)));   W = W + w;   A.c = A.c + w * u.c(q)",
                 "radius 0 returns the mean to the bit", "librtc_multi renders without it"):
        assert line in header, line


# ---- rtc_denoise_device: every refusal, with stand-in pointers and no device
GOOD = dict(mean=FAKE, sumsq=FAKE + 0x100000, hsize=64, vsize=48, passes=8, tile_passes=None, tile_w=0, tile_h=0, radius=7, patch=2,
            strength=0.45, cancel=1.0, out=FAKE + 0x200000, rgba=None)
MEAN_BYTES = 64 * 48 * 24
BAD = [
    (dict(mean=None), "null"), (dict(sumsq=None), "null"), (dict(out=None), "null"),
    (dict(hsize=0), "image"), (dict(vsize=0), "image"), (dict(hsize=1 << 21, vsize=(1 << 19) + 1), "image"),
    (dict(radius=11), "radius"), (dict(patch=4), "patch"), (dict(radius=0xFFFFFFFF), "radius"),
    (dict(strength=0.0), "strength"), (dict(strength=-1.0), "strength"), (dict(strength=float("nan")), "strength"),
    (dict(strength=float("inf")), "strength"),
    (dict(cancel=-1e-9), "cancel"), (dict(cancel=float("nan")), "cancel"), (dict(cancel=float("inf")), "cancel"),
    (dict(passes=1), "passes"), (dict(passes=0), "passes"),
    (dict(tile_passes=FAKE + 0x300000, tile_w=0, tile_h=16), "tile"), (dict(tile_passes=FAKE + 0x300000, tile_w=16, tile_h=1025), "tile"),
    (dict(out=FAKE), "overlaps"), (dict(out=FAKE + MEAN_BYTES - 8), "overlaps"), (dict(out=FAKE - MEAN_BYTES + 8), "overlaps"),
]


def _denoise(rtc, **kw):
    v = dict(GOOD)
    v.update(kw)
    return rtc.Denoise(v["mean"], v["sumsq"], v["hsize"], v["vsize"], v["passes"], v["tile_passes"], v["tile_w"], v["tile_h"],
                       rtc.DenoiseSetting(v["radius"], v["patch"], v["strength"], v["cancel"]), v["out"], v["rgba"])


@pytest.mark.parametrize("bad, word", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b, _ in BAD])
def test_each_invalid_argument_is_refused_before_the_device(rtc, bad, word):
    lib = rtc.hip_lib()
    d = _denoise(rtc, **bad)
    assert _status(lib, lib.rtc_denoise_device(C.byref(d), FAKE)) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert "denoise:" in text and word in text, text


def test_null_struct_and_null_stream_are_refused(rtc):
    lib = rtc.hip_lib()
    assert _status(lib, lib.rtc_denoise_device(None, FAKE)) == "InvalidArgument"
    assert _status(lib, lib.rtc_denoise_device(C.byref(_denoise(rtc)), None)) == "InvalidArgument"
    assert _status(lib, lib.rtc_diag_denoise_tile(None, None)) == "InvalidArgument"


def test_render_denoised_refuses_on_the_host_and_touches_nothing(rtc):
    lib = rtc.hip_lib()
    handle = (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))
    h = C.cast(handle, C.c_void_p)
    cam = rtc.make_camera(64, 48, 1.0, (0, 1.5, -5), (0, 1, 0), (0, 1, 0))
    out = np.zeros((48, 64, 3))
    ok = rtc.DenoiseSetting.make()
    adaptive = rtc.Adaptive.make(0.01, 8)
    calls = [(None, cam, 8, None, ok, out.ctypes.data), (h, cam, 8, None, ok, None), (h, None, 8, None, ok, out.ctypes.data),
             (h, cam, 1, None, ok, out.ctypes.data), (h, cam, 0, None, ok, out.ctypes.data),
             (h, cam, 8, None, rtc.DenoiseSetting.make(radius=11), out.ctypes.data),
             (h, cam, 8, None, rtc.DenoiseSetting.make(strength=0.0), out.ctypes.data),
             (h, cam, 8, None, rtc.DenoiseSetting.make(cancel=-1.0), out.ctypes.data),
             (h, cam, 8, rtc.Adaptive.make(0.01, 8, tile=0), ok, out.ctypes.data),
             (h, cam, 8, rtc.Adaptive.make(0.01, 3, min_passes=4), ok, out.ctypes.data),
             # (the stand-in's samples per pixel read as 0xA5A5A5A5: no pass count fits the sample index)
             (h, cam, 8, None, ok, out.ctypes.data), (h, cam, 8, adaptive, ok, out.ctypes.data)]
    for s, c, passes, a, setting, o in calls:
        st = lib.rtc_render_denoised(s, C.byref(c) if c is not None else None, DEPTH, passes, C.byref(a) if a is not None else None,
                                     C.byref(setting), o, None)
        assert _status(lib, st) == "InvalidArgument", (passes, lib.rtc_last_error())
    assert bytes(handle) == b"\xa5" * SENTINEL and not out.any()


# ---- the loader
def _scene(sampling=None):
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}], "objects": [{"type": {"sphere": {}}}]}
    if sampling is not None:
        s["camera"]["sampling"] = sampling
    return json.dumps(s)


@pytest.mark.parametrize("sampling, want", [
    (None, None), ({"passes": 8}, None), ({"passes": 8, "denoise": False}, None),
    ({"passes": 2, "denoise": True}, db.DEFAULTS), ({"passes": 8, "denoise": {}}, db.DEFAULTS),
    ({"passes": 8, "denoise": {"radius": 0, "patch": 0}}, dict(db.DEFAULTS, radius=0, patch=0)),
    ({"passes": 8, "denoise": {"radius": 10, "patch": 3, "strength": 0.7, "cancel": 0}}, {"radius": 10, "patch": 3, "strength": 0.7, "cancel": 0.0}),
    ({"passes": 8, "adaptive": {"threshold": 0.01}, "denoise": True}, db.DEFAULTS),
    ({"passes": 1, "denoise": False}, None),
])
def test_loader_reads_the_key(rtc, sampling, want):
    hs = rtc.HostScene(_scene(sampling))
    d = hs.denoise()
    assert (d.to_dict() if d is not None else None) == want


@pytest.mark.parametrize("sampling, error", [
    ({"passes": 8, "denoise": {"radius": 7, "window": 3}}, "UnknownField"),
    ({"passes": 8, "denoise": {"radius": 11}}, "InvalidData"), ({"passes": 8, "denoise": {"radius": -1}}, "InvalidData"),
    ({"passes": 8, "denoise": {"radius": 1.5}}, "InvalidData"), ({"passes": 8, "denoise": {"radius": "7"}}, "InvalidData"),
    ({"passes": 8, "denoise": {"patch": 4}}, "InvalidData"),
    ({"passes": 8, "denoise": {"strength": 0}}, "InvalidData"), ({"passes": 8, "denoise": {"strength": -0.45}}, "InvalidData"),
    ({"passes": 8, "denoise": {"strength": True}}, "InvalidData"),
    ({"passes": 8, "denoise": {"cancel": -1}}, "InvalidData"), ({"passes": 8, "denoise": {"cancel": [1]}}, "InvalidData"),
    ({"passes": 8, "denoise": 7}, "InvalidData"), ({"passes": 8, "denoise": "on"}, "InvalidData"), ({"passes": 8, "denoise": None}, "InvalidData"),
    ({"denoise": True}, "InvalidData"), ({"passes": 1, "denoise": {}}, "InvalidData"),
])
def test_loader_refuses(rtc, sampling, error):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(sampling))
    assert e.value.name == error, e.value.args


def test_the_key_changes_no_table(rtc):
    """A file without the key, with it false and with it set flatten to the same tables and the same digest."""
    plain = rtc.HostScene(_scene({"passes": 8}))
    base = rtc.build_tables_digest(plain.desc)[0]
    counts = [getattr(plain.desc, f) for f, t in rtc.SceneDesc._fields_ if t is C.c_uint32]
    for sampling in (None, {"passes": 8, "denoise": False}, {"passes": 8, "denoise": True}, {"passes": 8, "denoise": {"radius": 3}}):
        hs = rtc.HostScene(_scene(sampling))
        assert rtc.build_tables_digest(hs.desc)[0] == base
        assert [getattr(hs.desc, f) for f, t in rtc.SceneDesc._fields_ if t is C.c_uint32] == counts
    mix = mb.mix(rtc)
    scene = json.loads(open(mb.EMITTERS_MIX).read())
    scene["camera"]["sampling"].update(passes=8, denoise=True)
    assert rtc.build_tables_digest(rtc.HostScene(json.dumps(scene)).desc)[0] == rtc.build_tables_digest(mix.desc)[0]
    assert mix.denoise() is None


# ---- the checker's exact properties
def _noisy(truth, passes, seed, sigma=0.2):
    rng = np.random.default_rng(seed)
    return db.accumulate([truth + rng.normal(0.0, sigma, truth.shape) for _ in range(passes)])


def test_radius_0_returns_the_means_bits():
    mean, sumsq = _noisy(np.full((9, 13, 3), 0.5), 4, seed=3)
    for patch in (0, 2, 3):
        assert np.array_equal(db.denoise(mean, sumsq, 4, radius=0, patch=patch), mean)


def test_a_constant_image_stays_constant():
    mean = np.full((11, 7, 3), 0.3)
    for sumsq in (np.full((11, 7), 8 * 0.27), np.full((11, 7), 8 * 0.27 + 0.5)):      # (variance 0, and well above it)
        assert np.abs(db.denoise(mean, sumsq, 8) - 0.3).max() <= 1e-15


def tiles_case():
    """5 x 3 tiles over 17 x 11, every tile at its own pass count, tile 5 at P_t = 1 -> (mean, sumsq, tile_passes, tile, the rows
    and columns of tile 5).  The tiles with two passes or more are 0.5 with noise of variance about 4e-4 and say so in their
    sums of squares; the tile with one pass holds values from 2 to 3."""
    rng = np.random.default_rng(11)
    v = 4e-4 * rng.uniform(0.8, 1.2, (11, 17))
    mean = 0.5 + rng.normal(0.0, 1.0, (11, 17, 3)) * np.sqrt(v)[..., None]
    where = (slice(3, 6), slice(5, 10))
    mean[where] = rng.uniform(2.0, 3.0, (3, 5, 3))
    tile_passes = np.array([4, 8, 2, 5, 6, 1, 3, 7, 4, 2, 9, 5, 3, 6, 8, 2], dtype=np.uint32)
    p = np.repeat(np.repeat(tile_passes.reshape(4, 4), 3, axis=0), 5, axis=1)[:11, :17].astype(np.float64)
    sumsq = p * (mean ** 2).sum(axis=2) + 3.0 * (p - 1.0) * p * v
    return mean, sumsq, tile_passes, (5, 3), where


def test_a_tile_with_one_pass_passes_through_to_the_bit():
    """The tile at P_t = 1 has variance 0 by the rule, not by a division by P - 1 = 0.  Its values match no other patch: beside
    another pixel of the tile a term is a squared difference over eps, and against a pixel of another tile the patch's own
    centre alone adds 3 * 1.5^2 / (k2 * 1e-3) / (3 * 25) > 400 to the exponent - every weight but a pixel's own is below
    1e-170, and 1 + 1e-170 is 1.  The other tiles are smoothed."""
    mean, sumsq, tile_passes, tile, where = tiles_case()
    out = db.denoise(mean, sumsq, tile_passes=tile_passes, tile=tile)
    assert np.array_equal(out[where], mean[where])
    outside = np.ones((11, 17), dtype=bool)
    outside[where] = False
    assert np.isfinite(out).all() and (out[outside] != mean[outside]).mean() > 0.5
    assert np.abs(out[outside] - 0.5).mean() < 0.5 * np.abs(mean[outside] - 0.5).mean()


def test_a_window_larger_than_the_image_gives_finite_output():
    mean, sumsq = _noisy(np.full((2, 3, 3), 0.5), 8, seed=5)
    out = db.denoise(mean, sumsq, 8, radius=10, patch=3)
    assert np.isfinite(out).all() and out.min() >= mean.min() and out.max() <= mean.max()


# ---- i.i.d. noise: conditions, not measurements (a filter that does not do this on i.i.d. noise is broken)
def _flat_and_step():
    flat = np.full((32, 32, 3), 0.5)
    step = np.full((32, 32, 3), 0.2)
    step[:, 16:] = 0.8
    return flat, step


def _ratios(flags):
    flat, step = _flat_and_step()
    fm, fs = _noisy(flat, 8, seed=1)
    sm, ss = _noisy(step, 8, seed=1)
    f_out, s_out = db.denoise(fm, fs, 8, flags=flags), db.denoise(sm, ss, 8, flags=flags)
    edge = [float(np.abs(s_out[:, c] - step[:, c]).mean()) for c in (14, 15, 16, 17)]
    return db.rmse(fm, flat) / db.rmse(f_out, flat), db.rmse(sm, step) / db.rmse(s_out, step), edge


def test_flat_and_step_images_at_8_passes():
    flat_ratio, step_ratio, edge = _ratios(0)
    print(f"flat {flat_ratio:.3f} (>= 4), step {step_ratio:.3f} (>= 3), edge columns {edge} (<= 0.1)")
    assert flat_ratio >= 4.0 and step_ratio >= 3.0
    assert max(edge) <= 0.1


def test_without_the_variance_cancellation_the_bounds_are_missed():
    flat_ratio, step_ratio, _ = _ratios(db.NO_CANCEL)
    print(f"no c3 term: flat {flat_ratio:.3f}, step {step_ratio:.3f}")
    assert flat_ratio < 4.0 and step_ratio < 3.0


# ---- the fixture: passes 0 .. 7 against the mean of passes 32 .. 159, both from the emitter checker
@pytest.fixture(scope="module")
def fixture_passes(rtc):
    """(mean, sumsq, reference) per size, computed once and left unchanged"""
    hs = mb.mix(rtc)
    ck = mb.scene_of(rtc, hs)
    out = {}
    for w, h in ((80, 45), (240, 135)):
        cam = hs.camera(w, h)
        render = lambda p: ck.render(cam, DEPTH, hs.sampling(), hs.spots(), sample_pass=p)[0]
        mean, sumsq = db.accumulate([render(p) for p in range(8)])
        total = np.zeros_like(mean)
        for p in range(32, 160):
            total += render(p)
        out[(w, h)] = (mean, sumsq, total / 128.0)
        for a in out[(w, h)]:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("size, bound", [((80, 45), 1.2), ((240, 135), 1.7)])
def test_fixture_rmse_ratio(fixture_passes, size, bound):
    mean, sumsq, ref = fixture_passes[size]
    out = db.denoise(mean, sumsq, 8)
    noisy, den = db.rmse(mean, ref), db.rmse(out, ref)
    print(f"{size}: RMSE noisy {noisy:.5f}, denoised {den:.5f}, ratio {noisy / den:.3f} (>= {bound})")
    assert noisy / den >= bound
    bare = db.denoise(mean, sumsq, 8, flags=db.NO_CANCEL)
    print(f"{size}: without the c3 term {noisy / db.rmse(bare, ref):.3f}")
    assert noisy / db.rmse(bare, ref) < bound


# ---- documents and build
def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 29." in design
    for word in ("rtc_denoise_device", "rtc_render_denoised", "rtc_denoise_kernel_p2", "rtc_denoise_naive_kernel", "denoise_naive",
                 "Rousselle", "tests/cpp/denoise_oracle.cpp", "profiles/denoise/object_identity.txt", "profiles/denoise/times_1080p.txt",
                 "emitters_mix.json", "Out of scope", "librtc_multi", "Firefly"):
        assert word in design, word
    for doc, word in (("README.md", "rtc_denoise_device"), ("README.md", "\"denoise\""), ("INTEGRATION.md", "rtc_denoise_device"),
                      ("INTEGRATION.md", "RtcDenoiseSetting"), (os.path.join("tools", "README.md"), "--denoise"),
                      (os.path.join("profiles", "HISTORY.md"), "denoiser")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resource rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_denoise_kernel_p0", "rtc_denoise_kernel_p1", "rtc_denoise_kernel_p2", "rtc_denoise_kernel_p3", "rtc_denoise_naive_kernel"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} |" in design, name
            assert k["vgprs_spilled"] == 0 and k["scratch_bytes_per_lane"] == 0


def test_object_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "denoise", "object_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_kernels_ext.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o",
                "rtc_occlusion.o", "rtc_shadowfilter.o", "rtc_media.o", "rtc_environment.o", "rtc_skylight.o", "rtc_indirect.o",
                "rtc_emitters.o", "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    assert "rtc_capi.o" in text and "kernel_resources.json" in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_denoise.o", "rtc_denoise.remarks", "libdenoise_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_denoise.hip")).read()
    assert "static_assert(ldsDoubles(kMaxStage, kMaxStage, kMaxPair) * sizeof(double) <= kLdsLimit" in unit
    assert "rtc_kernels.hip" not in unit and "rtc_device.h" not in unit      # (a unit of its own: no render kernel compiles in it)
    oracle = open(os.path.join(REPO, "tests", "cpp", "denoise_oracle.cpp")).read()
    assert "#include \"" not in oracle                                        # (the checker includes nothing of the product)
