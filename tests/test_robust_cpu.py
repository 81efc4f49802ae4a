"""Robust accumulation without a GPU: the symbols, the structs and the constants, every refusal of
rtc_robust_device and rtc_render_robust made with stand-in pointers, the loader's "robust" key and rtch_scene_robust, and the
checker (tests/cpp/robust_oracle.cpp): known answers on one pixel, a synthetic image with and without spikes, the variance
the denoiser recovers, gain 0, and the fixture robust_lamp.json rendered by the emitter checker.

Measured with the checkers (printed by the tests):
  synthetic 32 x 32, sigma 0.2, a spike of +40 on a twentieth of the pixels: RMSE plain / robust 14.41 at (P, M) = (8, 5) and
  11.12 at (16, 5); without spikes robust / plain 1.006 (M = 3), 1.007 (5), 1.019 (7) at 16 passes; sqrt(mean v) 0.0507
  against a measured RMSE of 0.0496.
  robust_lamp.json at 80 x 45, 16 passes, M = 5, gain 1: speck share plain 0.0028, robust 0.0019; RMSE against the mean of
  passes 32 .. 159 plain 0.1098, robust 0.0543, ratio 2.022 (bound 2.022 - (2.022 - 1) / 3 = 1.681).
  emitters_mix.json likewise: mean luminance robust / plain 0.9957 (bound: within 0.0043 + 0.02 of 1)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import denoise_binding as db
import emitters_binding as mb
import robust_binding as rb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
FAKE = 0x7F0000001000   # (never dereferenced: validation comes first)
NEW = ["rtc_robust_device", "rtc_render_robust"]
DEPTH = 5
NAN, INF = float("nan"), float("inf")
LAMP_RATIO = 2.022      # (measured: the docstring)
LAMP_BOUND = LAMP_RATIO - (LAMP_RATIO - 1.0) / 3.0
MIX_LOSS = 0.0043       # (measured: 1 - 0.9957)


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


# ---- ABI
def test_symbols_structs_and_constants(rtc):
    assert set(NEW) <= set(rtc.RTC_SYMBOLS) and "rtch_scene_robust" in rtc.HOST_SYMBOLS and "rtc_diag_robust_grid" in rtc.RTC_DIAG_SYMBOLS
    for n in NEW + ["rtc_diag_robust_grid"]:
        assert getattr(rtc.hip_lib(), n) is not None
    assert rtc.host_lib().rtch_scene_robust is not None
    S, R = rtc.RobustSetting, rtc.Robust
    assert C.sizeof(S) == 16 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 8]
    assert C.sizeof(R) == 72 and [getattr(R, n).offset for n, _ in R._fields_] == [0, 8, 16, 24, 40, 48, 56, 64]
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("#define RTC_ROBUST_MAX_BUCKETS 15u", "#define RTC_ABI_VERSION 3u", "typedef struct rtc_robust_setting {",
                 "typedef struct rtc_robust {", "int rtc_robust_device(const rtc_robust *r, void *hip_stream);",
                 "int rtc_render_robust(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth, uint32_t passes,"):
        assert line in header, line
    assert rtc.ROBUST_MAX_BUCKETS == 15
    assert rtc.RobustSetting.make().to_dict() == rb.DEFAULTS
    assert rtc.RobustSetting.make(buckets=7, gain=0.5).to_dict() == {"buckets": 7, "gain": 0.5}
    assert "robust_naive" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "rtch_scene_robust" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    assert "rtc_robust" not in open(os.path.join(REPO, "include", "rtc_multi.h")).read()   # (librtc_multi does not get it)
    rtc.set_option("robust_naive", 1)
    rtc.set_option("robust_naive", 0)
    max_blocks, block = rtc.robust_grid()
    assert max_blocks >= 1 and block % 64 == 0
    zig = open(os.path.join(REPO, "integration", "gpu.zig")).read()
    for word in ("rtc_scene_accumulate_device", "rtc_robust_device", "rtc_render_robust", "RtcRobust", "RtcRobustSetting", "RtcAccum"):
        assert word in zig, word


def test_headers_are_still_strict_c99_and_the_binding_matches():
    import test_abi
    test_abi.test_headers_are_valid_c()
    test_abi.test_zig_binding_matches_the_header()


def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("m_j.c = sums[j].c / (double)n_j", "y_j = (0.2126 * m_j.r + 0.7152 * m_j.g) + 0.0722 * m_j.b",
                 "k_j = (y_j - y_j == 0) ? (y_j > 0 ? y_j : 0.0) : +infinity", "k_i < k_j || (k_i == k_j && i < j)",
                 "T = sum k_j;   A = sum (double)(rank_j + 1) * k_j",
                 "G0 = (T > 0 && T < infinity) ? (2.0 * A) / ((double)M * T) - (double)(M + 1) / (double)M : (T > 0 ? 1.0 : 0.0)",
                 "g = gain * G0;   G = g > 0 ? (g < 1 ? g : 1.0) : 0.0",
                 "c = min(h, (uint32_t)floor((1.0 - G) * (double)h + 0.5)) and k = 2 c + 1", "h - c <= rank_j <= h + c",
                 "rejected_out = M - k", "cv = c > 1 ? c : 1 and kv = 2 cv + 1", "v = D / (3.0 * ((double)(kv - 1) * (double)kv))",
                 "sumsq_out = P * ((u.r * u.r + u.g * u.g) + u.b * u.b) + (3.0 * ((P - 1.0) * P)) * v",
                 "sum = sums + (p % M) * n * 3", "passes = p / M + 1", "n_j = P / M + (j < P % M ? 1 : 0)",
                 "no library function is involved", "the same bits", "is NOT the plain mean", "NULL means NO film stage",
                 "fewer than half of the buckets do not reach mean_out", "librtc_multi renders"):
        assert line in header, line


# ---- rtc_robust_device: every refusal, with stand-in pointers and no device
N = 64 * 48
GOOD = dict(sums=FAKE, n_pixels=N, passes=16, buckets=5, gain=1.0, mean_out=FAKE + 0x400000, sumsq_out=FAKE + 0x500000,
            rejected_out=None, rgba=None)
SUMS_BYTES = 5 * N * 24
BAD = [
    (dict(sums=None), "null"), (dict(mean_out=None), "null"),
    (dict(n_pixels=0), "pixels"), (dict(n_pixels=(1 << 40) + 1), "pixels"),
    (dict(buckets=4), "buckets"), (dict(buckets=0), "buckets"), (dict(buckets=1), "buckets"), (dict(buckets=2), "buckets"),
    (dict(buckets=16), "buckets"), (dict(buckets=17), "buckets"), (dict(buckets=0xFFFFFFFF), "buckets"),
    (dict(passes=4), "passes"), (dict(passes=0), "passes"), (dict(passes=14, buckets=15), "passes"),
    (dict(gain=-0.5), "gain"), (dict(gain=NAN), "gain"), (dict(gain=INF), "gain"), (dict(gain=-INF), "gain"),
    (dict(mean_out=FAKE), "mean_out"), (dict(mean_out=FAKE + SUMS_BYTES - 8), "mean_out"), (dict(mean_out=FAKE - N * 24 + 8), "mean_out"),
    (dict(mean_out=FAKE + 2 * N * 24), "mean_out"),
    (dict(sumsq_out=FAKE), "sumsq_out"), (dict(sumsq_out=FAKE + SUMS_BYTES - 8), "sumsq_out"), (dict(sumsq_out=FAKE - N * 8 + 8), "sumsq_out"),
]


def _robust(rtc, **kw):
    v = dict(GOOD)
    v.update(kw)
    return rtc.Robust(v["sums"], v["n_pixels"], v["passes"], rtc.RobustSetting(v["buckets"], v["gain"]), v["mean_out"], v["sumsq_out"],
                      v["rejected_out"], v["rgba"])


def _ids(cases):
    return [",".join(f"{k}={v}" for k, v in b.items()) for b, _ in cases]


@pytest.mark.parametrize("bad, word", BAD, ids=_ids(BAD))
def test_each_invalid_argument_is_refused_before_the_device(rtc, bad, word):
    lib = rtc.hip_lib()
    r = _robust(rtc, **bad)
    assert _status(lib, lib.rtc_robust_device(C.byref(r), FAKE)) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert "robust:" in text and word in text, text


def test_null_struct_and_null_stream_are_refused(rtc):
    lib = rtc.hip_lib()
    assert _status(lib, lib.rtc_robust_device(None, FAKE)) == "InvalidArgument"
    assert _status(lib, lib.rtc_robust_device(C.byref(_robust(rtc)), None)) == "InvalidArgument"
    assert _status(lib, lib.rtc_diag_robust_grid(None, None)) == "InvalidArgument"


def test_render_robust_refuses_on_the_host_and_touches_nothing(rtc):
    lib = rtc.hip_lib()
    handle = (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))
    h = C.cast(handle, C.c_void_p)
    cam = rtc.make_camera(64, 48, 1.0, (0, 1.5, -5), (0, 1, 0), (0, 1, 0))
    out = np.zeros((48, 64, 3))
    px = np.zeros((48, 64, 4), dtype=np.uint8)
    o, p = out.ctypes.data, px.ctypes.data
    rs, dn, fs = rtc.RobustSetting.make, rtc.DenoiseSetting.make, rtc.FilmSetting.make
    calls = [(None, cam, 16, None, None, None, o, p), (h, cam, 16, None, None, None, None, None), (h, None, 16, None, None, None, o, p),
             (h, cam, 16, rs(buckets=4), None, None, o, p), (h, cam, 16, rs(buckets=1), None, None, o, p),
             (h, cam, 16, rs(buckets=17), None, None, o, p), (h, cam, 16, rs(gain=-1.0), None, None, o, p),
             (h, cam, 16, rs(gain=NAN), None, None, o, p), (h, cam, 16, rs(gain=INF), None, None, o, p),
             (h, cam, 4, None, None, None, o, p), (h, cam, 0, None, None, None, o, p), (h, cam, 6, rs(buckets=7), None, None, o, p),
             (h, cam, 16, None, dn(radius=11), None, o, p), (h, cam, 16, None, dn(strength=0.0), None, o, p),
             (h, cam, 16, None, None, fs(exposure=0.0), o, p), (h, cam, 16, None, None, fs(curve=4), o, p),
             (h, cam, 16, None, dn(), fs(gamma=INF), o, None),
             # (the stand-in's samples per pixel read as 0xA5A5A5A5: no pass count fits the sample index)
             (h, cam, 16, None, None, None, o, p), (h, cam, 5, rs(), dn(), fs(), None, p)]
    for s, c, passes, r, d, f, rgb, rgba in calls:
        st = lib.rtc_render_robust(s, C.byref(c) if c is not None else None, DEPTH, passes, C.byref(r) if r is not None else None,
                                   C.byref(d) if d is not None else None, C.byref(f) if f is not None else None, rgb, rgba, None, None, None)
        assert _status(lib, st) == "InvalidArgument", (passes, lib.rtc_last_error())
    assert bytes(handle) == b"\xa5" * SENTINEL and not out.any() and not px.any()


def test_progressive_without_buckets_says_so(rtc):
    """robust() of an object built without robust= raises before anything is touched (no device here: the object is bare)"""
    prog = object.__new__(rtc.Progressive)
    prog.buckets = None
    with pytest.raises(ValueError):
        prog.robust()
    with pytest.raises(ValueError):
        prog.denoised(robust={})
    with pytest.raises(ValueError):
        prog.filmed(robust={})
    for bad in (4, 1, 17, 0):
        with pytest.raises(ValueError):
            rtc.Progressive(None, None, robust=bad)
    import inspect
    assert list(inspect.signature(rtc.Progressive.__init__).parameters)[:5] == ["self", "gpu_scene", "cam", "max_depth", "noise"]
    assert "robust" not in inspect.signature(rtc.AdaptiveProgressive.__init__).parameters


# ---- the loader
def _scene(sampling=None):
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}], "objects": [{"type": {"sphere": {}}}]}
    if sampling is not None:
        s["camera"]["sampling"] = sampling
    return json.dumps(s)


D = rb.DEFAULTS


@pytest.mark.parametrize("sampling, want", [
    (None, None), ({}, None), ({"passes": 16}, None), ({"passes": 16, "robust": False}, None), ({"robust": False}, None),
    ({"passes": 16, "robust": True}, D), ({"passes": 5, "robust": True}, D), ({"passes": 16, "robust": {}}, D),
    ({"passes": 16, "robust": 3}, dict(D, buckets=3)), ({"passes": 16, "robust": 15}, dict(D, buckets=15)),
    ({"passes": 7, "robust": 7}, dict(D, buckets=7)),
    ({"passes": 16, "robust": {"buckets": 9}}, dict(D, buckets=9)), ({"passes": 16, "robust": {"gain": 0}}, dict(D, gain=0.0)),
    ({"passes": 16, "robust": {"buckets": 11, "gain": 2.5}}, {"buckets": 11, "gain": 2.5}),
    ({"passes": 16, "robust": True, "denoise": True}, D),
])
def test_loader_reads_the_key(rtc, sampling, want):
    r = rtc.HostScene(_scene(sampling)).robust()
    assert (r.to_dict() if r is not None else None) == want


@pytest.mark.parametrize("sampling, error", [
    ({"passes": 16, "robust": {"buckets": 5, "bins": 3}}, "UnknownField"), ({"passes": 16, "robust": {"strength": 1}}, "UnknownField"),
    ({"passes": 16, "robust": 4}, "InvalidData"), ({"passes": 16, "robust": 1}, "InvalidData"), ({"passes": 32, "robust": 17}, "InvalidData"),
    ({"passes": 16, "robust": 0}, "InvalidData"), ({"passes": 16, "robust": 5.5}, "InvalidData"), ({"passes": 16, "robust": -3}, "InvalidData"),
    ({"passes": 16, "robust": "on"}, "InvalidData"), ({"passes": 16, "robust": None}, "InvalidData"), ({"passes": 16, "robust": [5]}, "InvalidData"),
    ({"passes": 16, "robust": {"buckets": 6}}, "InvalidData"), ({"passes": 16, "robust": {"buckets": "5"}}, "InvalidData"),
    ({"passes": 16, "robust": {"buckets": True}}, "InvalidData"),
    ({"passes": 16, "robust": {"gain": -1}}, "InvalidData"), ({"passes": 16, "robust": {"gain": "1"}}, "InvalidData"),
    ({"passes": 16, "robust": {"gain": True}}, "InvalidData"),
    # beside "passes" below M (none is 1)
    ({"robust": True}, "InvalidData"), ({"passes": 4, "robust": True}, "InvalidData"), ({"passes": 6, "robust": 7}, "InvalidData"),
    ({"passes": 8, "robust": {"buckets": 9}}, "InvalidData"),
    # robust beside adaptive
    ({"passes": 16, "robust": True, "adaptive": {"threshold": 0.01}}, "InvalidData"),
    ({"passes": 16, "robust": 3, "adaptive": {"threshold": 0.01}, "denoise": True}, "InvalidData"),
])
def test_loader_refuses(rtc, sampling, error):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(sampling))
    assert e.value.name == error, e.value.args


def test_robust_false_beside_adaptive_is_no_key(rtc):
    hs = rtc.HostScene(_scene({"passes": 16, "robust": False, "adaptive": {"threshold": 0.01}}))
    assert hs.robust() is None and hs.adaptive() is not None


def test_the_key_changes_no_table(rtc):
    """A file without the key, with it false and with it set flatten to the same tables and the same digest."""
    plain = rtc.HostScene(_scene({"passes": 16}))
    base = rtc.build_tables_digest(plain.desc)[0]
    assert base == rtc.build_tables_digest(rtc.HostScene(_scene()).desc)[0]
    counts = [getattr(plain.desc, f) for f, t in rtc.SceneDesc._fields_ if t is C.c_uint32]
    for robust in (False, True, 7, {"buckets": 3, "gain": 4}):
        hs = rtc.HostScene(_scene({"passes": 16, "robust": robust}))
        assert hs.passes() == 16
        assert rtc.build_tables_digest(hs.desc)[0] == base
        assert [getattr(hs.desc, f) for f, t in rtc.SceneDesc._fields_ if t is C.c_uint32] == counts
    # the fixture without its key is the fixture; the room it was made from has none
    lamp = rtc.HostScene.from_file(rb.ROBUST_LAMP)
    scene = json.loads(open(rb.ROBUST_LAMP).read())
    del scene["camera"]["sampling"]["robust"]
    bare = rtc.HostScene(json.dumps(scene))
    assert rtc.build_tables_digest(bare.desc)[0] == rtc.build_tables_digest(lamp.desc)[0]
    assert bare.robust() is None and mb.mix(rtc).robust() is None
    assert lamp.robust().to_dict() == D and lamp.passes() == 16 and lamp.denoise() is None and lamp.film() is None


# ---- the checker: known answers on one grey pixel, one pass a bucket
def _grey(values, gain=1.0, passes=None):
    sums = np.repeat(np.asarray(values, dtype=np.float64)[:, None, None], 3, axis=2)   # [M][1][3]
    r = rb.robust(sums, passes if passes is not None else len(values), gain)
    return {k: v.reshape(-1)[0] if k != "mean" else v.reshape(3) for k, v in r.items()}


def test_one_spike_among_equals_is_dropped_and_ties_go_by_index():
    r = _grey((0.5, 0.5, 0.5, 0.5, 13.8))
    assert abs(r["gini"] - 0.6734177215189873) <= 1e-15
    assert r["rejected"] == 2 and (r["mean"] == 0.5).all() and r["variance"] == 0.0     # (c = 1: buckets 1, 2, 3 are kept)
    # ties go by index, seen through the clamp of the keys: negative luminances all have the key 0, and the mean keeps the values
    r = _grey((-1.0, -2.0, -3.0, -4.0, 13.8))
    assert abs(r["gini"] - 0.8) <= 1e-15 and r["rejected"] == 4 and (r["mean"] == -3.0).all()      # (the median is bucket 2)
    r = _grey((-1.0, -2.0, -3.0, -4.0, 13.8), gain=0.7)
    assert r["rejected"] == 2 and (r["mean"] == -3.0).all()                                        # (buckets 1, 2, 3)
    r = _grey((-4.0, -1.0, -2.0, -3.0, 13.8))
    assert r["rejected"] == 4 and (r["mean"] == -2.0).all()


def test_a_ramp():
    r = _grey((1, 2, 3, 4, 5))
    assert abs(r["gini"] - 4.0 / 15.0) <= 1e-15
    assert r["rejected"] == 2 and (r["mean"] == 3.0).all() and abs(r["variance"] - 1.0 / 3.0) <= 1e-15
    # in any order of the buckets
    r = _grey((4, 1, 5, 3, 2))
    assert r["rejected"] == 2 and (r["mean"] == 3.0).all() and abs(r["variance"] - 1.0 / 3.0) <= 1e-15


def test_equal_buckets_keep_everything():
    r = _grey((0.5,) * 5)
    assert r["rejected"] == 0 and (r["mean"] == 0.5).all() and r["variance"] == 0.0 and abs(r["gini"]) <= 1e-15
    r = _grey((0.0,) * 5)
    assert r["gini"] == 0.0 and r["rejected"] == 0 and (r["mean"] == 0.0).all() and r["variance"] == 0.0


def test_non_finite_buckets():
    r = _grey((0.5, NAN, 0.25, INF, 0.75))
    assert r["gini"] == 1.0 and r["rejected"] == 4 and (r["mean"] == 0.75).all()        # (T is infinite: the plain median of the keys)
    assert np.isfinite(_grey((0.5, NAN, 0.25, INF, 0.75), gain=4.0)["mean"]).all()
    assert not np.isfinite(_grey((0.5, NAN, 0.25, INF, 0.75), gain=0.0)["mean"]).all()   # (gain 0 keeps every bucket)
    r = _grey((NAN, 0.5, NAN, NAN, 0.25))
    assert not np.isfinite(r["mean"]).any()
    # negative luminance counts as 0 for the rank, but the mean keeps the values
    r = _grey((-1.0, -2.0, -3.0), gain=0.0)
    assert r["rejected"] == 0 and (r["mean"] == -2.0).all()


def test_bucket_frame_counts():
    """P = 7, M = 3: buckets hold 3, 2, 2 frames"""
    r = _grey((3.0, 2.0, 2.0), passes=7)
    assert (r["mean"] == 1.0).all() and r["rejected"] == 0


def test_the_checker_refuses_what_the_contract_refuses():
    sums = np.zeros((5, 4, 3))
    for bad in (dict(passes=4), dict(gain=-1.0), dict(gain=NAN), dict(gain=INF)):
        with pytest.raises(ValueError):
            rb.robust(sums, **dict(dict(passes=5), **bad))
    for m in (1, 2, 4, 16, 17):
        with pytest.raises(ValueError):
            rb.robust(np.zeros((m, 4, 3)), 32)


# ---- the checker: a synthetic image
TRUTH, SIGMA, SPIKE = 0.5, 0.2, 40.0


def _synthetic(passes, spikes):
    rng = np.random.default_rng(20211)
    frames = TRUTH + SIGMA * rng.standard_normal((passes, 32, 32, 3))
    hit = np.zeros((32, 32), dtype=bool)
    if spikes:
        where = rng.permutation(32 * 32)[:32 * 32 // 20]
        hit.reshape(-1)[where] = True
        at = rng.integers(0, passes, where.size)
        for w, p in zip(where, at):
            frames[p].reshape(-1, 3)[w] += SPIKE
    return frames, hit


@pytest.mark.parametrize("passes, buckets", [(8, 5), (16, 5)])
def test_spikes_leave_the_robust_mean(passes, buckets):
    frames, hit = _synthetic(passes, True)
    plain = frames.mean(axis=0)
    r = rb.robust(rb.bucket_sums(frames, buckets), passes)
    ratio = rb.rmse(plain, TRUTH) / rb.rmse(r["mean"], TRUTH)
    print(f"P {passes}, M {buckets}: RMSE plain {rb.rmse(plain, TRUTH):.4f}, robust {rb.rmse(r['mean'], TRUTH):.4f}, ratio {ratio:.2f}")
    assert ratio >= 5.0
    assert hit.sum() == 51 and r["mean"][hit].max() <= 2.0
    assert (r["rejected"][hit] >= 2).all()


@pytest.mark.parametrize("buckets", [3, 5, 7])
def test_the_price_on_clean_pixels(buckets):
    frames, _ = _synthetic(16, False)
    plain = frames.mean(axis=0)
    r = rb.robust(rb.bucket_sums(frames, buckets), 16)
    ratio = rb.rmse(r["mean"], TRUTH) / rb.rmse(plain, TRUTH)
    print(f"M {buckets}: RMSE robust / plain {ratio:.3f}")
    assert ratio <= 1.10


def test_the_denoisers_view():
    frames, _ = _synthetic(16, False)
    r = rb.robust(rb.bucket_sums(frames, 5), 16)
    predicted, measured = float(np.sqrt(r["variance"].mean())), rb.rmse(r["mean"], TRUTH)
    print(f"sqrt(mean v) {predicted:.4f}, RMSE {measured:.4f}")
    assert abs(predicted - measured) <= 0.10 * measured
    # the denoiser's own variance from (mean_out, sumsq_out, P), formed as rtc.h's v(x, y)
    u, s, P = r["mean"], r["sumsq"], 16.0
    got = np.maximum(0.0, s - P * ((u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])) / (3.0 * ((P - 1.0) * P))
    pick = r["variance"] > 1e-6 * (u ** 2).sum(axis=-1)
    assert pick.mean() > 0.9
    assert (np.abs(got[pick] - r["variance"][pick]) <= 1e-9 * r["variance"][pick]).all()
    # radius 0 returns the mean to the bit whatever the sums of squares: the checker takes the pair as it is
    out = db.denoise(u, s, passes=16, radius=0)
    assert (out == u).all()


@pytest.mark.parametrize("passes, buckets", [(15, 15), (10, 5)])
def test_gain_0_is_the_plain_mean(passes, buckets):
    frames, _ = _synthetic(passes, True)
    plain = frames.mean(axis=0)
    r = rb.robust(rb.bucket_sums(frames, buckets), passes, gain=0.0)
    assert (r["rejected"] == 0).all()
    assert (np.abs(r["mean"] - plain) <= 1e-15 * np.abs(plain)).all()


def test_gain_0_with_unequal_buckets_is_not_the_plain_mean():
    frames, _ = _synthetic(8, False)
    r = rb.robust(rb.bucket_sums(frames, 5), 8, gain=0.0)
    assert (r["rejected"] == 0).all() and np.abs(r["mean"] - frames.mean(axis=0)).max() > 1e-6


def test_bucket_sums_are_in_order():
    frames, _ = _synthetic(8, False)
    sums = rb.bucket_sums(frames, 5)
    assert (sums[0] == frames[0] + frames[5]).all() and (sums[2] == frames[2] + frames[7]).all() and (sums[4] == frames[4]).all()


# ---- the fixtures, rendered by the emitter checker
@pytest.fixture(scope="module")
def lamp_frames(rtc):
    hs = rtc.HostScene.from_file(rb.ROBUST_LAMP)
    ck = mb.scene_of(rtc, hs)
    cam = hs.camera()
    assert (cam.hsize, cam.vsize, hs.passes()) == (80, 45, 16)
    frames = {p: ck.render(cam, DEPTH, hs.sampling(), hs.spots(), sample_pass=p)[0] for p in list(range(16)) + list(range(32, 160))}
    return hs, frames


def test_the_fixture_has_fireflies_and_the_robust_mean_fewer(lamp_frames):
    hs, frames = lamp_frames
    first = [frames[p] for p in range(16)]
    plain = np.mean(first, axis=0)
    setting = hs.robust()
    r = rb.robust(rb.bucket_sums(first, setting.buckets), 16, setting.gain)
    reference = np.mean([frames[p] for p in range(32, 160)], axis=0)
    a_plain, a_robust = rb.speck_share(plain), rb.speck_share(r["mean"])
    e_plain, e_robust = rb.rmse(plain, reference), rb.rmse(r["mean"], reference)
    print(f"speck share: plain {a_plain:.4f}, robust {a_robust:.4f}; RMSE against passes 32 .. 159: plain {e_plain:.4f}, "
          f"robust {e_robust:.4f}, ratio {e_plain / e_robust:.3f} (bound {LAMP_BOUND:.3f}); rejected on {float((r['rejected'] > 0).mean()):.4f}")
    assert a_plain > 0.0 and a_robust < a_plain
    assert e_plain / e_robust >= LAMP_BOUND > 1.0


def test_the_darkening_on_the_unspiked_room(rtc):
    hs = mb.mix(rtc)
    ck = mb.scene_of(rtc, hs)
    cam = hs.camera()
    frames = [ck.render(cam, DEPTH, hs.sampling(), hs.spots(), sample_pass=p)[0] for p in range(16)]
    plain = np.mean(frames, axis=0)
    r = rb.robust(rb.bucket_sums(frames, 5), 16)
    ratio = float(rb.luminance(r["mean"]).mean() / rb.luminance(plain).mean())
    print(f"mean luminance robust / plain {ratio:.4f}")
    assert abs(1.0 - ratio) <= MIX_LOSS + 0.02


# ---- documents and build
KERNELS = [f"rtc_robust_m{m}{form}_kernel" for m in (3, 5, 7, 9, 11, 13, 15) for form in ("", "_narrow")] + ["rtc_robust_naive_kernel"]


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 31." in design
    for word in ("rtc_robust_device", "rtc_render_robust", "rtc_robust_naive_kernel", "rtc_robust_m5_kernel", "rtc_robust_m15_narrow_kernel",
                 "robust_naive", "Buisine", "tests/cpp/robust_oracle.cpp", "profiles/robust/object_identity.txt",
                 "profiles/robust/times_1080p.txt", "robust_lamp.json", "Out of scope", "librtc_multi", "Infinity Cache",
                 "AdaptiveProgressive", "Per-channel", "Multiple importance sampling"):
        assert word in design, word
    for doc, word in (("README.md", "rtc_robust_device"), ("README.md", "\"robust\""), ("INTEGRATION.md", "rtc_robust_device"),
                      ("INTEGRATION.md", "RtcRobustSetting"), (os.path.join("tools", "README.md"), "--robust"),
                      (os.path.join("profiles", "HISTORY.md"), "robust accumulation")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resource rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in KERNELS:
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} |" in design, name
            assert k["vgprs_spilled"] == 0 and k["scratch_bytes_per_lane"] == 0


def test_object_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "robust", "object_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_kernels_ext.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o",
                "rtc_occlusion.o", "rtc_shadowfilter.o", "rtc_media.o", "rtc_environment.o", "rtc_skylight.o", "rtc_indirect.o",
                "rtc_emitters.o", "rtc_accum.o", "rtc_adaptive.o", "rtc_denoise.o", "rtc_film.o"):
        assert obj in text and "identical" in text
    assert "rtc_capi.o" in text and "kernel_resources.json" in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_robust.o", "rtc_robust.remarks", "librobust_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_robust.hip")).read()
    assert "rtc_kernels.hip" not in unit and "rtc_device.h" not in unit      # (a unit of its own: no render kernel compiles in it)
    assert [line for line in unit.splitlines() if line.startswith("#include \"")] == ["#include \"../../include/rtc.h\""]
    oracle = open(os.path.join(REPO, "tests", "cpp", "robust_oracle.cpp")).read()
    assert "#include \"" not in oracle                                        # (the checker includes nothing of the product)
