"""Adaptive sampling without a GPU: the ABI of rtc_scene_adaptive_* and rtc_render_adaptive and their validation, the
loader's "adaptive", and the checker (tests/cpp/adaptive_oracle.cpp) against the progressive image, the stopping rule and
an independent restatement of the tile noise."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import adaptive_binding as ab
import camera_binding as cb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOFT_SHADOWS = os.path.join(REPO, "tests", "golden", "area_scenes", "soft_shadows.json")
SENTINEL = 1 << 16
NEW = ["rtc_scene_adaptive_begin_device", "rtc_scene_adaptive_accumulate_device", "rtc_scene_adaptive_step", "rtc_render_adaptive"]


def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (its samples per pixel read as 0xA5A5A5A5)."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


# ---- the symbols
def test_symbols_are_exported(rtc):
    assert set(NEW) <= set(rtc.RTC_SYMBOLS)
    assert "rtch_scene_adaptive" in rtc.HOST_SYMBOLS
    for n in NEW:
        assert getattr(rtc.hip_lib(), n) is not None
    assert rtc.host_lib().rtch_scene_adaptive is not None
    assert C.sizeof(rtc.Adaptive) == 24 and rtc.Adaptive.threshold.offset == 16
    # nine pointers and the host's round (+ 4 bytes of padding)
    assert C.sizeof(rtc.AdaptiveState) == 80 and rtc.AdaptiveState.round.offset == 72
    assert "#define RTC_ADAPTIVE_MAX_TILE 1024u" in open(os.path.join(REPO, "include", "rtc.h")).read()


# ---- every invalid argument is refused before anything is touched
FAKE = 0x7F0000001000   # (never dereferenced: validation comes first)
GOOD = dict(tile_w=16, tile_h=16, min_passes=4, max_passes=8, threshold=0.01)
BAD_SETTING = [
    (dict(tile_w=0), "tile"), (dict(tile_h=0), "tile"), (dict(tile_w=1025), "tile"), (dict(tile_h=4096), "tile"),
    (dict(min_passes=0), "min_passes"), (dict(min_passes=1), "min_passes"), (dict(max_passes=3), "max_passes"),
    (dict(min_passes=9), "max_passes"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=-1e-9), "threshold"),
    (dict(threshold=float("inf")), "threshold"), (dict(threshold=-0.0 - 1.0), "threshold"),
]


def _setting(rtc, **kw):
    v = dict(GOOD)
    v.update(kw)
    return rtc.Adaptive(v["tile_w"], v["tile_h"], v["min_passes"], v["max_passes"], v["threshold"])


def _state(rtc, **kw):
    names = [f for f, _ in rtc.AdaptiveState._fields_ if f != "round"]
    v = {f: FAKE + 0x1000 * i for i, f in enumerate(names)}
    v.update(kw)
    return rtc.AdaptiveState(*[v[f] for f in names], 77)


def _cam(rtc, w=64, h=48):
    return rtc.make_camera(w, h, 1.0, (0, 1.5, -5), (0, 1, 0), (0, 1, 0))


def _calls(rtc, handle, setting, state, cam, with_render=True):
    """Every entry point with these arguments: (name, status, error message)."""
    lib = rtc.hip_lib()
    n = C.c_uint32(12345)
    rgb = np.full((cam.vsize, cam.hsize, 3), 7.0)
    calls = [("begin", lambda: lib.rtc_scene_adaptive_begin_device(handle, cam.hsize, cam.vsize, setting, state, None)),
             ("accumulate", lambda: lib.rtc_scene_adaptive_accumulate_device(handle, cam.hsize, cam.vsize, setting, state, FAKE,
                                                                             FAKE + 8, 1, None)),
             ("step", lambda: lib.rtc_scene_adaptive_step(handle, C.byref(cam), 5, setting, state, C.byref(n), None))]
    if with_render:
        calls.append(("render", lambda: lib.rtc_render_adaptive(handle, C.byref(cam), 5, setting, rgb.ctypes.data, None)))
    out = []
    for name, call in calls:
        st = call()
        out.append((name, st, lib.rtc_last_error().decode()))
    assert n.value == 12345 and np.all(rgb == 7.0)
    return out


@pytest.mark.parametrize("bad, word", BAD_SETTING, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b, _ in BAD_SETTING])
def test_each_invalid_setting_is_refused(rtc, bad, word):
    lib = rtc.hip_lib()
    handle = _stand_in()
    state = _state(rtc)
    for name, st, msg in _calls(rtc, C.cast(handle, C.c_void_p), C.byref(_setting(rtc, **bad)), C.byref(state), _cam(rtc)):
        assert _status(lib, st) == "InvalidArgument", name
        assert "adaptive" in msg and word in msg, (name, msg)
    assert bytes(handle) == b"\xa5" * SENTINEL
    assert state.round == 77


def test_the_index_limit_is_refused(rtc):
    """A valid setting on the stand-in, whose samples per pixel read as 0xA5A5A5A5: max_passes * S breaks the limit.
    (The edge on a real handle is tested in test_adaptive_gpu.py.)"""
    lib = rtc.hip_lib()
    handle = _stand_in()
    state = _state(rtc)
    for name, st, msg in _calls(rtc, C.cast(handle, C.c_void_p), C.byref(_setting(rtc)), C.byref(state), _cam(rtc)):
        assert _status(lib, st) == "InvalidArgument", name
        assert "sample indices" in msg, name
    assert bytes(handle) == b"\xa5" * SENTINEL and state.round == 77


@pytest.mark.parametrize("field", ["sum", "sumsq", "tile_passes", "tile_noise", "active", "n_active"])
def test_each_null_state_buffer_is_refused(rtc, field):
    lib = rtc.hip_lib()
    handle = _stand_in()
    state = _state(rtc, **{field: None})
    for name, st, msg in _calls(rtc, C.cast(handle, C.c_void_p), C.byref(_setting(rtc)), C.byref(state), _cam(rtc), False):
        assert _status(lib, st) == "InvalidArgument", name
        assert "null state" in msg, name
    assert bytes(handle) == b"\xa5" * SENTINEL and state.round == 77


def test_null_handle_setting_state_and_outputs(rtc):
    lib = rtc.hip_lib()
    cam = _cam(rtc)
    handle = _stand_in()
    h = C.cast(handle, C.c_void_p)
    for name, st, msg in _calls(rtc, None, C.byref(_setting(rtc)), C.byref(_state(rtc)), cam):
        assert _status(lib, st) == "InvalidArgument" and "null" in msg, name
    for name, st, msg in _calls(rtc, h, None, C.byref(_state(rtc)), cam):
        assert _status(lib, st) == "InvalidArgument" and "null setting" in msg, name
    for name, st, msg in _calls(rtc, h, C.byref(_setting(rtc)), None, cam, False):
        assert _status(lib, st) == "InvalidArgument" and "null state" in msg, name
    n = C.c_uint32()
    s, a = C.byref(_setting(rtc)), C.byref(_state(rtc))
    assert _status(lib, lib.rtc_scene_adaptive_step(h, C.byref(cam), 5, s, a, None, None)) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_adaptive_step(h, None, 5, s, a, C.byref(n), None)) == "InvalidArgument"
    assert _status(lib, lib.rtc_render_adaptive(h, C.byref(cam), 5, s, None, None)) == "InvalidArgument"
    assert _status(lib, lib.rtc_render_adaptive(h, None, 5, s, FAKE, None)) == "InvalidArgument"
    assert bytes(handle) == b"\xa5" * SENTINEL


@pytest.mark.parametrize("frame, tiles, n", [(None, FAKE, 1), (FAKE, None, 1), (FAKE, FAKE, 0), (FAKE, FAKE, 13)])
def test_accumulate_refuses_its_frame_and_list(rtc, frame, tiles, n):
    """64 x 48 in 16 x 16 tiles: 12 of them."""
    lib = rtc.hip_lib()
    handle = _stand_in()
    st = lib.rtc_scene_adaptive_accumulate_device(C.cast(handle, C.c_void_p), 64, 48, C.byref(_setting(rtc)), C.byref(_state(rtc)),
                                                  frame, tiles, n, None)
    assert _status(lib, st) == "InvalidArgument"
    msg = lib.rtc_last_error().decode()
    assert ("null frame" in msg) if n == 1 else ("listed tiles of 12" in msg), msg
    assert bytes(handle) == b"\xa5" * SENTINEL


@pytest.mark.parametrize("w, h", [(0, 48), (64, 0)])
def test_an_empty_image_is_refused(rtc, w, h):
    lib = rtc.hip_lib()
    handle = _stand_in()
    st = lib.rtc_scene_adaptive_begin_device(C.cast(handle, C.c_void_p), w, h, C.byref(_setting(rtc)), C.byref(_state(rtc)), None)
    assert _status(lib, st) == "InvalidArgument" and "image" in lib.rtc_last_error().decode()


# ---- the loader
def _scene(sampling=None):
    cam = {"width": 40, "height": 20, "field-of-view": 1.0, "from": [0, 1.5, -5], "to": [0, 1, 0], "up": [0, 1, 0]}
    if sampling is not None:
        cam["sampling"] = sampling
    return json.dumps({"camera": cam, "lights": [{"point-light": {"position": [-10, 10, -10], "intensity": [1, 1, 1]}}],
                       "objects": [{"type": {"sphere": {}}}]})


def test_loader_without_adaptive(rtc):
    for sampling in (None, {}, {"grid": 2, "passes": 8}):
        assert rtc.HostScene(_scene(sampling)).adaptive() is None


def test_loader_reads_adaptive_and_its_defaults(rtc):
    a = rtc.HostScene(_scene({"passes": 32, "adaptive": {"threshold": 0.002}})).adaptive()
    assert a.to_dict() == {"tile_w": 16, "tile_h": 16, "min_passes": 4, "max_passes": 32, "threshold": 0.002}
    a = rtc.HostScene(_scene({"grid": 2, "passes": 9, "adaptive": {"threshold": 0, "min-passes": 2, "tile": [8, 4]}})).adaptive()
    assert a.to_dict() == {"tile_w": 8, "tile_h": 4, "min_passes": 2, "max_passes": 9, "threshold": 0.0}
    a = rtc.HostScene(_scene({"passes": 4, "adaptive": {"threshold": 1.5, "min-passes": 4, "tile": 1024}})).adaptive()
    assert (a.tile_w, a.tile_h, a.min_passes, a.max_passes) == (1024, 1024, 4, 4)
    hs = rtc.HostScene(_scene({"adaptive": {"threshold": 0.1, "tile": 8}, "passes": 6}))   # (key order does not matter)
    assert hs.adaptive().max_passes == 6 and hs.passes() == 6


@pytest.mark.parametrize("adaptive, passes, error, word", [
    ({}, 8, "MissingField", "threshold"),
    ({"threshold": 0.1, "tiles": 8}, 8, "UnknownField", "tiles"),
    ({"threshold": 0.1, "min_passes": 3}, 8, "UnknownField", "min_passes"),
    ({"threshold": -0.1}, 8, "InvalidData", "threshold"),
    ({"threshold": "0.1"}, 8, "UnexpectedToken", "threshold"),
    ({"threshold": 0.1, "min-passes": 1}, 8, "InvalidData", "min-passes"),
    ({"threshold": 0.1, "min-passes": 9}, 8, "InvalidData", "min-passes"),
    ({"threshold": 0.1, "min-passes": 2.5}, 8, "InvalidNumber", "min-passes"),
    ({"threshold": 0.1}, None, "InvalidData", "passes"),        # passes 1 < the default min-passes 4
    ({"threshold": 0.1}, 3, "InvalidData", "passes"),
    ({"threshold": 0.1, "tile": 0}, 8, "InvalidData", "tile"),
    ({"threshold": 0.1, "tile": 1025}, 8, "InvalidData", "tile"),
    ({"threshold": 0.1, "tile": [8]}, 8, "LengthMismatch", "tile"),
    ({"threshold": 0.1, "tile": [8, 0]}, 8, "InvalidData", "tile"),
    ({"threshold": 0.1, "tile": "8"}, 8, "UnexpectedToken", "tile"),
    ([], 8, "UnexpectedToken", "adaptive"),
])
def test_loader_refuses(rtc, adaptive, passes, error, word):
    sampling = {"adaptive": adaptive}
    if passes is not None:
        sampling["passes"] = passes
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(sampling))
    assert e.value.name == error
    assert word in str(e.value)


# ---- the checker
def _frames(shape, n, seed=1, scale=1.0):
    rng = np.random.default_rng(seed)
    return [rng.random(shape + (3,)) * scale for _ in range(n)]


def _progressive(frames, p):
    """The progressive image after p passes: the frames summed in pass order, divided once."""
    s = frames[0].copy()
    for f in frames[1:p]:
        s = s + f
    return s / p


def _noise(frames, p, mask):
    """Section 13's noise of the pixels under `mask` after p passes, summed by numpy (another order)."""
    s, q = frames[0].copy(), (frames[0] ** 2).sum(axis=2)
    for f in frames[1:p]:
        s = s + f
        q = q + ((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2])
    m = s / p
    d = np.maximum(0.0, q - p * (m ** 2).sum(axis=2))
    return math.sqrt(d[mask].sum() / mask.sum() / (3 * (p - 1) * p))


def test_a_threshold_nothing_reaches_is_the_progressive_image(rtc):
    h, w = 21, 37
    frames = _frames((h, w), 6)
    st = ab.run(lambda R: frames[R], w, h, rtc.Adaptive(8, 8, 2, 6, 0.0))
    assert np.all(st.tile_passes == 6) and st.rounds == 6 and st.tile_passes_run == 6 * len(st.tile_passes)
    assert np.array_equal(st.mean, _progressive(frames, 6))
    s = frames[0].copy()
    for f in frames[1:]:
        s = s + f
    assert np.array_equal(st.sum, s)


def test_the_progressive_checker_image_at_max_passes(rtc):
    """The same on a rendered scene: soft shadows through the sample-pass checker."""
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    cam = hs.camera(40, 18)
    chk = ab.PassScene(hs.desc, hs.lights)
    smp = cb.sampling(1, True, seed=3)
    frames = [chk.render(cam, 5, smp, P, light_seed=9) for P in range(4)]
    st = ab.run(lambda R: chk.render(cam, 5, smp, R, light_seed=9), cam.hsize, cam.vsize, rtc.Adaptive(16, 16, 2, 4, 0.0))
    assert np.all(st.tile_passes == 4)
    assert np.array_equal(st.mean, _progressive(frames, 4))


def test_a_zero_variance_tile_stops_at_min_passes(rtc):
    h, w = 16, 24
    frames = _frames((h, w), 10, seed=4)
    for f in frames:
        f[:8, :8] = (0.25, 0.5, 0.75)        # tile 0 of 8 x 8 tiles: the same colour every pass
        f[8:, 16:] = 0.0                     # tile 5: black
    st = ab.run(lambda R: frames[R], w, h, rtc.Adaptive(8, 8, 3, 10, 1e-6))
    assert st.tile_passes[0] == 3 and st.tile_passes[5] == 3
    assert st.tile_noise[0] == 0.0 and st.tile_noise[5] == 0.0
    assert np.all(st.tile_passes[[1, 2, 3, 4]] == 10)
    assert np.array_equal(st.mean[:8, :8], _progressive(frames, 3)[:8, :8])


def test_each_tile_is_the_progressive_image_after_its_passes(rtc):
    """The central property: tile t of a run is the progressive image after P_t passes; passes within [min, max];
    a tile that stopped has noise <= threshold or max passes; one that ran to the end had noise above it before."""
    h, w = 45, 61                                   # tiles 16 x 16 -> 4 x 3, edge tiles 13 wide and 13 high
    rng = np.random.default_rng(7)
    amp = np.zeros((h, w, 1))                       # tile t's noise amplitude grows with t: some stop early, some never
    for t in range(12):
        x0, y0, tw, th = ab.tile_rect(t, w, h, 16, 16)
        amp[y0:y0 + th, x0:x0 + tw] = 0.12 * t / 11
    base = rng.random((h, w, 3))
    frames = [base + amp * rng.standard_normal((h, w, 3)) for _ in range(24)]
    a = rtc.Adaptive(16, 16, 4, 24, 0.02)
    st = ab.run(lambda R: frames[R], w, h, a)
    P = st.tile_passes
    assert P.min() >= 4 and P.max() <= 24 and len(set(P.tolist())) >= 3, P
    for t in range(len(P)):
        x0, y0, tw, th = ab.tile_rect(t, w, h, 16, 16)
        want = _progressive(frames, int(P[t]))[y0:y0 + th, x0:x0 + tw]
        assert np.array_equal(st.mean[y0:y0 + th, x0:x0 + tw], want), t
        mask = np.zeros((h, w), dtype=bool)
        mask[y0:y0 + th, x0:x0 + tw] = True
        assert st.tile_noise[t] == pytest.approx(_noise(frames, int(P[t]), mask), rel=1e-12)
        assert st.tile_noise[t] <= a.threshold or P[t] == 24
        if P[t] > 4:
            assert _noise(frames, int(P[t]) - 1, mask) > a.threshold
    assert st.max_noise == st.tile_noise.max()
    assert st.tile_passes_run == P.sum() and st.rounds == P.max()


def test_passes_are_monotone_round_by_round(rtc):
    h, w = 33, 50
    rng = np.random.default_rng(11)
    frames = [rng.random((h, w, 3)) * rng.random((h, w, 1)) for _ in range(12)]
    st = ab.State(w, h, rtc.Adaptive(8, 8, 2, 12, 0.05))
    before = st.tile_passes.copy()
    active_sizes = []
    while True:
        n = st.step(lambda R: frames[R])
        assert np.all(st.tile_passes >= before) and np.all(st.tile_passes - before <= 1) and st.tile_passes.max() <= 12
        active = st.active
        assert np.all(np.diff(active.astype(np.int64)) > 0)                 # ascending
        assert np.all(st.tile_passes[active] == st.rounds)                   # the active tiles took every round
        before = st.tile_passes.copy()
        active_sizes.append(n)
        if n == 0:
            break
    assert active_sizes == sorted(active_sizes, reverse=True)                # a tile that stopped stays stopped


def test_the_noise_order_is_the_kernel_s(rtc):
    """The lanes' order matters to the bits: items l, l + B, ... per lane, a butterfly, then the waves.  A 32 x 32 tile
    has 512 items on B = 512 lanes; a 1024 x 3 tile 1536 items on 1024 lanes, two a lane for half of them."""
    assert [ab.lib().adapt_block(*s) for s in [(1, 1), (8, 8), (16, 16), (15, 16), (32, 32), (1024, 3), (1024, 1024)]] == \
        [64, 64, 128, 128, 512, 1024, 1024]
    for tw, th in [(32, 32), (1024, 3), (7, 5)]:
        h, w = th, tw
        frames = _frames((h, w), 2, seed=tw, scale=3.0)
        st = ab.State(w, h, rtc.Adaptive(tw, th, 2, 2, 0.0))
        for f in frames:
            st.accumulate(st.compact(f, [0]), [0])
        half, items = (tw + 1) // 2, th * ((tw + 1) // 2)
        B = ab.lib().adapt_block(tw, th)
        m = st.sum / 2
        d = np.maximum(0.0, st.sumsq - 2 * ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]))
        lanes = [0.0] * B
        for it in range(items):
            r, x = it // half, 2 * (it % half)
            lanes[it % B] += d[r, x] + (d[r, x + 1] if x + 1 < w else 0.0)
        waves = []
        for wv in range(B // 64):
            v = lanes[64 * wv:64 * wv + 64]
            for off in (32, 16, 8, 4, 2, 1):
                v = [v[l] + v[l ^ off] for l in range(64)]
            waves.append(v[0])
        total = waves[0]
        for x in waves[1:]:
            total += x
        assert st.tile_noise[0] == math.sqrt(total / (w * h) / (3.0 * 1.0 * 2.0))
