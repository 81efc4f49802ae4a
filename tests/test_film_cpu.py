"""The film stage without a GPU: the symbols, the structs and the constants, every refusal of
rtc_film_device, rtc_film_scratch_bytes and rtc_render_filmed made with stand-in pointers, the loader's "film" key and
rtch_scene_film, and the checker (tests/cpp/film_oracle.cpp): known answers of the curves and the transfer functions, the
bloom of one pixel, the automatic exposure, and the fixture film_lamp.json rendered by the emitter checker - the share of its
8-bit channels at 255 with the film stage and with the plain clamp.

Measured with the checkers on the fixture at 80 x 45, 8 passes: 0.6814 of the channels of the plain clamp are at 255, 0.0156
of the film's."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import emitters_binding as mb
import film_binding as fb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
FAKE = 0x7F0000001000   # (never dereferenced: validation comes first)
NEW = ["rtc_film_scratch_bytes", "rtc_film_device", "rtc_render_filmed"]
DEPTH = 5
NAN, INF = float("nan"), float("inf")


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


# ---- ABI
def test_symbols_structs_and_constants(rtc):
    assert set(NEW) <= set(rtc.RTC_SYMBOLS) and "rtch_scene_film" in rtc.HOST_SYMBOLS and "rtc_diag_film_tile" in rtc.RTC_DIAG_SYMBOLS
    for n in NEW + ["rtc_diag_film_tile"]:
        assert getattr(rtc.hip_lib(), n) is not None
    assert rtc.host_lib().rtch_scene_film is not None
    S, F = rtc.FilmSetting, rtc.Film
    assert C.sizeof(S) == 80
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    assert C.sizeof(F) == 128
    assert [getattr(F, n).offset for n, _ in F._fields_] == [0, 8, 12, 16, 96, 104, 112, 120]
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("#define RTC_FILM_MAX_RADIUS 32u", "#define RTC_FILM_EPS 1e-10", "#define RTC_FILM_CURVE_LINEAR 0",
                 "#define RTC_FILM_CURVE_REINHARD 1", "#define RTC_FILM_CURVE_ACES 2", "#define RTC_FILM_CURVE_HABLE 3",
                 "#define RTC_FILM_TRANSFER_LINEAR 0", "#define RTC_FILM_TRANSFER_SRGB 1", "#define RTC_FILM_TRANSFER_GAMMA 2",
                 "#define RTC_ABI_VERSION 3u", "typedef struct rtc_film_setting {", "typedef struct rtc_film {",
                 "size_t rtc_film_scratch_bytes(uint32_t hsize, uint32_t vsize, const rtc_film_setting *s);",
                 "int rtc_film_device(const rtc_film *f, void *hip_stream);"):
        assert line in header, line
    assert (rtc.FILM_MAX_RADIUS, rtc.FILM_EPS) == (32, 1e-10)
    assert rtc.FILM_CURVES == {"linear": fb.LINEAR, "reinhard": fb.REINHARD, "aces": fb.ACES, "hable": fb.HABLE}
    assert rtc.FILM_TRANSFERS == {"linear": fb.T_LINEAR, "srgb": fb.T_SRGB, "gamma": fb.T_GAMMA}
    assert rtc.FilmSetting.make().to_dict() == fb.DEFAULTS
    assert rtc.FilmSetting.make(bloom=True).to_dict() == dict(fb.DEFAULTS, **fb.BLOOM)
    assert "film_naive" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "rtch_scene_film" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    assert "rtc_film" not in open(os.path.join(REPO, "include", "rtc_multi.h")).read()   # (librtc_multi does not get it)
    rtc.set_option("film_naive", 1)
    rtc.set_option("film_naive", 0)
    row_w, col_w, col_h = rtc.film_tile()
    assert row_w >= 1 and col_w >= 1 and col_h >= 1
    zig = open(os.path.join(REPO, "integration", "gpu.zig")).read()
    for word in ("rtc_film_scratch_bytes", "rtc_film_device", "rtc_render_filmed", "RtcFilm", "RtcFilmSetting"):
        assert word in zig, word


def test_headers_are_still_strict_c99_and_the_binding_matches():
    import test_abi
    test_abi.test_headers_are_valid_c()
    test_abi.test_zig_binding_matches_the_header()


def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("Y(c) = (0.2126 * c.r + 0.7152 * c.g) + 0.0722 * c.b", "E = (exposure * auto_key) / exp(T / n)",
                 "log(RTC_FILM_EPS + max(0, Y(in(q))))", "x(p).c = E * in(p).c",
                 "w = max(0, y - bloom_threshold) / (y > RTC_FILM_EPS ? y : RTC_FILM_EPS);  b(p).c = x(p).c * w",
                 "raw[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma)) for i = 0 .. R",
                 "norm = raw[0], then norm = norm + 2.0 * raw[i] for i ascending;  g[i] = raw[i] / norm",
                 "c = x(p).c + bloom_intensity * B(p).c", "t = (c * (1.0 + c / (white * white))) / (1.0 + c)",
                 "t = (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14)",
                 "f(v) = ((v * (0.15 * v + 0.05) + 0.004) / (v * (0.15 * v + 0.5) + 0.06)) - 0.02 / 0.3",
                 "o = t <= 0.0031308 ? 12.92 * t : 1.055 * pow(t, 1.0 / 2.4) - 0.055", "o = t > 0 ? pow(t, 1.0 / gamma) : 0.0",
                 "returns `in` to the bit", "no library function is involved", "1e-12 * max(1, |value|)",
                 "there is no renormalisation", "librtc_multi renders"):
        assert line in header, line


# ---- rtc_film_device: every refusal, with stand-in pointers and no device
GOOD = dict(in_=FAKE, hsize=64, vsize=48, exposure=1.0, auto_key=0.18, bloom_radius=12, bloom_sigma=4.0, bloom_threshold=1.0,
            bloom_intensity=0.15, curve=fb.ACES, white=4.0, transfer=fb.T_SRGB, gamma=2.2, scratch=FAKE + 0x400000, out=FAKE + 0x200000,
            rgba=None, scale_out=None)
IN_BYTES = 64 * 48 * 24
BAD_SETTING = [
    (dict(exposure=0.0), "exposure"), (dict(exposure=-1.0), "exposure"), (dict(exposure=NAN), "exposure"), (dict(exposure=INF), "exposure"),
    (dict(auto_key=-0.18), "auto_key"), (dict(auto_key=NAN), "auto_key"), (dict(auto_key=INF), "auto_key"),
    (dict(bloom_radius=33), "bloom_radius"), (dict(bloom_radius=0xFFFFFFFF), "bloom_radius"),
    (dict(bloom_sigma=0.0), "bloom_sigma"), (dict(bloom_sigma=-4.0), "bloom_sigma"), (dict(bloom_sigma=NAN), "bloom_sigma"),
    (dict(bloom_sigma=INF), "bloom_sigma"),
    (dict(bloom_threshold=-1e-9), "bloom_threshold"), (dict(bloom_threshold=NAN), "bloom_threshold"), (dict(bloom_threshold=INF), "bloom_threshold"),
    (dict(bloom_intensity=-0.1), "bloom_intensity"), (dict(bloom_intensity=NAN), "bloom_intensity"), (dict(bloom_intensity=INF), "bloom_intensity"),
    (dict(curve=4), "curve"), (dict(curve=0xFFFFFFFF), "curve"),
    (dict(white=0.0), "white"), (dict(white=-4.0), "white"), (dict(white=NAN), "white"), (dict(white=INF), "white"),
    (dict(transfer=3), "transfer"),
    (dict(gamma=0.0), "gamma"), (dict(gamma=-2.2), "gamma"), (dict(gamma=NAN), "gamma"), (dict(gamma=INF), "gamma"),
]
BAD = [
    (dict(in_=None), "null"), (dict(out=None), "null"),
    (dict(scratch=None), "scratch"), (dict(scratch=None, bloom_radius=0), "scratch"), (dict(scratch=None, auto_key=0.0), "scratch"),
    (dict(hsize=0), "image"), (dict(vsize=0), "image"), (dict(hsize=1 << 21, vsize=(1 << 19) + 1), "image"),
    (dict(out=FAKE), "overlaps"), (dict(out=FAKE + IN_BYTES - 8), "overlaps"), (dict(out=FAKE - IN_BYTES + 8), "overlaps"),
] + BAD_SETTING


def _setting(rtc, v):
    return rtc.FilmSetting(v["exposure"], v["auto_key"], v["bloom_radius"], v["bloom_sigma"], v["bloom_threshold"], v["bloom_intensity"],
                           v["curve"], v["white"], v["transfer"], v["gamma"])


def _film(rtc, **kw):
    v = dict(GOOD)
    v.update(kw)
    return rtc.Film(v["in_"], v["hsize"], v["vsize"], _setting(rtc, v), v["scratch"], v["out"], v["rgba"], v["scale_out"])


def _ids(cases):
    return [",".join(f"{k}={v}" for k, v in b.items()) for b, _ in cases]


@pytest.mark.parametrize("bad, word", BAD, ids=_ids(BAD))
def test_each_invalid_argument_is_refused_before_the_device(rtc, bad, word):
    lib = rtc.hip_lib()
    f = _film(rtc, **bad)
    assert _status(lib, lib.rtc_film_device(C.byref(f), FAKE)) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert "film:" in text and word in text, text


def test_null_struct_and_null_stream_are_refused(rtc):
    lib = rtc.hip_lib()
    assert _status(lib, lib.rtc_film_device(None, FAKE)) == "InvalidArgument"
    assert _status(lib, lib.rtc_film_device(C.byref(_film(rtc)), None)) == "InvalidArgument"
    assert _status(lib, lib.rtc_diag_film_tile(None, None, None)) == "InvalidArgument"


def test_a_sigma_is_read_only_with_a_radius(rtc):
    """bloom_sigma is "finite, > 0 where radius > 0": with radius 0 any value passes the check (here: up to the scratch)"""
    assert rtc.film_scratch_bytes(64, 48, _setting(rtc, dict(GOOD, bloom_radius=0, bloom_sigma=NAN, auto_key=0.0))) == 0


@pytest.mark.parametrize("bad, word", BAD_SETTING, ids=_ids(BAD_SETTING))
def test_scratch_bytes_refuses_what_the_contract_refuses(rtc, bad, word):
    lib = rtc.hip_lib()
    assert lib.rtc_film_scratch_bytes(64, 48, C.byref(_setting(rtc, dict(GOOD, **bad)))) == 0
    text = lib.rtc_last_error().decode()
    assert "film:" in text and word in text, text
    with pytest.raises(rtc.RtcError):
        rtc.film_scratch_bytes(64, 48, _setting(rtc, dict(GOOD, **bad)))


def test_scratch_bytes(rtc):
    lib = rtc.hip_lib()
    for w, h in ((0, 48), (64, 0), (1 << 21, (1 << 19) + 1)):
        assert lib.rtc_film_scratch_bytes(w, h, C.byref(rtc.FilmSetting.make())) == 0 and b"film: image" in lib.rtc_last_error()
    assert lib.rtc_film_scratch_bytes(64, 48, None) == 0 and b"null" in lib.rtc_last_error()
    make = rtc.FilmSetting.make
    n = 64 * 48
    assert rtc.film_scratch_bytes(64, 48) == 0 and not lib.rtc_last_error()           # (the defaults: manual, no bloom)
    assert rtc.film_scratch_bytes(64, 48, make(bloom_radius=12, bloom_intensity=0.0)) == 0   # (intensity 0 is no bloom)
    assert rtc.film_scratch_bytes(64, 48, make(bloom_radius=0, bloom_intensity=0.2)) == 0    # (radius 0 is no bloom)
    bloom = rtc.film_scratch_bytes(64, 48, make(bloom=True))
    auto = rtc.film_scratch_bytes(64, 48, make(auto_key=0.18))
    assert bloom == 3 * n * 8                                                              # (H)
    assert 16 + 8 * ((n + 255) // 256) <= auto <= 16 + 8 * 2048 + 16                       # (E and a partial per block)
    assert rtc.film_scratch_bytes(64, 48, make(bloom=True, auto_key=0.18)) == bloom + auto
    assert rtc.film_scratch_bytes(1920, 1080, make(auto_key=0.18)) == rtc.film_scratch_bytes(4096, 4096, make(auto_key=0.18))  # (the grid is capped)


def test_render_filmed_refuses_on_the_host_and_touches_nothing(rtc):
    lib = rtc.hip_lib()
    handle = (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))
    h = C.cast(handle, C.c_void_p)
    cam = rtc.make_camera(64, 48, 1.0, (0, 1.5, -5), (0, 1, 0), (0, 1, 0))
    out = np.zeros((48, 64, 3))
    px = np.zeros((48, 64, 4), dtype=np.uint8)
    o, p = out.ctypes.data, px.ctypes.data
    ok, dn = rtc.FilmSetting.make(), rtc.DenoiseSetting.make()
    adaptive = rtc.Adaptive.make(0.01, 8)
    make = rtc.FilmSetting.make
    calls = [(None, cam, 8, None, None, ok, o, p), (h, cam, 8, None, None, ok, None, None), (h, None, 8, None, None, ok, o, p),
             (h, cam, 0, None, None, ok, o, p), (h, cam, 1, None, dn, ok, o, p), (h, cam, 0, None, dn, ok, o, None),
             (h, cam, 8, None, rtc.DenoiseSetting.make(radius=11), ok, o, p), (h, cam, 8, None, rtc.DenoiseSetting.make(strength=0.0), ok, o, p),
             (h, cam, 8, None, None, make(exposure=0.0), o, p), (h, cam, 8, None, None, make(auto_key=-1.0), o, p),
             (h, cam, 8, None, None, make(bloom_radius=33), o, p), (h, cam, 8, None, None, make(bloom_radius=3, bloom_sigma=0.0), o, p),
             (h, cam, 8, None, None, make(bloom_threshold=NAN), o, p), (h, cam, 8, None, None, make(bloom_intensity=-1.0), o, p),
             (h, cam, 8, None, None, make(curve=4), o, p), (h, cam, 8, None, None, make(white=0.0), o, p),
             (h, cam, 8, None, None, make(transfer=3), o, p), (h, cam, 8, None, None, make(gamma=INF), o, p),
             (h, cam, 8, rtc.Adaptive.make(0.01, 8, tile=0), None, ok, o, p), (h, cam, 8, rtc.Adaptive.make(0.01, 3, min_passes=4), None, ok, o, p),
             # (the stand-in's samples per pixel read as 0xA5A5A5A5: no pass count fits the sample index)
             (h, cam, 1, None, None, ok, o, p), (h, cam, 8, None, None, None, o, None), (h, cam, 8, adaptive, dn, ok, None, p)]
    for s, c, passes, a, d, film, rgb, rgba in calls:
        st = lib.rtc_render_filmed(s, C.byref(c) if c is not None else None, DEPTH, passes, C.byref(a) if a is not None else None,
                                   C.byref(d) if d is not None else None, C.byref(film) if film is not None else None, rgb, rgba, None)
        assert _status(lib, st) == "InvalidArgument", (passes, lib.rtc_last_error())
    assert bytes(handle) == b"\xa5" * SENTINEL and not out.any() and not px.any()


# ---- the loader
def _scene(film=None, sampling=None):
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}], "objects": [{"type": {"sphere": {}}}]}
    if film is not None:
        s["camera"]["film"] = film
    if sampling is not None:
        s["camera"]["sampling"] = sampling
    return json.dumps(s)


D = fb.DEFAULTS


@pytest.mark.parametrize("film, want", [
    (None, None), (False, None), (True, D), ({}, D),
    ({"exposure": 2.5}, dict(D, exposure=2.5)), ({"exposure": {"stops": -1}}, dict(D, exposure=0.5)),
    ({"exposure": {"stops": 1.5}}, dict(D, exposure=2.0 ** 1.5)),
    ({"auto-exposure": True}, dict(D, auto_key=0.18)), ({"auto-exposure": 0.36}, dict(D, auto_key=0.36)), ({"auto-exposure": 0}, D),
    ({"auto-exposure": False}, D),
    ({"bloom": True}, dict(D, **fb.BLOOM)), ({"bloom": False}, D),
    ({"bloom": {}}, dict(D, **fb.BLOOM)),                                         # (radius 12: sigma is 12 / 3)
    ({"bloom": {"radius": 6}}, dict(D, bloom_radius=6, bloom_sigma=2.0, bloom_threshold=1.0, bloom_intensity=0.15)),
    ({"bloom": {"radius": 32, "sigma": 9.5, "threshold": 0, "intensity": 0.5}},
     dict(D, bloom_radius=32, bloom_sigma=9.5, bloom_threshold=0.0, bloom_intensity=0.5)),
    ({"bloom": {"radius": 0}}, dict(D, bloom_radius=0, bloom_intensity=0.15)),
    ({"bloom": {"intensity": 0}}, dict(D, **dict(fb.BLOOM, bloom_intensity=0.0))),
    ({"tone-curve": "linear"}, dict(D, curve=fb.LINEAR)), ({"tone-curve": "reinhard"}, dict(D, curve=fb.REINHARD)),
    ({"tone-curve": "aces"}, D), ({"tone-curve": "hable", "white": 11.2}, dict(D, curve=fb.HABLE, white=11.2)),
    ({"transfer": "linear"}, dict(D, transfer=fb.T_LINEAR)), ({"transfer": "srgb"}, D),
    ({"transfer": {"gamma": 2.4}}, dict(D, transfer=fb.T_GAMMA, gamma=2.4)),
])
def test_loader_reads_the_key(rtc, film, want):
    f = rtc.HostScene(_scene(film)).film()
    assert (f.to_dict() if f is not None else None) == want


@pytest.mark.parametrize("film, error", [
    ({"exposure": 1, "iso": 100}, "UnknownField"), ({"bloom": {"radius": 3, "size": 2}}, "UnknownField"),
    ({"exposure": {"stops": 1, "ev": 2}}, "UnknownField"), ({"transfer": {"gamma": 2.2, "srgb": True}}, "UnknownField"),
    ({"exposure": 0}, "InvalidData"), ({"exposure": -1}, "InvalidData"), ({"exposure": "1"}, "InvalidData"), ({"exposure": {}}, "InvalidData"),
    ({"exposure": {"stops": "1"}}, "InvalidData"), ({"exposure": {"stops": 5000}}, "InvalidData"), ({"exposure": {"stops": -5000}}, "InvalidData"),
    ({"auto-exposure": -0.18}, "InvalidData"), ({"auto-exposure": "on"}, "InvalidData"),
    ({"bloom": 12}, "InvalidData"), ({"bloom": {"radius": 33}}, "InvalidData"), ({"bloom": {"radius": -1}}, "InvalidData"),
    ({"bloom": {"radius": 2.5}}, "InvalidData"), ({"bloom": {"radius": "6"}}, "InvalidData"), ({"bloom": {"sigma": 0}}, "InvalidData"),
    ({"bloom": {"sigma": -1}}, "InvalidData"), ({"bloom": {"threshold": -1}}, "InvalidData"), ({"bloom": {"intensity": -0.1}}, "InvalidData"),
    ({"bloom": {"intensity": True}}, "InvalidData"),
    ({"tone-curve": "filmic"}, "InvalidData"), ({"tone-curve": 2}, "InvalidData"),
    ({"white": 0}, "InvalidData"), ({"white": -4}, "InvalidData"), ({"white": [4]}, "InvalidData"),
    ({"transfer": "rec709"}, "InvalidData"), ({"transfer": 2.2}, "InvalidData"), ({"transfer": {}}, "InvalidData"),
    ({"transfer": {"gamma": 0}}, "InvalidData"), ({"transfer": {"gamma": "2.2"}}, "InvalidData"),
    (7, "InvalidData"), ("on", "InvalidData"), (None, "InvalidData"), ([], "InvalidData"),
])
def test_loader_refuses(rtc, film, error):
    s = json.loads(_scene())
    s["camera"]["film"] = film
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(json.dumps(s))
    assert e.value.name == error, e.value.args


def test_the_key_needs_no_passes_and_changes_no_table(rtc):
    """A file without the key, with it false and with it set flatten to the same tables and the same digest."""
    plain = rtc.HostScene(_scene())
    base = rtc.build_tables_digest(plain.desc)[0]
    counts = [getattr(plain.desc, f) for f, t in rtc.SceneDesc._fields_ if t is C.c_uint32]
    for film in (False, True, {"bloom": True, "auto-exposure": True}):
        hs = rtc.HostScene(_scene(film))
        assert hs.passes() == 1
        assert rtc.build_tables_digest(hs.desc)[0] == base
        assert [getattr(hs.desc, f) for f, t in rtc.SceneDesc._fields_ if t is C.c_uint32] == counts
    # beside "sampling", with its denoiser
    hs = rtc.HostScene(_scene({"bloom": True}, {"passes": 8, "denoise": True}))
    assert hs.film().to_dict() == dict(D, **fb.BLOOM) and hs.denoise() is not None and hs.passes() == 8
    # the fixture without its key is the fixture
    lamp = rtc.HostScene.from_file(fb.FILM_LAMP)
    scene = json.loads(open(fb.FILM_LAMP).read())
    del scene["camera"]["film"]
    bare = rtc.HostScene(json.dumps(scene))
    assert rtc.build_tables_digest(bare.desc)[0] == rtc.build_tables_digest(lamp.desc)[0]
    assert bare.film() is None and mb.mix(rtc).film() is None
    want = dict(D, exposure=2.0 ** -0.5, bloom_radius=6, bloom_sigma=2.0, bloom_threshold=1.0, bloom_intensity=0.2)
    assert lamp.film().to_dict() == want


# ---- the checker: known answers
def _image(h, w, seed, lo=0.0, hi=16.0):
    return np.random.default_rng(seed).uniform(lo, hi, (h, w, 3))


def test_the_identity_setting_returns_the_inputs_bits():
    image = _image(9, 13, 3)
    image[2, 3] = (-0.0, 1e-300, 1e300)
    out, E = fb.film(image, **fb.IDENTITY)
    assert E == 1.0 and np.array_equal(out.view(np.uint64), image.view(np.uint64))


def test_srgb():
    assert fb.develop(0.5, transfer=fb.T_SRGB) == 0.7353569830524495
    # the two branches meet at 0.0031308: the linear one is taken there
    assert fb.develop(0.0031308, transfer=fb.T_SRGB) == 12.92 * 0.0031308 and abs(12.92 * 0.0031308 - 0.040449936) <= 1e-15
    above = fb.develop(np.nextafter(0.0031308, 1.0), transfer=fb.T_SRGB)
    assert abs(above - 0.04044990748) <= 1e-11 and abs(above - 0.040449936) < 1e-7
    assert fb.develop(0.0, transfer=fb.T_SRGB) == 0.0 and fb.develop(-0.25, transfer=fb.T_SRGB) == 12.92 * -0.25
    assert abs(fb.develop(1.0, transfer=fb.T_SRGB) - 1.0) <= 1e-15


def test_gamma():
    assert fb.develop(0.25, transfer=fb.T_GAMMA, gamma=2.0) == 0.5
    assert fb.develop(0.0, transfer=fb.T_GAMMA) == 0.0 and fb.develop(-1.0, transfer=fb.T_GAMMA) == 0.0
    assert abs(fb.develop(0.5, transfer=fb.T_GAMMA, gamma=2.2) - 0.5 ** (1 / 2.2)) <= 1e-15


def test_curves():
    assert fb.develop(1.0, curve=fb.ACES) == 0.8037974683544302
    assert fb.develop(0.5, curve=fb.REINHARD, white=4.0) == 0.34375 and fb.develop(4.0, curve=fb.REINHARD, white=4.0) == 1.0
    for white in (1.0, 4.0, 11.2):
        assert abs(fb.develop(white, curve=fb.HABLE, white=white) - 1.0) <= 1e-15
    assert fb.develop(0.0, curve=fb.HABLE) == 0.0 or abs(fb.develop(0.0, curve=fb.HABLE)) <= 1e-15
    assert fb.develop(3.7, curve=fb.LINEAR) == 3.7
    grid = np.linspace(0.0, 16.0, 4097)
    for curve in (fb.LINEAR, fb.REINHARD, fb.ACES, fb.HABLE):
        t = np.array([fb.develop(float(c), curve=curve) for c in grid])
        assert (np.diff(t) > 0.0).all(), curve


# ---- the bloom
BLOOM_ONLY = dict(fb.IDENTITY, bloom_radius=3, bloom_sigma=1.5, bloom_threshold=1.0, bloom_intensity=1.0)


def _one_pixel(h, w, y, x, value=(5.0, 3.0, 9.0)):
    image = np.zeros((h, w, 3))
    image[y, x] = value
    lum = (0.2126 * value[0] + 0.7152 * value[1]) + 0.0722 * value[2]
    b = np.array(value) * ((lum - 1.0) / lum)
    return image, b


def test_one_bright_pixel_spreads_as_the_outer_product_of_the_weights():
    R = 3
    g = fb.weights(R, 1.5)
    assert abs(g[0] + 2.0 * g[1:].sum() - 1.0) <= 1e-15 and (np.diff(g) < 0).all()
    image, b = _one_pixel(11, 13, 5, 6)                              # (wider and taller than 2 R + 1)
    out, _ = fb.film(image, **BLOOM_ONLY)
    glow = out - image                                               # (intensity 1, LINEAR, LINEAR: out = x + B)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            want = g[abs(j)] * (g[abs(i)] * b)
            if (i, j) == (0, 0):                                     # ((x + B) - x is B within an ulp of x + B)
                assert np.abs(glow[5, 6] - want).max() <= 4e-15
            else:
                assert np.array_equal(glow[5 + j, 6 + i], want)
    window = np.zeros((11, 13), dtype=bool)
    window[5 - R:5 + R + 1, 6 - R:6 + R + 1] = True
    assert not glow[~window].any()
    assert np.array_equal(glow, glow[::-1]) and np.array_equal(glow[:, 6 - R:6 + R + 1], glow[:, 6 - R:6 + R + 1][:, ::-1])
    assert np.abs(glow.sum(axis=(0, 1)) - b).max() <= 1e-12


def test_a_bright_pixel_in_a_corner_loses_light():
    image, b = _one_pixel(11, 13, 0, 0)
    out, _ = fb.film(image, **BLOOM_ONLY)
    total = (out - image).sum(axis=(0, 1))
    assert (total < b).all() and (total > 0.25 * b).all()           # (a quarter of the kernel and the axes stay inside)


def test_a_pixel_below_the_threshold_does_not_bloom():
    image = np.full((7, 7, 3), 0.9)
    out, _ = fb.film(image, **BLOOM_ONLY)
    assert np.array_equal(out, image)


def test_threshold_0_with_intensity_0_is_no_bloom_to_the_bit():
    image = _image(12, 17, 8)
    for rest in (dict(curve=fb.ACES, transfer=fb.T_SRGB), dict(curve=fb.HABLE, transfer=fb.T_GAMMA), fb.IDENTITY):
        base = dict(fb.DEFAULTS, **rest)
        a, _ = fb.film(image, **dict(base, bloom_radius=5, bloom_sigma=2.0, bloom_threshold=0.0, bloom_intensity=0.0))
        b, _ = fb.film(image, **dict(base, bloom_radius=0))
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the automatic exposure
def test_a_flat_image_is_taken_to_the_key():
    """E = key / (L + eps) by the contract, which is key / L less key * eps / L^2 about: at L = 8, 2.8e-13"""
    L, key = 8.0, 0.18
    image = np.full((6, 5, 3), L)       # (Y of a grey is its value, the three weights summing to 1 within an ulp)
    _, E = fb.film(image, **dict(fb.IDENTITY, auto_key=key))
    assert abs(E - key / L) <= 1e-12
    assert abs(E - key / (L + 1e-10)) <= 1e-12 * (key / L)
    _, E2 = fb.film(image, **dict(fb.IDENTITY, auto_key=key, exposure=2.0))
    assert abs(E2 - 2.0 * E) <= 1e-15


def test_an_image_and_4_times_it_give_the_same_picture():
    """log(eps + 4 Y) is log 4 + log(eps / 4 + Y): the two exposures differ from 1 : 4 by 0.75 eps times the mean of 1 / Y,
    relatively - below 1e-12 for luminances of 100 and more, which the image here has"""
    image = _image(16, 24, 21, 100.0, 1000.0)
    setting = dict(fb.IDENTITY, auto_key=0.18)
    a, Ea = fb.film(image, **setting)
    b, Eb = fb.film(4.0 * image, **setting)
    assert abs(Ea / Eb - 4.0) <= 4e-12
    assert fb.close(b, a)[1] and a.max() < 1.0
    given, E = fb.film(image, E=0.5, **setting)                      # (an E handed in is the E used)
    assert E == 0.5 and np.array_equal(given, 0.5 * image)


def test_black_pixels_count_as_eps():
    image = np.zeros((4, 4, 3))
    image[0, 0] = -3.0                                               # (a negative luminance counts as 0)
    _, E = fb.film(image, **dict(fb.IDENTITY, auto_key=0.18))
    assert abs(E - 0.18 / 1e-10) <= 1e-12 * (0.18 / 1e-10)


def test_the_checker_refuses_what_the_contract_refuses():
    image = _image(3, 3, 1)
    for bad in (dict(exposure=0.0), dict(auto_key=-1.0), dict(bloom_radius=33), dict(bloom_radius=2, bloom_sigma=0.0), dict(bloom_threshold=-1.0),
                dict(bloom_intensity=NAN), dict(curve=4), dict(white=0.0), dict(transfer=3), dict(gamma=0.0)):
        with pytest.raises(ValueError):
            fb.film(image, **bad)


# ---- the fixture: its highlights with the film and with the plain clamp
def test_the_film_keeps_the_fixtures_highlights(rtc):
    hs = rtc.HostScene.from_file(fb.FILM_LAMP)
    ck = mb.scene_of(rtc, hs)
    cam = hs.camera()
    mean = np.zeros((cam.vsize, cam.hsize, 3))
    for p in range(hs.passes()):
        mean = mean + ck.render(cam, DEPTH, hs.sampling(), hs.spots(), sample_pass=p)[0]
    mean = mean / float(hs.passes())
    assert mean.max() >= 20.0                                       # (the lamp is well above 1.0)
    out, _ = fb.film(mean, **hs.film().to_dict())
    filmed, clamped = fb.share_at_255(fb.rgba(out)), fb.share_at_255(fb.rgba(mean))
    print(f"share of channels at 255: film {filmed:.4f}, plain clamp {clamped:.4f}")
    assert filmed < clamped
    assert 0.0 < filmed and clamped > 0.1                           # (the lamp itself still reaches white; the clamp cuts the walls flat)


# ---- documents and build
def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 30." in design
    for word in ("rtc_film_device", "rtc_render_filmed", "rtc_film_scratch_bytes", "rtc_film_row_kernel", "rtc_film_resolve_kernel",
                 "rtc_film_naive_row_kernel", "rtc_film_naive_resolve_kernel", "rtc_film_point_kernel", "rtc_film_log_kernel",
                 "rtc_film_exposure_kernel", "film_naive", "Narkowicz", "tests/cpp/film_oracle.cpp", "profiles/film/object_identity.txt",
                 "profiles/film/times_1080p.txt", "film_lamp.json", "Out of scope", "librtc_multi"):
        assert word in design, word
    for doc, word in (("README.md", "rtc_film_device"), ("README.md", "\"film\""), ("INTEGRATION.md", "rtc_film_device"),
                      ("INTEGRATION.md", "RtcFilmSetting"), (os.path.join("tools", "README.md"), "--film"),
                      (os.path.join("profiles", "HISTORY.md"), "film stage")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resource rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_film_log_kernel", "rtc_film_exposure_kernel", "rtc_film_point_kernel", "rtc_film_point_narrow_kernel",
                     "rtc_film_row_kernel", "rtc_film_resolve_kernel", "rtc_film_naive_row_kernel", "rtc_film_naive_resolve_kernel"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} |" in design, name
            assert k["vgprs_spilled"] == 0 and k["scratch_bytes_per_lane"] == 0


def test_object_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "film", "object_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_kernels_ext.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o",
                "rtc_occlusion.o", "rtc_shadowfilter.o", "rtc_media.o", "rtc_environment.o", "rtc_skylight.o", "rtc_indirect.o",
                "rtc_emitters.o", "rtc_accum.o", "rtc_adaptive.o", "rtc_denoise.o"):
        assert obj in text and "identical" in text
    assert "rtc_capi.o" in text and "kernel_resources.json" in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_film.o", "rtc_film.remarks", "libfilm_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_film.hip")).read()
    assert "static_assert(resolveLdsDoubles(RTC_FILM_MAX_RADIUS) * sizeof(double) <= kLdsLimit" in unit
    assert "rtc_kernels.hip" not in unit and "rtc_device.h" not in unit      # (a unit of its own: no render kernel compiles in it)
    oracle = open(os.path.join(REPO, "tests", "cpp", "film_oracle.cpp")).read()
    assert "#include \"" not in oracle                                        # (the checker includes nothing of the product)
