"""The environment without a GPU: the symbols and the struct, the setter's validation through the ABI on a
stand-in handle, the loader's "environment" and rtch_scene_environment, the appended pattern rows, the checker
(tests/cpp/environment_oracle.cpp) against values derived by hand - an empty world under a sky and in fog, a stripes and a
gradient sky in both projections, a mirror floor, a sun on a matte floor, occluders far up and far down its line, a closed
room of two sizes -, its identity with the media checker without a table, the fixtures' counters, and the documents.

The derived cases: 9 x 9, the centre pixel's ray is the camera's axis.  Ambient light is a term of Material.lighting, once
per light and per sun: the matte floor has ambient 0, diffuse 1, specular 0, so a sun of intensity I adds K * I times the
cosine, and nothing else does."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import environment_binding as eb
import media_binding as mdb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
W, H, DEPTH = 80, 45, 5
TOL = 1e-12
HALF_PI = 1.5707963267948966


# ---- ABI and options
def test_symbols_struct_and_option(rtc):
    assert "rtc_scene_set_environment" in rtc.RTC_SYMBOLS and "rtch_scene_environment" in rtc.HOST_SYMBOLS
    assert "environment_kernels" in rtc.KERNEL_OPTIONS
    assert rtc.hip_lib().rtc_scene_set_environment is not None and rtc.host_lib().rtch_scene_environment is not None
    E = rtc.Environment
    assert C.sizeof(E) == 56
    assert (E.rgb.offset, E.pattern.offset, E.projection.offset, E.n_suns.offset, E.sun_direction.offset, E.sun_rgb.offset) == (0, 24, 28, 32, 40, 48)
    assert (rtc.ENV_NO_PATTERN, rtc.ENV_SPHERE, rtc.ENV_CUBE, rtc.ENV_MAX_SUNS) == (0xFFFFFFFF, 0, 1, 16)
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_environment(rtc_scene *scene, const rtc_environment *environment);" in text
    for line in ("#define RTC_ENV_NO_PATTERN 0xFFFFFFFFu", "#define RTC_ENV_SPHERE 0u", "#define RTC_ENV_CUBE 1u", "#define RTC_ENV_MAX_SUNS 16u",
                 "#define RTC_ABI_VERSION 3u"):
        assert line in text, line
    assert "environment_kernels" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    rtc.set_option("environment_kernels", 1)
    rtc.set_option("environment_kernels", 0)
    zig = open(os.path.join(REPO, "integration", "gpu.zig")).read()
    assert "rtc_scene_set_environment" in zig and "RtcEnvironment" in zig


def test_headers_are_still_strict_c99():
    import test_abi
    test_abi.test_headers_are_valid_c()


# ---- rtc_scene_set_environment: refused on the host before anything changes
def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (tests/test_bump_cpu.py's way).  Its pattern
    count reads as 0xA5A5A5A5."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    e, _keep = rtc.environment_struct({"rgb": [0.5, 0.5, 0.5]})
    assert _status(lib, lib.rtc_scene_set_environment(None, C.byref(e))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_environment(None, None)) == "InvalidArgument"


UP = {"sun_direction": [[0, -1, 0]], "sun_rgb": [[1, 1, 1]]}


@pytest.mark.parametrize("env, words", [
    ({"rgb": [0.1, np.nan, 0.1]}, "not finite"),
    ({"rgb": [np.inf, 0, 0]}, "not finite"),
    ({"rgb": [0.1, -1e-300, 0.1]}, "negative"),
    ({"rgb": [1, 1, 1], "pattern": 0xFFFFFFFE}, "pattern"),
    ({"rgb": [1, 1, 1], "projection": 2}, "projection"),
    ({"sun_direction": np.tile([0, -1, 0], (17, 1)), "sun_rgb": np.ones((17, 3))}, "suns"),
    ({"sun_direction": [[0, -1, 0]], "sun_rgb": [[1, -0.5, 1]]}, "negative"),
    ({"sun_direction": [[0, -1, 0]], "sun_rgb": [[1, np.inf, 1]]}, "not finite"),
    ({"sun_direction": [[0, np.nan, 0]], "sun_rgb": [[1, 1, 1]]}, "not finite"),
    ({"sun_direction": [[0, 0, 0]], "sun_rgb": [[1, 1, 1]]}, "direction"),
    ({"sun_direction": [[1e200, 1e200, 0]], "sun_rgb": [[1, 1, 1]]}, "direction"),
], ids=["colour-nan", "colour-inf", "colour-negative", "pattern", "projection", "17-suns", "sun-negative", "sun-inf", "direction-nan",
        "direction-zero", "direction-overflows"])
def test_setter_rejects_an_invalid_table_and_touches_nothing(rtc, env, words):
    lib = rtc.hip_lib()
    handle = _stand_in()
    e, _keep = rtc.environment_struct(env)
    st = lib.rtc_scene_set_environment(C.cast(handle, C.c_void_p), C.byref(e))
    assert _status(lib, st) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert words in text and "environment:" in text
    assert bytes(handle) == b"\xa5" * SENTINEL


def test_setter_rejects_suns_without_a_table(rtc):
    lib = rtc.hip_lib()
    handle = _stand_in()
    e, _keep = rtc.environment_struct(UP)
    e.sun_rgb = None
    assert _status(lib, lib.rtc_scene_set_environment(C.cast(handle, C.c_void_p), C.byref(e))) == "InvalidArgument"
    e, _keep = rtc.environment_struct(UP)
    e.sun_direction = None
    assert _status(lib, lib.rtc_scene_set_environment(C.cast(handle, C.c_void_p), C.byref(e))) == "InvalidArgument"
    assert "without a table" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


def test_python_refuses_a_misshapen_table(rtc):
    with pytest.raises(ValueError):
        rtc.environment_struct({"rgb": [1, 2]})
    with pytest.raises(ValueError):
        rtc.environment_struct({"sun_direction": [[0, -1, 0]], "sun_rgb": np.ones((2, 3))})


# ---- the loader
STRIPES = {"type": {"stripes": [{"type": {"solid": [1, 0, 0]}}, {"type": {"solid": [0, 0, 1]}}]}}
MESH = {"type": {"texture-map": {"mesh": {"uv-pattern": {"checkers": {"width": 2, "height": 2, "patterns": [{"type": {"solid": [1, 1, 1]}},
                                                                                                         {"type": {"solid": [0, 0, 0]}}]}}}}}}


def _scene(environment=None, material=None):
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
         "objects": [{"type": {"sphere": {}}, "material": material or {"pattern": {"type": {"solid": [0.2, 0.4, 0.6]}}}}]}
    if environment is not None:
        s["environment"] = environment
    return json.dumps(s)


def _sun(**kw):
    return dict({"direction": [0, -1, 0], "intensity": [1, 1, 1]}, **kw)


@pytest.mark.parametrize("environment, want", [
    ({"color": [0.25, 0.5, 2]}, {"rgb": [0.25, 0.5, 2.0], "pattern": 0xFFFFFFFF, "projection": 0, "suns": 0}),
    ({"pattern": STRIPES}, {"rgb": [1.0, 1.0, 1.0], "projection": 0, "suns": 0}),
    ({"pattern": STRIPES, "color": [0.5, 0.5, 0.5], "projection": "cube"}, {"rgb": [0.5, 0.5, 0.5], "projection": 1, "suns": 0}),
    ({"projection": "sphere"}, {"rgb": [0.0, 0.0, 0.0], "pattern": 0xFFFFFFFF, "projection": 0, "suns": 0}),
    ({"suns": [_sun(), _sun(direction=[3, -4, 0], intensity=[0.5, 0.25, 0])]}, {"rgb": [0.0, 0.0, 0.0], "pattern": 0xFFFFFFFF, "suns": 2}),
    ({"suns": []}, {"rgb": [0.0, 0.0, 0.0], "suns": 0}),
], ids=["color", "pattern", "pattern-color-cube", "projection", "suns", "no-suns"])
def test_loader_reads_every_key(rtc, environment, want):
    e = rtc.HostScene(_scene(environment)).environment()
    assert e is not None
    assert e["rgb"] == want["rgb"] and len(e["sun_direction"]) == want["suns"] == len(e["sun_rgb"])
    for k in ("pattern", "projection"):
        if k in want:
            assert e[k] == want[k], k
    if "pattern" in environment:
        assert e["pattern"] != 0xFFFFFFFF
    if want["suns"] == 2:   # the rows as the file has them: the setter normalises
        assert e["sun_direction"].tolist() == [[0, -1, 0], [3, -4, 0]] and e["sun_rgb"].tolist() == [[1, 1, 1], [0.5, 0.25, 0]]


@pytest.mark.parametrize("environment, name", [
    ({}, "MissingField"),
    ({"suns": [{"intensity": [1, 1, 1]}]}, "MissingField"),
    ({"suns": [{"direction": [0, -1, 0]}]}, "MissingField"),
    ({"colour": [1, 1, 1]}, "UnknownField"),
    ({"color": [1, 1, 1], "horizon": 0.5}, "UnknownField"),
    ({"suns": [_sun(size=0.1)]}, "UnknownField"),
    ({"color": [1, 1]}, "LengthMismatch"),
    ({"suns": [_sun(direction=[0, -1, 0, 0])]}, "LengthMismatch"),
    ({"suns": [_sun(intensity=[1, 1])]}, "LengthMismatch"),
    ({"color": [1, "blue", 1]}, "InvalidData"),
    ({"color": 0.5}, "InvalidData"),
    ({"color": [1, -0.5, 1]}, "InvalidData"),
    ({"suns": [_sun(intensity=[1, -1, 1])]}, "InvalidData"),
    ({"suns": [_sun(direction=[0, 0, 0])]}, "InvalidData"),
    ({"suns": [_sun(direction=[1e200, 1e200, 0])]}, "InvalidData"),
    ({"suns": [_sun(direction=[0, True, 0])]}, "InvalidData"),
    ({"color": [1, 1, 1], "projection": "plane"}, "InvalidData"),
    ({"color": [1, 1, 1], "projection": 1}, "InvalidData"),
    ({"suns": [_sun()] * 17}, "InvalidData"),
    ({"suns": {"direction": [0, -1, 0]}}, "InvalidData"),
    ({"pattern": MESH}, "InvalidData"),
    ({"pattern": {"type": {"stripes": [STRIPES, {"type": {"perturb": MESH}}]}}}, "InvalidData"),
], ids=["empty", "sun-no-direction", "sun-no-intensity", "unknown-key", "unknown-key-beside", "unknown-sun-key", "color-two", "direction-four",
        "intensity-two", "color-string", "color-number", "color-negative", "intensity-negative", "direction-zero", "direction-overflows",
        "direction-bool", "projection-word", "projection-number", "17-suns", "suns-object", "mesh-map", "mesh-map-nested"])
def test_loader_refuses_a_malformed_environment(rtc, environment, name):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(environment))
    assert e.value.name == name, (e.value.name, str(e.value))


def test_sixteen_suns_load(rtc):
    assert len(rtc.HostScene(_scene({"suns": [_sun()] * 16})).environment()["sun_rgb"]) == 16


def _tables(desc):
    """every table of a description that patterns, texture maps and images reach, as lists"""
    def arr(p, n):
        return [p[i] for i in range(n)]
    np_, nt, nu, ni = desc.n_patterns, desc.n_texmaps, desc.n_uvs, desc.n_images
    n_px = sum(desc.img_width[i] * desc.img_height[i] for i in range(ni))
    return {"pat_kind": arr(desc.pat_kind, np_), "pat_inv": arr(desc.pat_inv, 16 * np_), "pat_rgb": arr(desc.pat_rgb, 3 * np_),
            "pat_a": arr(desc.pat_a, np_), "pat_b": arr(desc.pat_b, np_), "tex_mapping": arr(desc.tex_mapping, nt), "tex_uv": arr(desc.tex_uv, 6 * nt),
            "uv_kind": arr(desc.uv_kind, nu), "uv_image": arr(desc.uv_image, nu), "img_width": arr(desc.img_width, ni),
            "img_offset": arr(desc.img_offset, ni), "img_rgb_head": arr(desc.img_rgb, min(3 * n_px, 300)),
            "mat_pattern": arr(desc.mat_pattern, desc.n_materials), "n_leaves": [desc.n_leaves], "n_materials": [desc.n_materials]}


@pytest.mark.parametrize("path", [eb.SKY_MIX, eb.SKY_BOX], ids=["sky_mix", "sky_box"])
def test_environment_rows_follow_every_materials_rows(rtc, path):
    """A file with the key deleted flattens to the same tables, minus the trailing rows; the images the pattern names join
    the image table the same way."""
    scene = json.loads(open(path).read())
    with_env = rtc.HostScene(json.dumps(scene))
    del scene["environment"]
    bare = rtc.HostScene(json.dumps(scene))
    assert bare.environment() is None
    a, b = _tables(with_env.desc), _tables(bare.desc)
    assert with_env.desc.n_patterns > bare.desc.n_patterns and with_env.desc.n_images >= bare.desc.n_images
    for k in b:
        assert a[k][:len(b[k])] == b[k], k
    for k in ("mat_pattern", "n_leaves", "n_materials"):
        assert a[k] == b[k], k
    assert with_env.environment()["pattern"] >= bare.desc.n_patterns     # a trailing row
    assert with_env.environment()["pattern"] == with_env.desc.n_patterns - 1   # the pattern's root is interned last


def test_host_environment_is_the_table_of_rtch_scene_environment(rtc):
    hs = eb.mix(rtc)
    e = rtc.Environment()
    d, c, present = np.zeros((16, 3)), np.zeros((16, 3)), C.c_int()
    dp = C.POINTER(C.c_double)
    rtc._check_host(rtc.host_lib().rtch_scene_environment(hs._h, C.byref(e), d.ctypes.data_as(dp), c.ctypes.data_as(dp), C.byref(present)))
    env = hs.environment()
    assert present.value == 1 and e.n_suns == 2 and list(e.rgb) == env["rgb"] == [0.9, 0.9, 1.0] and e.pattern == env["pattern"]
    assert np.array_equal(d[:2], env["sun_direction"]) and np.array_equal(c[:2], env["sun_rgb"])
    assert C.addressof(e.sun_direction.contents) == d.ctypes.data     # the struct points into the caller's arrays
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_environment(hs._h, None, d.ctypes.data_as(dp), c.ctypes.data_as(dp), None))
    assert mdb.mix(rtc).environment() is None                          # the media fixture has no environment


def test_reference_scenes_load_without_an_environment(rtc):
    scenes = os.path.join(REPO, "tests", "golden", "scenes")
    for name in sorted(f for f in os.listdir(scenes) if f.endswith(".json")):
        assert rtc.HostScene.from_file(name).environment() is None, name


# ---- the checker against derived values (shared with tests/test_environment_gpu.py)
SKY_C = np.array([0.25, 0.5, 0.75])
FOG_D, FOG_F = 0.12, np.array([0.6, 0.3, 0.1])
COL_A, COL_B = np.array([0.9, 0.2, 0.1]), np.array([0.1, 0.3, 0.8])
FLOOR_K, SUN_I = np.array([0.8, 0.5, 0.2]), np.array([0.9, 0.7, 1.1])
FILTER_F, FILTER_H = 0.5, 0.25


def _solid(c):
    return {"type": {"solid": [float(x) for x in c]}}


def _camera(frm, to):
    return {"width": 9, "height": 9, "field-of-view": 0.5, "from": list(frm), "to": list(to), "up": [0, 1, 0]}


LOOK_RIGHT = _camera((0, 0, 0), (3, 0, 4))    # along (0.6, 0, 0.8)
LOOK_LEFT = _camera((0, 0, 0), (-3, 0, 4))    # along (-0.6, 0, 0.8)
LOOK_DOWN = _camera((0, 2, -2), (0, 0, 0))    # the axis meets the floor at the origin, at 45 degrees


def _matte_floor():
    return {"type": {"plane": {}}, "material": {"pattern": _solid(FLOOR_K), "ambient": 0, "diffuse": 1, "specular": 0}}


def _sun_env(direction):
    return {"suns": [{"direction": list(direction), "intensity": SUN_I.tolist()}]}


def _ball_at(y, material):
    return {"type": {"sphere": {}}, "transform": [{"translate": [0, y, 0]}], "material": material}


OPAQUE = {"pattern": _solid([0.3, 0.3, 0.3]), "ambient": 0, "diffuse": 0.5, "specular": 0}


def derived_scene(camera, objects=(), lights=(), environment=None, atmosphere=None):
    s = {"camera": camera, "lights": list(lights), "objects": list(objects)}
    if environment is not None:
        s["environment"] = environment
    if atmosphere is not None:
        s["atmosphere"] = {"density": atmosphere[0], "color": list(atmosphere[1])}
    return json.dumps(s)


def check_derived_cases(render):
    """The derived values, for a `render(scene json, depth) -> ([9][9][3], shadow rays traced)`: the checker's here, the GPU's
    in tests/test_environment_gpu.py.  Prints each figure before it asserts."""
    def centre(name, out, want):
        img = out[0]
        delta = float(np.abs(img[4, 4] - want).max())
        print(f"{name}: centre {img[4, 4]} derived {np.asarray(want)} |delta| {delta:.3e}")
        assert delta <= TOL, (name, delta)

    sky = {"color": SKY_C.tolist()}
    # ---- an empty world: every ray misses and every pixel is the sky's colour; in a fog every miss has T = 0 and every pixel
    # is the fog's colour; with a density of zero the sky again
    img, _ = render(derived_scene(LOOK_RIGHT, environment=sky), 5)
    print("empty world: max |delta|", float(np.abs(img - SKY_C).max()))
    assert np.abs(img - SKY_C).max() <= TOL
    img, _ = render(derived_scene(LOOK_RIGHT, environment=sky, atmosphere=(FOG_D, FOG_F)), 5)
    print("empty world in fog: max |delta|", float(np.abs(img - FOG_F).max()))
    assert np.abs(img - FOG_F).max() <= TOL
    img, _ = render(derived_scene(LOOK_RIGHT, environment=sky, atmosphere=(0.0, FOG_F)), 5)
    assert np.abs(img - SKY_C).max() <= TOL
    # ---- a stripes sky: p.x = 0.6 is in [0, 1): a; p.x = -0.6 is 1.4 modulo 2: b
    stripes = {"pattern": {"type": {"stripes": [_solid(COL_A), _solid(COL_B)]}}}
    centre("stripes, right", render(derived_scene(LOOK_RIGHT, environment=stripes), 5), COL_A)
    centre("stripes, left", render(derived_scene(LOOK_LEFT, environment=stripes), 5), COL_B)
    # ---- a gradient sky: the fraction of p.x - 0.6 on the unit sphere, 0.6 / 0.8 on the unit cube
    gradient = {"type": {"gradient": [_solid(COL_A), _solid(COL_B)]}}
    centre("gradient, sphere", render(derived_scene(LOOK_RIGHT, environment={"pattern": gradient, "projection": "sphere"}), 5),
           COL_A + (COL_B - COL_A) * 0.6)
    centre("gradient, cube", render(derived_scene(LOOK_RIGHT, environment={"pattern": gradient, "projection": "cube"}), 5),
           COL_A + (COL_B - COL_A) * 0.75)
    # ... and the sky's colour is the factor on the pattern's
    centre("gradient, tinted", render(derived_scene(LOOK_RIGHT, environment={"pattern": gradient, "color": SKY_C.tolist()}), 5),
           (COL_A + (COL_B - COL_A) * 0.6) * SKY_C)
    # ---- a mirror floor under a sky that is U above the horizon and D below it (stripes turned so that they run along y):
    # the reflected ray goes up; with depth 0 there is no reflected ray
    halves = {"pattern": {"type": {"stripes": [_solid(COL_A), _solid(COL_B)]}, "transform": [{"rotate-z": HALF_PI}]}}
    mirror = {"type": {"plane": {}}, "material": {"pattern": _solid([1, 1, 1]), "ambient": 0, "diffuse": 0, "specular": 0, "reflective": 1}}
    centre("mirror floor", render(derived_scene(LOOK_DOWN, [mirror], environment=halves), 5), COL_A)
    assert not render(derived_scene(LOOK_DOWN, [mirror], environment=halves), 0)[0][4, 4].any()
    centre("sky below the horizon", render(derived_scene(LOOK_DOWN, environment=halves), 5), COL_B)
    # ---- a sun on a matte floor: overhead K * I; at cosine 0.6, 0.6 * (K * I); from below nothing, and no shadow ray
    lit = FLOOR_K * SUN_I
    centre("sun overhead", render(derived_scene(LOOK_DOWN, [_matte_floor()], environment=_sun_env((0, -1, 0))), 5), lit)
    centre("sun at 0.6", render(derived_scene(LOOK_DOWN, [_matte_floor()], environment=_sun_env((0, -0.6, -0.8))), 5), 0.6 * lit)
    centre("sun of another length", render(derived_scene(LOOK_DOWN, [_matte_floor()], environment=_sun_env((0, -3, -4))), 5), 0.6 * lit)
    img, traced = render(derived_scene(LOOK_DOWN, [_matte_floor()], environment=_sun_env((0, 1, 0))), 5)
    assert not img.any() and traced == 0
    # ---- occluders on the sun's line through the floor point: 1e6 units up it blocks, 1e6 units down it does not; a sphere
    # that filters (f, f, f) is crossed twice
    up = _sun_env((0, -1, 0))
    assert not render(derived_scene(LOOK_DOWN, [_matte_floor(), _ball_at(1e6, OPAQUE)], environment=up), 5)[0][4, 4].any()
    centre("occluder below", render(derived_scene(LOOK_DOWN, [_matte_floor(), _ball_at(-1e6, OPAQUE)], environment=up), 5), lit)
    glass = dict(OPAQUE, **{"shadow-filter": [FILTER_F] * 3})
    centre("filtering sphere", render(derived_scene(LOOK_DOWN, [_matte_floor(), _ball_at(1e6, glass)], environment=up), 5),
           FILTER_F * FILTER_F * lit)
    # ---- a closed room around camera and floor, the sun outside; the point light of intensity zero inside marks the room.
    # The sun adds nothing; a room that filters (h, h, h) lets h * (K * I) through its ceiling.  At scale 2e5 the local
    # direction is 5e-6 long: below the room early-out's 1e-5.
    dark = [{"point-light": {"position": [0, 3, 0], "intensity": [0, 0, 0]}}]
    for scale in (5.0, 2e5):
        room = {"type": {"cube": {}}, "transform": [{"scale": [scale] * 3}], "material": dict(OPAQUE)}
        assert not render(derived_scene(LOOK_DOWN, [_matte_floor(), room], dark, up), 5)[0][4, 4].any(), scale
        room["material"]["shadow-filter"] = [FILTER_H] * 3
        centre(f"room of {scale:g} that filters", render(derived_scene(LOOK_DOWN, [_matte_floor(), room], dark, up), 5), FILTER_H * lit)


def _render(rtc, scene, depth=DEPTH):
    hs = rtc.HostScene(scene)
    img, c = eb.scene_of(rtc, hs).render(hs.camera(), depth, spots=hs.spots())
    return img, c["sun_clear"] + c["sun_blocked"] + c["sun_partial"] + c["t_one"] + c["t_partial"] + c["t_blocked"]


def test_derived_cases_on_the_checker(rtc):
    check_derived_cases(lambda scene, depth: _render(rtc, scene, depth))


# ---- identity
@pytest.mark.parametrize("fixture", ["sky_mix", "media_mix"])
def test_without_a_table_is_the_media_checker_bit_for_bit(rtc, fixture):
    hs = eb.mix(rtc) if fixture == "sky_mix" else mdb.mix(rtc)
    cam = hs.camera(W, H)
    ck = eb.scene_of(rtc, hs, environment=None)
    got, c = ck.render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    want, cm = ck.render_media(cam, DEPTH, spots=hs.spots(), light_seed=3)
    assert np.array_equal(got, want)
    for k in eb.MEDIA_ALL:
        assert c[k] == cm[k], k
    for k in eb.ENV_COUNTERS:
        assert c[k] == 0, k


def test_counts_with_the_environment(rtc):
    """A miss stays a miss and a sun is one shadow call per hit: primary and secondary stay, shadow_calls grows by the suns
    times the hits."""
    hs = eb.mix(rtc)
    cam = hs.camera(W, H)
    _, c1 = eb.scene_of(rtc, hs).render(cam, DEPTH, spots=hs.spots())
    _, c0 = eb.scene_of(rtc, hs, environment=None).render(cam, DEPTH, spots=hs.spots())
    assert c1["primary"] == c0["primary"] and c1["secondary"] == c0["secondary"]
    misses = c1["miss_camera"] + c1["miss_reflected"] + c1["miss_refracted"] + c1["miss_dark"]
    hits = c1["primary"] + c1["secondary"] - misses
    assert c1["shadow_calls"] == c0["shadow_calls"] + 2 * hits


# ---- the fixtures
def test_fixture_meets_its_conditions(rtc):
    hs = eb.mix(rtc)
    e = hs.environment()
    assert os.path.getsize(eb.SKY_MIX) < 8192
    assert len(e["sun_rgb"]) == 2 and e["pattern"] != rtc.ENV_NO_PATTERN and e["projection"] == rtc.ENV_SPHERE
    assert hs.occlusion() is not None and hs.shadow_filters() is not None and hs.gloss() is not None and hs.media() is not None
    assert hs.lights.n_lights == 1 and hs.desc.n_images == 1
    kinds = [int(hs.desc.leaf_kind[i]) for i in range(hs.desc.n_leaves)]
    assert rtc.RTC_TORUS in kinds and rtc.RTC_PLANE not in kinds          # no enclosing geometry: the floor is a slab
    img, c = eb.scene_of(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    print(c)
    for k in eb.ENV_COUNTERS:
        assert c[k] > 0, k
    assert c["miss_camera"] > W * H // 3                                  # the sky fills the frame above the floor
    assert img.std() > 0.05
    # the occluder far above the scene: without it more of the suns' rays are clear, and only theirs
    scene = json.loads(open(eb.SKY_MIX).read())
    far = [o for o in scene["objects"] if o.get("transform", [{}])[-1].get("translate", [0, 0, 0])[1] > 300]
    assert len(far) == 1
    scene["objects"].remove(far[0])
    near = rtc.HostScene(json.dumps(scene))
    _, c2 = eb.scene_of(rtc, near).render(near.camera(W, H), DEPTH, spots=near.spots())
    assert c2["sun_blocked"] < c["sun_blocked"] and c2["t_blocked"] == c["t_blocked"]


def test_sky_box_is_the_demo_without_its_cube(rtc):
    demo = json.loads(open(os.path.join(REPO, "tests", "golden", "scenes", "skybox_demo.json")).read())
    box = json.loads(open(eb.SKY_BOX).read())
    cube = [o for o in demo["objects"] if "cube" in o["type"]]
    assert len(cube) == 1 and box["objects"] == [o for o in demo["objects"] if "cube" not in o["type"]]
    assert box["camera"] == demo["camera"] and box["lights"] == demo["lights"]
    assert box["environment"]["projection"] == "cube" and box["environment"]["pattern"]["type"] == cube[0]["material"]["pattern"]["type"]
    assert box["environment"]["pattern"]["transform"] == [{"rotate-y": 0.3}]
    hs = eb.box(rtc)
    img, c = eb.scene_of(rtc, hs).render(hs.camera(80, 40), DEPTH, spots=hs.spots())
    assert c["miss_camera"] > 0 and c["miss_reflected"] > 0 and c["miss_refracted"] > 0 and img.std() > 0.05


# ---- documents and build
def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("typedef struct rtc_environment {", "len = sqrt((dx*dx + dy*dy) + dz*dz)", "len = max(|dx|, max(|dy|, |dz|))",
                 "p   = (dx / len, dy / len, dz / len)", "E.c = pattern == RTC_ENV_NO_PATTERN ? rgb.c : pattern_at(pattern, p).c * rgb.c",
                 "acc.c = acc.c + W.c * E.c", "a pattern transform turns the sky", "A miss stays a miss",
                 "Occlusion rays and shadow rays do not see the sky", "point_to_light = lv, distance = +infinity",
                 "shadow_calls grows by", "however far away", "Spot cones do not apply", "librtc_multi renders without it"):
        assert line in header, line
    assert "rtch_scene_environment" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    assert "rtc_scene_set_environment" in open(os.path.join(REPO, "include", "rtc_multi.h")).read()


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 24." in design
    for word in ("rtc_scene_set_environment", "rtc_render_kernel_env", "rtc_render_kernel_env_bigworld", "environment_kernels", "pattern_at_shared",
                 "segment_stays_inside_cube", "cube_entirely_behind", "far_limit", "tests/cpp/environment_oracle.cpp",
                 "profiles/environment/disassembly_identity.txt", "sky_mix.json", "sky_box.json", "Out of scope"):
        assert word in design, word
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resources rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_render_kernel_env", "rtc_render_kernel_env_bigworld"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} | {k['lds_bytes_per_block']} |" in design, name
            assert k["lds_bytes_per_block"] == resources.get("kernels", resources)[name.replace("_env", "_media")]["lds_bytes_per_block"]
    for doc, word in (("README.md", "rtc_scene_set_environment"), ("README.md", "suns"), ("INTEGRATION.md", "rtc_scene_set_environment"),
                      (os.path.join("tools", "README.md"), "--environment"), (os.path.join("profiles", "HISTORY.md"), "environment")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)


def test_disassembly_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "environment", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o", "rtc_occlusion.o",
                "rtc_shadowfilter.o", "rtc_media.o", "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_env", "rtc_render_kernel_env_bigworld", "rtc_render_kernel_media", "rtc_render_kernel_media_bigworld"):
        assert kernel in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_environment.o", "rtc_environment.remarks", "libenvironment_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_environment.hip")).read()
    for word in ("#define RTC_ENV_TU", "#define RTC_MEDIA_TU", "#define RTC_SFILT_TU", "#define RTC_OCCL_TU", "#define RTC_GLOSS_TU",
                 "#define RTC_MESHUV_TU", "#define RTC_TORUS_TU", '#include "rtc_kernels.hip"'):
        assert word in unit, word
    kernels = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_kernels.hip")).read()
    assert "static_assert(!ENV || MEDIA" in kernels and "pattern_at_shared" in kernels
