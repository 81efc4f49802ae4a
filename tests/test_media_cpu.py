"""Participating media without a GPU: the symbols and the struct, the setter's validation through the
ABI on a stand-in handle, the loader's "absorption" and "atmosphere" and rtch_scene_media, the checker
(tests/cpp/media_oracle.cpp) against values derived by hand - fog over an empty world and over a wall, a slab, two slabs, too
little depth, a sphere inside a sphere -, its identity with the shadow-filter checker where every table is zero, the bound
under a black fog, the fixture's counters, and the documents.

The derived cases: 9 x 9, the centre pixel's ray is the camera's axis.  Ambient light is a term of Material.lighting, once
per light, so a world with "lights": [] renders every surface black: there the fog's own term is all that is left, and that
is what the cases with "lights": [] hold.  Where a case needs the wall's colour C, the scene has one white point light and
the wall ambient 1, diffuse 0, specular 0: the light adds exactly C, whatever shadows it.  A refracted ray starts at the
hit's under_point, EPS = 1e-5 beyond the surface along the ray here, so a segment through a slab of thickness h has the
length h - EPS: the derived values say so."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import media_binding as mb
import sfilter_binding as sb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
W, H, DEPTH = 80, 45, 5
TOL = 1e-12
EPS = 1e-5   # PreComputations.new's over_point / under_point offset (world.zig)
HALF_PI = 1.5707963267948966


# ---- ABI and options
def test_symbols_struct_and_option(rtc):
    assert "rtc_scene_set_media" in rtc.RTC_SYMBOLS and "rtch_scene_media" in rtc.HOST_SYMBOLS
    assert "media_kernels" in rtc.KERNEL_OPTIONS
    assert rtc.hip_lib().rtc_scene_set_media is not None and rtc.host_lib().rtch_scene_media is not None
    assert C.sizeof(rtc.Media) == 48
    assert (rtc.Media.n_materials.offset, rtc.Media.absorption.offset, rtc.Media.fog_density.offset, rtc.Media.fog_color.offset) == (0, 8, 16, 24)
    assert rtc.NO_MEDIUM == 0xFFFFFFFF
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_media(rtc_scene *scene, const rtc_media *media);" in text
    assert "#define RTC_NO_MEDIUM 0xFFFFFFFFu" in text
    assert "#define RTC_ABI_VERSION 3u" in text   # (the description and the ABI version stay as they were)
    assert "media_kernels" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    rtc.set_option("media_kernels", 1)
    rtc.set_option("media_kernels", 0)


def test_headers_are_still_strict_c99():
    import test_abi
    test_abi.test_headers_are_valid_c()


# ---- rtc_scene_set_media: refused on the host before anything changes
def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (tests/test_bump_cpu.py's way)."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    m, _keep = rtc.media_struct({"absorption": [[0.5, 0.5, 0.5]]})
    assert _status(lib, lib.rtc_scene_set_media(None, C.byref(m))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_media(None, None)) == "InvalidArgument"


@pytest.mark.parametrize("media, words", [
    ({"absorption": [[0.1, -1e-300, 0.1], [0, 0, 0]]}, "negative"),
    ({"absorption": [[0, 0, 0], [0, 0, np.inf]]}, "not finite"),
    ({"absorption": [[np.nan, 0, 0], [0, 0, 0]]}, "not finite"),
    ({"absorption": [[0, 0, 0], [0, -np.inf, 0]]}, "not finite"),
    ({"absorption": np.zeros((2, 3)), "fog_density": -0.5}, "negative"),
    ({"absorption": np.zeros((2, 3)), "fog_density": np.inf}, "not finite"),
    ({"absorption": np.zeros((2, 3)), "fog_density": np.nan}, "not finite"),
    ({"absorption": np.zeros((2, 3)), "fog_density": 0.1, "fog_color": [0.1, -0.1, 0.1]}, "negative"),
    ({"absorption": np.zeros((2, 3)), "fog_density": 0.1, "fog_color": [0.1, 0.1, np.nan]}, "not finite"),
    ({"absorption": None, "n_materials": 2, "fog_color": [np.inf, 0, 0]}, "not finite"),
], ids=["negative", "inf", "nan", "neg-inf", "density-negative", "density-inf", "density-nan", "colour-negative", "colour-nan", "colour-inf"])
def test_setter_rejects_an_invalid_value_and_touches_nothing(rtc, media, words):
    """The table's own values are checked before its count against the handle: the stand-in's material count reads as
    0xA5A5A5A5, so each of these is refused for its own reason."""
    lib = rtc.hip_lib()
    handle = _stand_in()
    m, _keep = rtc.media_struct(media)
    st = lib.rtc_scene_set_media(C.cast(handle, C.c_void_p), C.byref(m))
    assert _status(lib, st) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert words in text and "media:" in text
    assert bytes(handle) == b"\xa5" * SENTINEL


@pytest.mark.parametrize("media", [{"absorption": np.zeros((0, 3))}, {"absorption": np.full((1, 3), 0.5)}, {"absorption": np.full((7, 3), 0.5)},
                                   {"absorption": None, "n_materials": 2, "fog_density": 0.1}], ids=["0", "1", "7", "null-rows"])
def test_setter_rejects_a_wrong_material_count_and_touches_nothing(rtc, media):
    lib = rtc.hip_lib()
    handle = _stand_in()
    m, _keep = rtc.media_struct(media)
    st = lib.rtc_scene_set_media(C.cast(handle, C.c_void_p), C.byref(m))
    assert _status(lib, st) == "InvalidArgument"
    assert "n_materials" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


def test_python_refuses_a_misshapen_table(rtc):
    with pytest.raises(ValueError):
        rtc.media_struct({"absorption": np.zeros(6)})
    with pytest.raises(ValueError):
        rtc.media_struct({"absorption": np.zeros((2, 3)), "fog_color": [1, 2]})


# ---- the loader
def _scene(material, atmosphere=None, **obj):
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
         "objects": [dict({"type": {"sphere": {}}, "material": material}, **obj)]}
    if atmosphere is not None:
        s["atmosphere"] = atmosphere
    return json.dumps(s)


def test_loader_reads_every_form(rtc):
    m = rtc.HostScene(_scene({"absorption": 0.25})).media()
    assert m["absorption"].tolist() == [[0.25] * 3] and m["fog_density"] == 0.0 and m["fog_color"] == [0.0] * 3
    assert rtc.HostScene(_scene({"absorption": [0.5, 0, 7.5]})).media()["absorption"].tolist() == [[0.5, 0.0, 7.5]]
    color, d = [0.35, 1, 0.9], 2.5
    got = rtc.HostScene(_scene({"absorption": {"color": color, "distance": d}})).media()["absorption"][0]
    want = np.array([-np.log(c) / d for c in color])
    assert np.abs(got - want).max() <= 1e-15 * want.max()        # (std::log against numpy's: a last bit)
    assert got[1] == 0.0 and not np.signbit(got[1])              # -log(1) / d is -0.0: stored as 0.0
    assert rtc.HostScene(_scene({"diffuse": 0.5})).media() is None
    zero = rtc.HostScene(_scene({"absorption": 0})).media()       # the key is there, its value is zero
    assert zero is not None and not zero["absorption"].any()
    fog = rtc.HostScene(_scene({}, {"density": 0.125, "color": [0.5, 0.25, 2]})).media()
    assert fog["fog_density"] == 0.125 and fog["fog_color"] == [0.5, 0.25, 2.0] and not fog["absorption"].any()
    both = rtc.HostScene(_scene({"absorption": 1}, {"density": 0, "color": [0, 0, 0]})).media()
    assert both["absorption"].tolist() == [[1.0] * 3] and both["fog_density"] == 0.0


def test_absorption_is_inherited_overridden_and_a_row_only_when_non_zero(rtc):
    base = {"pattern": {"type": {"solid": [1, 0, 0]}}, "reflective": 0.5}
    objs = [{"type": {"sphere": {}}, "material": dict(base)},
            {"type": {"sphere": {}}, "material": dict(base, absorption=0)},                                   # the same row as the first
            {"type": {"sphere": {}}, "material": dict(base, absorption={"color": [1, 1, 1], "distance": 3})},   # zero too: -0.0 is 0.0
            {"type": {"group": [{"type": {"sphere": {}}},                                                     # inherits 0.5
                                {"type": {"sphere": {}}, "material": {"absorption": [0.1, 0.2, 0.3]}}]},        # overrides
             "material": dict(base, absorption=0.5)}]
    scene = json.loads(_scene({}))
    scene["objects"] = objs
    hs = rtc.HostScene(json.dumps(scene))
    assert hs.desc.n_materials == 3
    assert sorted(hs.media()["absorption"].tolist()) == [[0.0] * 3, [0.1, 0.2, 0.3], [0.5] * 3]
    mats = [int(hs.desc.leaf_material[i]) for i in range(hs.desc.n_leaves)]
    assert mats[0] == mats[1] == mats[2] and len(set(mats)) == 3


@pytest.mark.parametrize("material, name", [
    ({"absorption": -0.1}, "InvalidData"), ({"absorption": "green"}, "InvalidData"), ({"absorption": True}, "InvalidData"),
    ({"absorption": [0.5, 0.5]}, "LengthMismatch"), ({"absorption": [0.5, 0.5, 0.5, 0.5]}, "LengthMismatch"),
    ({"absorption": [0.5, -2, 0.5]}, "InvalidData"), ({"absorption": [0.5, "x", 0.5]}, "InvalidData"),
    ({"absorption": {"color": [0.5, 0.5, 0.5]}}, "MissingField"), ({"absorption": {"distance": 1}}, "MissingField"),
    ({"absorption": {"color": [0.5, 0.5, 0.5], "distance": 0}}, "InvalidData"),
    ({"absorption": {"color": [0.5, 0.5, 0.5], "distance": -1}}, "InvalidData"),
    ({"absorption": {"color": [0.5, 0, 0.5], "distance": 1}}, "InvalidData"),
    ({"absorption": {"color": [0.5, 1.5, 0.5], "distance": 1}}, "InvalidData"),
    ({"absorption": {"color": [0.5, 0.5], "distance": 1}}, "LengthMismatch"),
    ({"absorption": {"color": 0.5, "distance": 1}}, "InvalidData"),
    ({"absorption": {"color": [0.5, 0.5, 0.5], "distance": 1, "tint": 1}}, "UnknownField"),
], ids=["negative", "string", "bool", "two", "four", "entry-negative", "entry-string", "no-distance", "no-color", "distance-0",
        "distance-negative", "color-0", "color-above-1", "color-two", "color-number", "unknown-field"])
def test_loader_refuses_a_malformed_absorption(rtc, material, name):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(material))
    assert e.value.name == name and ("absorption" in str(e.value) or name == "UnknownField")


@pytest.mark.parametrize("atmosphere, name", [
    ({"density": -1, "color": [0, 0, 0]}, "InvalidData"), ({"density": "thick", "color": [0, 0, 0]}, "InvalidData"),
    ({"color": [0, 0, 0]}, "MissingField"), ({"density": 0.1}, "MissingField"),
    ({"density": 0.1, "color": [0, 0]}, "LengthMismatch"), ({"density": 0.1, "color": [0, -1, 0]}, "InvalidData"),
    ({"density": 0.1, "color": 0.5}, "InvalidData"), ({"density": 0.1, "color": [0, 0, 0], "height": 2}, "UnknownField"),
    (0.1, "InvalidData"),
], ids=["density-negative", "density-string", "no-density", "no-color", "color-two", "color-negative", "color-number", "unknown-field", "number"])
def test_loader_refuses_a_malformed_atmosphere(rtc, atmosphere, name):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene({}, atmosphere))
    assert e.value.name == name or (name == "InvalidData" and e.value.name in ("InvalidData", "InvalidType", "UnexpectedToken"))


def test_scene_refuses_an_unknown_top_level_key(rtc):
    scene = json.loads(_scene({}))
    scene["fog"] = {"density": 1}
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(json.dumps(scene))
    assert e.value.name == "UnknownField"


def test_host_media_is_the_table_of_rtch_scene_media(rtc):
    hs = mb.mix(rtc)
    n = hs.desc.n_materials
    a, fog, present = np.zeros((n, 3)), np.zeros(4), C.c_int()
    dp = C.POINTER(C.c_double)
    rtc._check_host(rtc.host_lib().rtch_scene_media(hs._h, a.ctypes.data_as(dp), fog.ctypes.data_as(dp), C.byref(present), n))
    m = hs.media()
    assert present.value == 1 and np.array_equal(m["absorption"], a) and m["fog_density"] == fog[0] and m["fog_color"] == fog[1:].tolist()
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_media(hs._h, a.ctypes.data_as(dp), fog.ctypes.data_as(dp), None, n + 1))
    assert sb.mix(rtc).media() is None                       # the shadow-filter fixture has no media


# ---- the checker against derived values (shared with tests/test_media_gpu.py)
CAM = {"width": 9, "height": 9, "field-of-view": 0.5, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]}
WHITE = [{"point-light": {"position": [0, 8, -5], "intensity": [1, 1, 1]}}]
WALL_C = np.array([0.8, 0.5, 0.2])
WALL_Z = 6.0                      # the wall's plane: z = 6, the camera at z = -5
FOG_D, FOG_F = 0.12, np.array([0.25, 0.5, 0.75])
ABS_A = np.array([0.9, 0.1, 0.35])
SLAB_H = 1.5


def _wall():
    return {"type": {"plane": {}}, "transform": [{"rotate-x": HALF_PI}, {"translate": [0, 0, WALL_Z]}],
            "material": {"pattern": {"type": {"solid": WALL_C.tolist()}}, "ambient": 1, "diffuse": 0, "specular": 0}}


def _clear(absorption):
    return {"pattern": {"type": {"solid": [1, 1, 1]}}, "ambient": 0, "diffuse": 0, "specular": 0, "transparency": 1,
            "refractive-index": 1, "absorption": list(absorption)}


def _slab(z0, h, absorption=ABS_A):
    """a slab between z0 and z0 + h, wider than the view"""
    return {"type": {"cube": {}}, "transform": [{"scale": [20, 20, h / 2]}, {"translate": [0, 0, z0 + h / 2]}], "material": _clear(absorption)}


def _ball(radius, absorption):
    return {"type": {"sphere": {}}, "transform": [{"scale": [radius] * 3}], "material": _clear(absorption)}


def derived_scene(objects, lights=(), atmosphere=None):
    s = {"camera": CAM, "lights": list(lights), "objects": list(objects)}
    if atmosphere is not None:
        s["atmosphere"] = {"density": atmosphere[0], "color": list(atmosphere[1])}
    return json.dumps(s)


def check_derived_cases(render):
    """The derived values, for a `render(scene json, depth) -> [9][9][3]`: the checker's here, the GPU's in
    tests/test_media_gpu.py.  Prints each figure before it asserts."""
    def centre(name, img, want):
        delta = float(np.abs(img[4, 4] - want).max())
        print(f"{name}: centre {img[4, 4]} derived {np.asarray(want)} |delta| {delta:.3e}")
        assert delta <= TOL, (name, delta)

    # an empty world in fog (d, F): every ray misses, T = 0, every pixel is F; with d = 0: black
    img = render(derived_scene([], (), (FOG_D, FOG_F)), 5)
    centre("empty world in fog", img, FOG_F)
    assert np.abs(img - FOG_F).max() <= TOL
    assert not render(derived_scene([], (), (0.0, FOG_F)), 5).any()
    # the wall at distance D = 11 in fog: C e^(-dD) + F (1 - e^(-dD)); with "lights": [] the wall is black and F's term is left
    D = WALL_Z + 5.0
    T = np.exp(-FOG_D * D)
    centre("wall in fog", render(derived_scene([_wall()], WHITE, (FOG_D, FOG_F)), 5), WALL_C * T + FOG_F * (1.0 - T))
    centre("wall in fog, no light", render(derived_scene([_wall()], (), (FOG_D, FOG_F)), 5), FOG_F * (1.0 - T))
    # ... and with a density of zero the wall's own colour, to the bit
    assert np.array_equal(render(derived_scene([_wall()], WHITE, (0.0, FOG_F)), 5)[4, 4], WALL_C)
    # a slab of thickness h in front of the wall, no fog: the segment inside starts EPS behind the first face
    one = render(derived_scene([_slab(0.0, SLAB_H), _wall()], WHITE), 5)
    centre("slab", one, WALL_C * np.exp(-ABS_A * (SLAB_H - EPS)))
    # two slabs of h / 2 with a gap: two such segments - the single slab's value but for one more EPS
    two = render(derived_scene([_slab(-1.0, SLAB_H / 2), _slab(1.0, SLAB_H / 2), _wall()], WHITE), 5)
    centre("two slabs", two, WALL_C * np.exp(-ABS_A * (SLAB_H / 2 - EPS)) * np.exp(-ABS_A * (SLAB_H / 2 - EPS)))
    assert np.abs(two[4, 4] - one[4, 4]).max() <= 2.0 * ABS_A.max() * EPS          # e^(a EPS) - 1 < 2 a EPS, and C <= 1
    # too little depth to leave the slab: the ray ends inside it, black
    assert not render(derived_scene([_slab(0.0, SLAB_H), _wall()], WHITE), 1)[4, 4].any()
    centre("slab at depth 2", render(derived_scene([_slab(0.0, SLAB_H), _wall()], WHITE), 2), WALL_C * np.exp(-ABS_A * (SLAB_H - EPS)))
    # a sphere of radius 0.5 inside a sphere of radius 2, distinct absorptions: three chords on the axis
    a_out, a_in, R, r = np.array([0.2, 0.6, 0.05]), np.array([1.1, 0.3, 0.7]), 2.0, 0.5
    nested = render(derived_scene([_ball(R, a_out), _ball(r, a_in), _wall()], WHITE), 5)
    centre("sphere in sphere", nested, WALL_C * np.exp(-a_out * (R - r - EPS)) * np.exp(-a_in * (2 * r - EPS)) * np.exp(-a_out * (R - r - EPS)))
    # ... which is not what one medium for the whole way would give
    assert np.abs(nested[4, 4] - WALL_C * np.exp(-a_out * (2 * R - EPS))).max() > 1e-3


def _render(rtc, scene, depth=DEPTH, media="file"):
    hs = rtc.HostScene(scene, mb.MEDIA_DIR)
    return mb.scene_of(rtc, hs, media).render(hs.camera(), depth, spots=hs.spots())[0]


def test_derived_cases_on_the_checker(rtc):
    check_derived_cases(lambda scene, depth: _render(rtc, scene, depth))


# ---- identity and bounds
@pytest.mark.parametrize("fixture", ["media_mix", "filter_mix"])
@pytest.mark.parametrize("which", ["no table", "all-zero rows"])
def test_without_media_is_the_shadow_filter_checker_bit_for_bit(rtc, fixture, which):
    hs = mb.mix(rtc) if fixture == "media_mix" else sb.mix(rtc)
    table = None if which == "no table" else {"absorption": np.zeros((hs.desc.n_materials, 3)), "fog_density": 0.0, "fog_color": [0.3, 0.3, 0.3]}
    cam = hs.camera(W, H)
    ck = mb.scene_of(rtc, hs, table)
    got, c = ck.render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    want, cs = ck.render_sfilt(cam, DEPTH, spots=hs.spots(), light_seed=3)
    assert np.array_equal(got, want)
    for k in mb.SFILT_COUNTERS:
        assert c[k] == cs[k], k
    assert c["seg_tinted"] == 0 and c["miss_in_medium"] == 0


def test_black_fog_and_absorption_only_darken(rtc):
    hs = mb.mix(rtc)
    m = hs.media()
    m["fog_color"] = [0.0, 0.0, 0.0]
    cam = hs.camera(W, H)
    with_media, c = mb.scene_of(rtc, hs, m).render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    without, c0 = mb.scene_of(rtc, hs, None).render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    assert (with_media <= without + 1e-12).all() and (with_media < without - 1e-3).any()
    for k in ("primary", "secondary", "shadow_calls"):            # nothing is culled by a small weight
        assert c[k] == c0[k], k


# ---- the fixture
def test_fixture_meets_its_conditions(rtc):
    hs = mb.mix(rtc)
    m = hs.media()
    assert os.path.getsize(mb.MEDIA_MIX) < 8192
    assert m["fog_density"] > 0 and np.count_nonzero(m["absorption"].any(axis=1)) == 5
    thick_and_thin = [int(hs.desc.leaf_material[i]) for i in (2, 3)]        # the two pieces of the same glass share a row
    assert thick_and_thin[0] == thick_and_thin[1] and m["absorption"][thick_and_thin[0]].all()
    assert hs.occlusion() is not None and hs.shadow_filters() is not None and hs.spots() is not None
    assert hs.lights.n_lights == 3
    img, c = mb.scene_of(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots(), light_seed=3)
    print(c)
    for k in mb.MEDIA_COUNTERS:
        assert c[k] > 0, k
    assert c["unoccluded"] > 0 and c["t_partial"] > 0
    assert img.std() > 0.05


def test_reference_scenes_load_without_media(rtc):
    scenes = os.path.join(REPO, "tests", "golden", "scenes")
    for name in sorted(f for f in os.listdir(scenes) if f.endswith(".json")):
        assert rtc.HostScene.from_file(name).media() is None, name


# ---- documents and build
def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("typedef struct rtc_media {", "dist = t * sqrt((dx*dx + dy*dy) + dz*dz)", "T.c  = sigma.c == 0.0 ? 1.0 : exp(-(sigma.c * dist))",
                 "miss:      T.c  = sigma.c == 0.0 ? 1.0 : 0.0", "acc.c = acc.c + W.c * ((1.0 - T.c) * fog_color.c)", "W.c = W.c * T.c",
                 "the camera is taken to stand outside every", "A reflected child has its parent's medium", "Nothing is culled by a small weight",
                 "occlusion rays are not attenuated", "The fog is not lit by the lights", "librtc_multi renders"):
        assert line in header, line
    assert "rtch_scene_media" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    assert "rtc_scene_set_media" in open(os.path.join(REPO, "include", "rtc_multi.h")).read()


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 23." in design
    for word in ("rtc_scene_set_media", "rtc_render_kernel_media", "rtc_render_kernel_media_bigworld", "media_kernels", "absorption",
                 "atmosphere", "stack_ext", "tests/cpp/media_oracle.cpp", "profiles/media/disassembly_identity.txt",
                 "profiles/media/times_1080p_depth5.txt"):
        assert word in design, word
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resources rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_render_kernel_media", "rtc_render_kernel_media_bigworld"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} | {k['lds_bytes_per_block']} |" in design, name
    for doc, word in (("README.md", "rtc_scene_set_media"), ("README.md", "absorption"), ("INTEGRATION.md", "rtc_scene_set_media"),
                      (os.path.join("tools", "README.md"), "--media"), (os.path.join("profiles", "HISTORY.md"), "media")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)


def test_disassembly_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "media", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o", "rtc_occlusion.o",
                "rtc_shadowfilter.o", "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_media", "rtc_render_kernel_media_bigworld", "rtc_render_kernel_sfilter", "rtc_render_kernel_sfilter_bigworld"):
        assert kernel in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_media.o", "rtc_media.remarks", "libmedia_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_media.hip")).read()
    for word in ("#define RTC_MEDIA_TU", "#define RTC_SFILT_TU", "#define RTC_OCCL_TU", "#define RTC_GLOSS_TU", "#define RTC_MESHUV_TU",
                 "#define RTC_TORUS_TU", '#include "rtc_kernels.hip"'):
        assert word in unit, word
    kernels = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_kernels.hip")).read()
    assert "static_assert(!MEDIA || SFILT" in kernels and "lds_pend_x" in kernels
