"""Shadow filters without a GPU: the checker (tests/cpp/sfilter_oracle.cpp) against the occlusion
checker it stacks on where no factor is partial, the exact small cases - one plane, a sphere in the way, the light inside a
sphere, an object behind the shaded point, filter 1 against "casts-shadow": false, stacked planes in two orders, an area
light -, the fixture's conditions, the loader's "shadow-filter" and rtch_scene_shadow_filters, the setter's validation through
the ABI, and the documents."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import occlusion_binding as ob
import sfilter_binding as sb
import test_torus_cpu as ttc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(REPO, "tests", "golden", "scenes")
SENTINEL = 1 << 16
W, H, DEPTH = 80, 45, 5
FILTER = [0.5, 0.25, 1.0]


# ---- the symbols
def test_symbols_are_exported(rtc):
    assert "rtc_scene_set_shadow_filters" in rtc.RTC_SYMBOLS and "rtch_scene_shadow_filters" in rtc.HOST_SYMBOLS
    assert "shadow_filter_kernels" in rtc.KERNEL_OPTIONS
    assert rtc.hip_lib().rtc_scene_set_shadow_filters is not None and rtc.host_lib().rtch_scene_shadow_filters is not None
    assert C.sizeof(rtc.ShadowFilters) == 16 and rtc.ShadowFilters.rgb.offset == 8
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_shadow_filters(rtc_scene *scene, const rtc_shadow_filters *filters);" in text
    assert "#define RTC_ABI_VERSION 3u" in text   # (the description and the ABI version stay as they were)
    rtc.set_option("shadow_filter_kernels", 1)
    rtc.set_option("shadow_filter_kernels", 0)


# ---- small scenes (shared with tests/test_shadow_filter_gpu.py)
def small_scene(extra=(), lights=None, floor=None):
    """A floor of ambient 0, specular 0 and diffuse 0.7 seen from above at a slant, every pixel on it, under a point light
    at (0, 10, 0); `extra`: the objects between (or not between) the floor and the light, none of them in the camera's view."""
    cam = {"width": 16, "height": 9, "field-of-view": 0.8, "from": [0, 3, -1], "to": [0, 0, 0], "up": [0, 0, 1]}
    floor = floor or {"pattern": {"type": {"checkers": [{"type": {"solid": [1, 0.9, 0.8]}}, {"type": {"solid": [0.3, 0.5, 0.7]}}]},
                                  "transform": [{"scale": [0.4, 0.4, 0.4]}]},
                      "ambient": 0, "diffuse": 0.7, "specular": 0}
    lights = lights or [{"point-light": {"position": [0, 10, 0], "intensity": [0.9, 0.8, 1.0]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": [{"type": {"plane": {}}, "material": floor}] + list(extra)})


def pane(y, filt=None, shadow=None):
    o = {"type": {"plane": {}}, "transform": [{"translate": [0, y, 0]}], "material": {}}
    if filt is not None:
        o["material"]["shadow-filter"] = filt
    if shadow is not None:
        o["casts-shadow"] = shadow
    return o


def ball(center, radius, filt=None):
    o = {"type": {"sphere": {}}, "transform": [{"scale": [radius] * 3}, {"translate": list(center)}], "material": {}}
    if filt is not None:
        o["material"]["shadow-filter"] = filt
    return o


CASES = {
    "bare": small_scene(),
    "one plane": small_scene([pane(5, FILTER)]),
    "sphere": small_scene([ball((1.2, 6, 0), 1, FILTER)]),
    "light inside": small_scene([ball((0, 10, 0), 2, FILTER)]),
    "behind": small_scene([ball((0, -3, 0), 1, FILTER)]),
    "filter 1": small_scene([pane(5, 1)]),
    "no shadow": small_scene([pane(5, None, False)]),
    "two a": small_scene([pane(5, [0.3, 0.7, 0.9]), pane(6, [0.6, 0.11, 0.77])]),
    "two b": small_scene([pane(5, [0.6, 0.11, 0.77]), pane(6, [0.3, 0.7, 0.9])]),
    "three a": small_scene([pane(5, [0.3, 0.7, 0.9]), pane(6, [0.6, 0.11, 0.77]), pane(7, [0.83, 0.37, 0.41])]),
    "three b": small_scene([pane(5, [0.83, 0.37, 0.41]), pane(6, [0.6, 0.11, 0.77]), pane(7, [0.3, 0.7, 0.9])]),
}


# an opaque pane in whose plane the light lies: its one entry of every shadow ray falls at t == distance
_AT_LIGHT = [{"point-light": {"position": [0.3, 5, 0.2], "intensity": [0.9, 0.8, 1.0]}}]
AT_LIGHT = small_scene([pane(5, 0)], _AT_LIGHT)
AT_LIGHT_BARE = small_scene([], _AT_LIGHT)


def check_small_cases(render):
    """The exact properties of the small scenes, for a `render(scene json) -> [9][16][3]`: the checker's here, the GPU's in
    tests/test_shadow_filter_gpu.py."""
    img = {k: render(v) for k, v in CASES.items()}
    bare = img["bare"]
    f = np.array(FILTER)
    assert (bare > 0).all()                                        # every pixel is a lit floor pixel
    # one plane: one rounding of the same product
    assert np.array_equal(img["one plane"], bare * f)
    # a sphere in the way: two entries, the filter squared; the other pixels keep their bits
    crossed = (img["sphere"] != bare).any(axis=2)
    assert crossed.any() and not crossed.all()
    assert np.array_equal(img["sphere"][crossed], (bare * (f * f))[crossed])
    # the light inside the sphere: the second entry lies beyond the light
    assert np.array_equal(img["light inside"], bare * f)
    # an entry behind the shaded point counts for nothing
    assert np.array_equal(img["behind"], bare)
    # a filter of 1 is no shadow at all
    assert np.array_equal(img["filter 1"], img["no shadow"]) and np.array_equal(img["filter 1"], bare)
    # two factors commute exactly; three agree to the last bits
    assert np.array_equal(img["two a"], img["two b"]) and not np.array_equal(img["two a"], bare)
    assert (np.abs(img["three a"] - img["three b"]) <= 1e-15 * bare).all()
    assert (img["three a"] < img["two a"]).all()
    return img


def _render(rtc, scene, filters="file", w=None, h=None, **kw):
    hs = rtc.HostScene(scene, sb.SFILT_DIR)
    cam = hs.camera(w, h) if w else hs.camera()
    return sb.scene_of(rtc, hs, filters).render(cam, DEPTH, spots=hs.spots(), **kw)


def test_small_cases_on_the_checker(rtc):
    img = check_small_cases(lambda scene: _render(rtc, scene)[0])
    # the sphere's pixels against the product written the other way round: (d * f) * f is another rounding for some pixel,
    # so the test above does tell T = f * f from two successive scalings
    bare, f = img["bare"], np.array(FILTER)
    print("pixels where d * (f * f) != (d * f) * f:", int((bare * (f * f) != (bare * f) * f).any(axis=2).sum()))


def test_an_entry_at_the_light_does_not_count(rtc):
    """t == distance to the bit for every one of the 144 shadow rays (t = vy / (vy / distance) here), and `t < distance`
    leaves the entry out: the floor is lit as without the pane."""
    with_pane, c = _render(rtc, AT_LIGHT)
    without, _ = _render(rtc, AT_LIGHT_BARE)
    assert c["at_light"] == 16 * 9 and c["t_blocked"] == 0 and c["factors"] == 0
    assert (with_pane > 0).all() and np.array_equal(with_pane, without)


def test_small_cases_count_their_factors(rtc):
    for name, entries in (("bare", 0), ("one plane", 1), ("sphere", None), ("light inside", 1), ("behind", 0), ("three a", 3)):
        _, c = _render(rtc, CASES[name])
        n = c["t_one"] + c["t_partial"] + c["t_blocked"]
        assert n == 16 * 9 and c["t_blocked"] == 0, name
        if entries is not None:
            assert c["factors"] == entries * n, name
        else:
            assert c["factors"] % 2 == 0 and 0 < c["factors"] < 2 * n, name   # a sphere gives two or none
        assert c["three_entries"] == (n if entries == 3 else 0), name


# ---- equality with the occlusion checker
@pytest.mark.parametrize("fixture", ["occlusion_mix", "filter_mix"])
@pytest.mark.parametrize("which", ["no table", "all-zero rows", "every filter 0"])
def test_without_filters_is_the_occlusion_checker_bit_for_bit(rtc, fixture, which):
    path, base = (ob.OCCL_MIX, ob.OCCL_DIR) if fixture == "occlusion_mix" else (sb.SFILT_MIX, sb.SFILT_DIR)
    scene = json.loads(open(path).read())
    if which == "every filter 0":
        for o in scene["objects"]:
            o["material"]["shadow-filter"] = [0, 0, 0]
    else:
        for o in scene["objects"]:
            o["material"].pop("shadow-filter", None)
    hs = rtc.HostScene(json.dumps(scene), base)
    if which == "every filter 0":
        table = hs.shadow_filters()
        assert table is not None and not table["rgb"].any()
    else:
        assert hs.shadow_filters() is None
        table = None if which == "no table" else {"rgb": np.zeros((hs.desc.n_materials, 3))}
    cam = hs.camera(W, H)
    ck = sb.scene_of(rtc, hs, table)
    got, c = ck.render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    want, co = ck.render_occl(cam, DEPTH, spots=hs.spots(), light_seed=3)
    assert np.array_equal(got, want)
    for k in sb.OCCL_COUNTERS:
        assert c[k] == co[k], k
    assert c["t_partial"] == 0 and c["t_blocked"] > 0 and c["t_one"] > 0


# ---- area lights
def _area_scene(filt, shadow=None):
    lights = [{"area-light": {"corner": [-0.5, 10, -0.5], "uvec": [1, 0, 0], "usteps": 2, "vvec": [0, 0, 1], "vsteps": 2,
                              "intensity": [0.9, 0.8, 1.0], "jitter": True}}]
    o = ball((0.6, 6, 0), 1, filt)
    if shadow is not None:
        o["casts-shadow"] = shadow
    return small_scene([o, ball((-1.5, 4, 0.3), 0.5)], lights)


def check_area_cases(render):
    opaque, ones, clear, part = (render(_area_scene(f, s)) for f, s in ((0, None), (1, None), (None, False), ([0.5, 0.25, 1.0], None)))
    assert np.array_equal(ones, clear)                       # filters of 0 and 1 only: the integer count's bits
    assert (opaque <= part).all() and (part <= clear).all()  # a partial filter lies between the two
    assert (part < clear).any() and (opaque < part).any()
    soft = (opaque < clear).any(axis=2)
    assert soft.any() and not soft.all()
    assert np.array_equal(part[~soft], clear[~soft])
    return opaque, clear, part


def test_area_light_on_the_checker(rtc):
    check_area_cases(lambda scene: _render(rtc, scene, light_seed=5)[0])
    # ... and with filters of 0 and 1 only the checker is the occlusion checker of the same scene without the sphere's shadow
    hs1 = rtc.HostScene(_area_scene(1), sb.SFILT_DIR)
    hs0 = rtc.HostScene(_area_scene(None, False), sb.SFILT_DIR)
    a, ca = sb.scene_of(rtc, hs1).render(hs1.camera(), DEPTH, light_seed=5)
    b, cb_ = sb.scene_of(rtc, hs0, None).render_occl(hs0.camera(), DEPTH, light_seed=5)
    assert np.array_equal(a, b) and ca["shadow_calls"] == cb_["shadow_calls"]


# ---- the fixture
def test_fixture_meets_its_conditions(rtc):
    hs = sb.mix(rtc)
    f = hs.shadow_filters()
    assert os.path.getsize(sb.SFILT_MIX) < 8192
    assert f["rgb"].shape == (hs.desc.n_materials, 3) and np.count_nonzero(f["rgb"].any(axis=1)) == 10
    assert [0.9, 0.9, 0.9] in f["rgb"].tolist()                   # `true`: the clear glass sphere's transparency
    assert hs.occlusion() is not None and hs.gloss() is not None and hs.spots() is not None
    kinds = {int(hs.desc.leaf_kind[i]) for i in range(hs.desc.n_leaves)}
    assert {rtc.RTC_SPHERE, rtc.RTC_PLANE, rtc.RTC_CUBE, rtc.RTC_TORUS, rtc.RTC_TRIANGLE} <= kinds
    img, c = sb.scene_of(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots(), light_seed=3)
    print(c)
    n = c["t_one"] + c["t_partial"] + c["t_blocked"]
    assert c["t_partial"] >= 0.1 * n and c["t_blocked"] >= 0.1 * n and c["t_one"] >= 0.1 * n
    assert c["three_entries"] >= 0.01 * n and c["three_partial"] >= 0.01 * n
    # between the all-opaque render and the render in which no filtering object casts a shadow
    opaque, _ = sb.scene_of(rtc, hs, None).render(hs.camera(W, H), DEPTH, spots=hs.spots(), light_seed=3)
    assert (img >= opaque - 1e-12).all() and not np.array_equal(img, opaque)


# ---- the loader
def _scene(material, **obj):
    return json.dumps({"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
                       "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
                       "objects": [dict({"type": {"sphere": {}}, "material": material}, **obj)]})


def test_loader_reads_every_form(rtc):
    assert rtc.HostScene(_scene({"shadow-filter": 0.25})).shadow_filters()["rgb"].tolist() == [[0.25, 0.25, 0.25]]
    assert rtc.HostScene(_scene({"shadow-filter": [0.5, 0.25, 1]})).shadow_filters()["rgb"].tolist() == [[0.5, 0.25, 1.0]]
    assert rtc.HostScene(_scene({"shadow-filter": True, "transparency": 0.75})).shadow_filters()["rgb"].tolist() == [[0.75] * 3]
    assert rtc.HostScene(_scene({"shadow-filter": True})).shadow_filters()["rgb"].tolist() == [[0.0] * 3]   # transparency 0
    assert rtc.HostScene(_scene({"shadow-filter": 1})).shadow_filters()["rgb"].tolist() == [[1.0] * 3]
    assert rtc.HostScene(_scene({"diffuse": 0.5})).shadow_filters() is None
    zero = rtc.HostScene(_scene({"shadow-filter": 0})).shadow_filters()       # the key is there, its value is zero
    assert zero is not None and not zero["rgb"].any()


def test_filter_is_inherited_overridden_and_a_row_only_when_non_zero(rtc):
    base = {"pattern": {"type": {"solid": [1, 0, 0]}}, "reflective": 0.5}
    objs = [{"type": {"sphere": {}}, "material": dict(base)},
            {"type": {"sphere": {}}, "material": dict(base, **{"shadow-filter": 0})},                     # the same row as the first
            {"type": {"group": [{"type": {"sphere": {}}},                                                # inherits 0.5
                                {"type": {"sphere": {}}, "material": {"shadow-filter": [0.1, 0.2, 0.3]}}]},   # overrides
             "material": dict(base, **{"shadow-filter": 0.5})},
            {"type": {"group": [{"type": {"sphere": {}}, "material": {"transparency": 0.25}}]},          # `true` follows the child's
             "material": dict(base, **{"shadow-filter": True, "transparency": 0.75})}]
    scene = json.loads(_scene({}))
    scene["objects"] = objs
    hs = rtc.HostScene(json.dumps(scene))
    assert hs.desc.n_materials == 4
    assert sorted(hs.shadow_filters()["rgb"].tolist()) == [[0.0] * 3, [0.1, 0.2, 0.3], [0.25] * 3, [0.5] * 3]
    mats = [int(hs.desc.leaf_material[i]) for i in range(hs.desc.n_leaves)]
    assert mats[0] == mats[1] and len(set(mats)) == 4


@pytest.mark.parametrize("material", [
    {"shadow-filter": -0.1}, {"shadow-filter": 1.5}, {"shadow-filter": "clear"}, {"shadow-filter": False},
    {"shadow-filter": [0.5, 0.5]}, {"shadow-filter": [0.5, 0.5, 0.5, 0.5]}, {"shadow-filter": [0.5, 2, 0.5]},
    {"shadow-filter": [0.5, "x", 0.5]}, {"shadow-filter": {"r": 1}}, {"shadow-filter": True, "transparency": 1.5},
    {"shadow-filter": True, "transparency": -0.5},
], ids=["negative", "above-1", "string", "false", "two", "four", "entry-above-1", "entry-string", "object", "true-transparency-above-1",
        "true-transparency-negative"])
def test_loader_refuses_a_malformed_entry_by_key(rtc, material):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(material))
    assert "shadow-filter" in str(e.value)


def test_host_filters_need_the_material_count(rtc):
    hs = sb.mix(rtc)
    a = np.zeros(9)
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_shadow_filters(hs._h, a.ctypes.data_as(C.POINTER(C.c_double)), None, 3))


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(SCENES) if f.endswith(".json")))
def test_reference_scenes_load_without_filters_and_with_their_digests(rtc, name):
    """tests/golden/torus_scenes/reference_tables.json: the digests of the 17 scenes' tables (tests/test_torus_cpu.py)."""
    want = json.load(open(os.path.join(REPO, "tests", "golden", "torus_scenes", "reference_tables.json")))
    hs = rtc.HostScene.from_file(name)
    assert hs.shadow_filters() is None
    assert ttc._digest(hs) == want[name]


def test_the_occlusion_fixture_has_no_filters(rtc):
    assert ob.mix(rtc).shadow_filters() is None


# ---- rtc_scene_set_shadow_filters: refused before anything changes
def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (tests/test_bump_cpu.py's way)."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    f, _keep = rtc.shadow_filters_struct({"rgb": [[0.5, 0.5, 0.5]]})
    assert _status(lib, lib.rtc_scene_set_shadow_filters(None, C.byref(f))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_shadow_filters(None, None)) == "InvalidArgument"


@pytest.mark.parametrize("rgb, words", [
    ([[0.1, np.nan, 0.1], [0, 0, 0]], "not finite"), ([[np.inf, 0, 0], [0, 0, 0]], "not finite"), ([[0, 0, 0], [0, -np.inf, 0]], "not finite"),
    ([[-1e-300, 0, 0], [0, 0, 0]], "outside [0, 1]"), ([[0, 0, 0], [0, 0, 1.0000000000000002]], "outside [0, 1]"),
], ids=["nan", "inf", "neg-inf", "below-0", "above-1"])
def test_setter_rejects_an_invalid_value_and_touches_nothing(rtc, rgb, words):
    """The table's own values are checked before its count against the handle: the stand-in's material count reads as
    0xA5A5A5A5, so each of these is refused for its own reason."""
    lib = rtc.hip_lib()
    handle = _stand_in()
    f, _keep = rtc.shadow_filters_struct({"rgb": rgb})
    st = lib.rtc_scene_set_shadow_filters(C.cast(handle, C.c_void_p), C.byref(f))
    assert _status(lib, st) == "InvalidArgument"
    assert words in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


@pytest.mark.parametrize("table", [{"rgb": np.zeros((0, 3))}, {"rgb": np.full((1, 3), 0.5)}, {"rgb": np.full((7, 3), 0.5)},
                                   {"rgb": None, "n_materials": 2}], ids=["0", "1", "7", "null-rows"])
def test_setter_rejects_a_wrong_material_count_and_touches_nothing(rtc, table):
    lib = rtc.hip_lib()
    handle = _stand_in()
    f, _keep = rtc.shadow_filters_struct(table)
    st = lib.rtc_scene_set_shadow_filters(C.cast(handle, C.c_void_p), C.byref(f))
    assert _status(lib, st) == "InvalidArgument"
    assert "n_materials" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


def test_python_refuses_a_misshapen_table(rtc):
    with pytest.raises(ValueError):
        rtc.shadow_filters_struct({"rgb": np.zeros(6)})


# ---- documents and build
def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("typedef struct rtc_shadow_filters {", "T = (1.0, 1.0, 1.0)", "blocked = T.r == 0.0 && T.g == 0.0 && T.b == 0.0",
                 "0.0 <= t < distance", "(dr, dg, db) = (dr * T.r, dg * T.g, db * T.b)", "(pr, pg, pb) = (pr * T.r, pg * T.g, pb * T.b)",
                 "v outer, u inner", "a pane of glass still darkens the corner behind it", "shadow_traced"):
        assert line in header, line
    assert "rtch_scene_shadow_filters" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    assert "shadow_filter_kernels" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "rtc_scene_set_shadow_filters" in open(os.path.join(REPO, "include", "rtc_multi.h")).read()


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 22." in design
    for word in ("rtc_scene_set_shadow_filters", "rtc_render_kernel_sfilter", "rtc_render_kernel_sfilter_bigworld", "shadow_filter_kernels",
                 "shadow-filter", "FilterVisitor", "kShadowOnly", "tests/cpp/sfilter_oracle.cpp",
                 "profiles/shadowfilter/disassembly_identity.txt", "profiles/shadowfilter/times_1080p_depth5.txt"):
        assert word in design, word
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resources rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_render_kernel_sfilter", "rtc_render_kernel_sfilter_bigworld"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} |" in design, name
    for doc, word in (("README.md", "rtc_scene_set_shadow_filters"), ("README.md", "shadow-filter"), ("INTEGRATION.md", "rtc_scene_set_shadow_filters"),
                      (os.path.join("tools", "README.md"), "--shadow-filter"), (os.path.join("profiles", "HISTORY.md"), "shadow filter")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)


def test_disassembly_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "shadowfilter", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o", "rtc_occlusion.o",
                "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_sfilter", "rtc_render_kernel_sfilter_bigworld", "rtc_render_kernel_occl", "rtc_render_kernel_occl_bigworld"):
        assert kernel in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_shadowfilter.o", "rtc_shadowfilter.remarks", "libsfilter_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_shadowfilter.hip")).read()
    for word in ("#define RTC_SFILT_TU", "#define RTC_OCCL_TU", "#define RTC_GLOSS_TU", "#define RTC_MESHUV_TU", "#define RTC_TORUS_TU",
                 '#include "rtc_kernels.hip"'):
        assert word in unit, word
    kernels = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_kernels.hip")).read()
    assert "static_assert(!SFILT || OCCL" in kernels and "struct FilterVisitor {" in kernels
