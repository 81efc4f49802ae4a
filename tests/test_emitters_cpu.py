"""Emitter sampling without a GPU: the symbols and the struct, the setter's validation through the ABI on a
stand-in handle, the loader's "emitters" key and rtch_scene_emitters, the derived list against the checker's own derivation
(tests/cpp/emitters_oracle.cpp), the CDF picks, and the checker - its identity with the indirect checker wherever no sample is
drawn, a floor under a rectangular panel whose value is a closed form, the furnace of section 27 with a cube, whose mean must
not move, and the variance of a floor lit by a small panel with the samples and without -, the fixture's conditions, and the
documents.

The refusals that need a handle (a moving emitter in both call orders, the order of the setters, one entry too many on a
handle that has a table) are in tests/test_emitters_gpu.py: no handle exists without a device."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import emitters_binding as mb
import indirect_binding as ib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
W, H, DEPTH = 80, 45, 5
FIXTURES = {"indirect_mix": ib.INDIRECT_MIX, "emitters_mix": mb.EMITTERS_MIX}


# ---- ABI and options
def test_symbols_struct_and_option(rtc):
    assert "rtc_scene_set_emitters" in rtc.RTC_SYMBOLS and "rtch_scene_emitters" in rtc.HOST_SYMBOLS
    assert "rtc_diag_emitters" in rtc.RTC_DIAG_SYMBOLS and "emitter_kernels" in rtc.KERNEL_OPTIONS
    assert rtc.hip_lib().rtc_scene_set_emitters is not None and rtc.host_lib().rtch_scene_emitters is not None
    E = rtc.Emitters
    assert C.sizeof(E) == 16 and (E.samples.offset, E.seed.offset) == (0, 8)
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("int rtc_scene_set_emitters(rtc_scene *scene, const rtc_emitters *emitters);", "typedef struct rtc_emitters {",
                 "#define RTC_ABI_VERSION 3u", "#define RTC_MAX_EMITTERS 4096u", "#define RTC_EMITTER_MAX_SAMPLES 16u"):
        assert line in text, line
    assert (rtc.MAX_EMITTERS, rtc.EMITTER_MAX_SAMPLES, rtc.EMITTER_ROW) == (4096, 16, 18)
    diag = open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "emitter_kernels" in diag and "rtc_diag_emitters" in diag
    assert "rtc_scene_set_emitters" in open(os.path.join(REPO, "include", "rtc_multi.h")).read()
    assert "rtch_scene_emitters" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    rtc.set_option("emitter_kernels", 1)
    rtc.set_option("emitter_kernels", 0)
    zig = open(os.path.join(REPO, "integration", "gpu.zig")).read()
    assert "rtc_scene_set_emitters" in zig and "RtcEmitters" in zig


def test_headers_are_still_strict_c99_and_the_binding_matches():
    import test_abi
    test_abi.test_headers_are_valid_c()
    test_abi.test_zig_binding_matches_the_header()


def test_the_key_is_new_and_the_constants_agree():
    """0xC0AC29B7C97C50DD: the word of pi's expansion after the two section 27 took (its salt, and its decorrelation constant made
    odd); the product has it once, the checker once.  RTC_PI is rtc.h's in the device header, token for token."""
    device = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_device.h")).read()
    assert device.count("0xC0AC29B7C97C50DD") == 1
    assert open(os.path.join(REPO, "tests", "cpp", "emitters_oracle.cpp")).read().count("0xC0AC29B7C97C50DD") == 1
    pi_words = "452821E638D01377 BE5466CF34E90C6C C0AC29B7C97C50DD".split()
    assert device.index("0x" + pi_words[0]) < device.index("0x" + pi_words[1][:-1]) < device.index("0x" + pi_words[2])
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "#define RTC_PI 3.14159265358979323846\n" in header and "#define RTC_PI 3.14159265358979323846 " in device
    assert float("3.14159265358979323846") == math.pi


# ---- rtc_scene_set_emitters: refused on the host before anything changes
def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (tests/test_bump_cpu.py's way)."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    e = rtc.emitters_struct({"samples": 1})
    assert _status(lib, lib.rtc_scene_set_emitters(None, C.byref(e))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_emitters(None, None)) == "InvalidArgument"


@pytest.mark.parametrize("samples", [0, 17, 0xFFFFFFFF])
def test_setter_rejects_a_sample_count_outside_1_to_16_and_touches_nothing(rtc, samples):
    lib = rtc.hip_lib()
    handle = _stand_in()
    e = rtc.emitters_struct({"samples": samples, "seed": 3})
    st = lib.rtc_scene_set_emitters(C.cast(handle, C.c_void_p), C.byref(e))
    assert _status(lib, st) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert "samples" in text and "emitters:" in text
    assert bytes(handle) == b"\xa5" * SENTINEL


# ---- the loader
def _solid(c):
    return {"type": {"solid": [float(x) for x in c]}}


def _loader_scene(emitters="absent", indirect=True):
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
         "objects": [{"type": {"cube": {}}, "material": {"pattern": _solid([0.2, 0.4, 0.6]), "emission": 1.5}}]}
    if indirect:
        s["indirect"] = {"gain": 0.5, "bounces": 2, "seed": 4}
        if emitters != "absent":
            s["indirect"]["emitters"] = emitters
    return json.dumps(s)


@pytest.mark.parametrize("emitters, want", [
    (True, {"samples": 1, "seed": 0}),
    (False, None),
    (1, {"samples": 1, "seed": 0}),
    (16, {"samples": 16, "seed": 0}),
    ({}, {"samples": 1, "seed": 0}),
    ({"samples": 4}, {"samples": 4, "seed": 0}),
    ({"seed": 2 ** 53}, {"samples": 1, "seed": 2 ** 53}),
    ({"samples": 3, "seed": 9}, {"samples": 3, "seed": 9}),
], ids=["true", "false", "one", "sixteen", "defaults", "samples", "seed-2^53", "every-key"])
def test_loader_reads_the_key(rtc, emitters, want):
    hs = rtc.HostScene(_loader_scene(emitters))
    assert hs.emitters() == want
    assert hs.indirect()["gain"] == 0.5 and hs.indirect()["bounces"] == 2


@pytest.mark.parametrize("emitters, name", [
    ({"sample": 2}, "UnknownField"),
    ({"samples": 2, "gain": 1}, "UnknownField"),
    ("on", "InvalidData"),
    ([2], "InvalidData"),
    (0, "InvalidData"),
    (17, "InvalidData"),
    (2.5, "InvalidData"),
    (-1, "InvalidData"),
    ({"samples": 0}, "InvalidData"),
    ({"samples": 17}, "InvalidData"),
    ({"samples": "2"}, "InvalidData"),
    ({"samples": 1.5}, "InvalidData"),
    ({"seed": -1}, "InvalidData"),
    ({"seed": 0.5}, "InvalidData"),
    ({"seed": 2 ** 53 + 2}, "InvalidData"),
    ({"seed": "x"}, "InvalidData"),
], ids=["unknown-key", "unknown-key-beside", "string", "list", "zero", "seventeen", "fraction", "negative", "samples-0", "samples-17",
        "samples-string", "samples-fraction", "seed-negative", "seed-fraction", "seed-above-2^53", "seed-string"])
def test_loader_refuses_malformed_keys(rtc, emitters, name):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_loader_scene(emitters))
    assert e.value.name == name, (e.value.name, str(e.value))


def test_a_file_without_the_key_has_no_table_and_the_same_tables(rtc):
    """The fixture with the key deleted flattens to the same tables and the same digest: the key is no row of any of them."""
    import test_environment_cpu as ecpu
    with_key = mb.mix(rtc)
    scene = json.loads(open(mb.EMITTERS_MIX).read())
    del scene["indirect"]["emitters"]
    bare = rtc.HostScene(json.dumps(scene))
    assert with_key.emitters() == {"samples": 2, "seed": 11} and bare.emitters() is None
    assert ecpu._tables(with_key.desc) == ecpu._tables(bare.desc)
    digests = []
    for hs in (with_key, bare):
        d = C.c_uint64()
        rtc._check_hip(rtc.hip_lib().rtc_diag_build_tables(C.byref(hs.desc), C.byref(d), None))
        digests.append(d.value)
    assert digests[0] == digests[1]
    assert np.array_equal(with_key.indirect()["emission"], bare.indirect()["emission"])
    assert rtc.HostScene(_loader_scene(indirect=False)).emitters() is None and ib.mix(rtc).emitters() is None


def test_host_emitters_is_the_table_of_rtch_scene_emitters(rtc):
    hs = mb.mix(rtc)
    e, present = rtc.Emitters(), C.c_int()
    rtc._check_host(rtc.host_lib().rtch_scene_emitters(hs._h, C.byref(e), C.byref(present)))
    assert (present.value, e.samples, e.seed) == (1, 2, 11)
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_emitters(hs._h, None, None))
    rtc._check_host(rtc.host_lib().rtch_scene_emitters(ib.mix(rtc)._h, C.byref(e), C.byref(present)))
    assert (present.value, e.samples, e.seed) == (0, 1, 0)


# ---- identity: where no sample is drawn the render is the indirect checker's, bit for bit
def _spheres_only_emit(path):
    """the fixture with the emission taken from every leaf that is not a sphere: the derived list is empty"""
    scene = json.loads(open(path).read())
    for o in scene["objects"]:
        if "sphere" not in o["type"]:
            o.get("material", {}).pop("emission", None)
    return json.dumps(scene)


IDENTITY = ["no-table", "empty-list", "gain-0", "bounces-0"]


@pytest.mark.parametrize("case", IDENTITY)
@pytest.mark.parametrize("fixture", list(FIXTURES))
def test_where_no_sample_is_drawn_is_the_indirect_checker_bit_for_bit(rtc, fixture, case):
    path = FIXTURES[fixture]
    hs = rtc.HostScene(_spheres_only_emit(path)) if case == "empty-list" else rtc.HostScene.from_file(path)
    indirect = hs.indirect()
    if case == "gain-0":
        indirect = dict(indirect, gain=0.0)
    if case == "bounces-0":
        indirect = dict(indirect, bounces=0)
    cam = hs.camera(W, H)
    ck = mb.scene_of(rtc, hs, indirect=indirect, emitters=None if case == "no-table" else {"samples": 2, "seed": 11})
    got, c = ck.render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    want, ci = ck.render_indir(cam, DEPTH, spots=hs.spots(), light_seed=3)
    assert np.array_equal(got, want)
    for k in mb.IND_ALL:
        assert c[k] == ci[k], k
    for k in mb.EMIT_COUNTERS:
        assert c[k] == 0, k
    if case in ("no-table", "empty-list"):
        assert c["ind_formed"] > 0        # (the children are there: only the samples are not)
    rows, cdf = ck.emitter_list()
    assert (len(cdf) == 0) == (case == "empty-list")


# ---- the derived list: rtc_diag_emitters against the checker's own derivation, row for row and bit for bit
def _both_lists(rtc, hs, filters="file"):
    f = hs.shadow_filters() if filters == "file" else filters
    emission = hs.indirect()["emission"] if hs.indirect() is not None else None
    got = rtc.diag_emitters(hs.desc, emission, None if f is None else f["rgb"])
    want = mb.scene_of(rtc, hs, emitters={"samples": 1}, filters=f).emitter_list()
    return got, want


def _assert_same_list(got, want):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def _world(objects, indirect=None, size=(8, 8), camera=None):
    cam = camera or {"field-of-view": 1.0, "from": [0, 1.5, -6], "to": [0, 1, 0], "up": [0, 1, 0]}
    return json.dumps({"camera": dict(cam, width=size[0], height=size[1]), "lights": [], "objects": list(objects),
                       "indirect": indirect or {"gain": 0.8, "bounces": 1, "seed": 2}})


def _emissive(e, diffuse=0.0, colour=(1, 1, 1)):
    return {"pattern": _solid(colour), "ambient": 0, "diffuse": diffuse, "specular": 0, "emission": e}


FLOOR = {"type": {"plane": {}}, "material": {"pattern": _solid([0.8, 0.7, 0.6]), "ambient": 0, "diffuse": 0.9, "specular": 0}}


def sheared_cube_world():
    cube = {"type": {"cube": {}}, "transform": [{"scale": [0.5, 0.2, 0.4]}, {"shear": {"xy": 0.3, "xz": 0.1, "yz": 0.2, "zx": 0.15}}, {"rotate-x": 0.4}],
            "material": _emissive([1.0, 2.0, 0.5])}
    inner = {"type": {"group": [cube]}, "transform": [{"rotate-y": 0.7}, {"translate": [0.3, 0.0, 0.1]}]}
    outer = {"type": {"group": [inner]}, "transform": [{"rotate-z": -0.3}, {"translate": [0.2, 2.0, 0.5]}]}
    return _world([FLOOR, outer])


def one_entry_world():
    tri = {"type": {"triangle": {"p1": [-1, 2, -1], "p2": [1, 2, -1], "p3": [0, 2, 1]}}, "material": _emissive([0.5, 1.0, 2.0])}
    return _world([FLOOR, tri])


def two_entry_world():
    """two triangles whose weights differ by a factor of 1e12: the areas by 1e6, the emissions by 1e6"""
    big = {"type": {"triangle": {"p1": [-1, 2, -1], "p2": [1, 2, -1], "p3": [0, 2, 1]}}, "material": _emissive([1000.0, 1000.0, 1000.0])}
    s = 1e-3
    small = {"type": {"triangle": {"p1": [2 - s, 2, -s], "p2": [2 + s, 2, -s], "p3": [2, 2, s]}}, "material": _emissive([1e-3, 1e-3, 1e-3])}
    return _world([FLOOR, small, big])


def mesh_world(n):
    """a strip of n emissive triangles in one group, above the floor"""
    tris = []
    for i in range(n):
        x = -2.0 + 4.0 * (i // 2) / max(1, n // 2)
        dx = 4.0 / max(1, n // 2)
        if i % 2 == 0:
            p = ([x, 2.5, -1], [x + dx, 2.5, -1], [x + dx, 2.5, 1])
        else:
            p = ([x, 2.5, -1], [x + dx, 2.5, 1], [x, 2.5, 1])
        tris.append({"type": {"triangle": {"p1": p[0], "p2": p[1], "p3": p[2]}}})
    return _world([FLOOR, {"type": {"group": tris}, "material": _emissive([1.0, 0.9, 0.8])}])


@pytest.mark.parametrize("world, count", [("fixture", 8), ("sheared", 6), ("one", 1), ("two", 2), ("mesh", 4096)])
def test_derived_list_is_the_checkers_row_for_row(rtc, world, count):
    scene = {"fixture": None, "sheared": sheared_cube_world, "one": one_entry_world, "two": two_entry_world,
             "mesh": lambda: mesh_world(rtc.MAX_EMITTERS)}[world]
    hs = mb.mix(rtc) if scene is None else rtc.HostScene(scene())
    got, want = _both_lists(rtc, hs)
    assert len(got[1]) == count
    _assert_same_list(got, want)
    rows, cdf = got
    assert (np.diff(np.concatenate([[0.0], cdf])) > 0).all()
    assert np.allclose(np.linalg.norm(rows[:, 9:12], axis=1), 1.0, atol=1e-15)
    assert (rows[:, 15] == cdf[-1] / ((rows[:, 12] + rows[:, 13]) + rows[:, 14])).all()
    if world == "two":
        w = np.diff(np.concatenate([[0.0], cdf]))
        assert 0.5e12 < w[1] / w[0] < 2e12
    if world == "sheared":      # (six faces of one leaf, two by two parallel and of equal area)
        n = rows[:, 9:12]
        for k in (0, 2, 4):
            assert np.allclose(np.abs(n[k] @ n[k + 1]), 1.0, atol=1e-12)
        areas = np.diff(np.concatenate([[0.0], cdf])) / 3.5
        assert np.allclose(areas[0::2], areas[1::2], rtol=1e-12) and len(set(np.round(areas, 9))) == 3
    if world == "fixture":      # (the panel's six faces, then the quad's two triangles; the sphere is not listed)
        assert rows[:, 16].tolist() == [0.0] * 6 + [1.0] * 2
        assert len(set(rows[:6, 17])) == 1 and rows[6, 17] + 1 == rows[7, 17]


def test_one_entry_too_many_is_refused(rtc):
    hs = rtc.HostScene(mesh_world(rtc.MAX_EMITTERS + 1))
    with pytest.raises(rtc.RtcError) as e:
        rtc.diag_emitters(hs.desc, hs.indirect()["emission"])
    assert e.value.name == "Unsupported"
    with pytest.raises(RuntimeError):
        mb.scene_of(rtc, hs, emitters={"samples": 1}).emitter_list()


def test_what_is_not_listed(rtc):
    """a leaf that casts no shadow, a leaf whose material lets light through, a leaf below a csg node, and every kind that is
    neither a triangle nor a cube: none of them is an entry, in the product's list or in the checker's"""
    e = [1.0, 1.0, 1.0]
    cube = lambda x, **kw: dict({"type": {"cube": {}}, "transform": [{"scale": [0.2, 0.2, 0.2]}, {"translate": [x, 2, 0]}], "material": _emissive(e)}, **kw)
    filtered = cube(-2)
    filtered["material"] = dict(_emissive(e), **{"shadow-filter": [0.5, 0.5, 0.5]})
    objects = [FLOOR, cube(-3, **{"casts-shadow": False}), filtered,
               {"type": {"csg": {"left": cube(-1), "right": cube(-0.9), "operation": "union"}}},
               {"type": {"sphere": {}}, "transform": [{"translate": [0, 3, 0]}], "material": _emissive(e)},
               {"type": {"cylinder": {"min": 0, "max": 1, "closed": True}}, "transform": [{"translate": [3, 3, 0]}], "material": _emissive(e)},
               cube(2)]
    hs = rtc.HostScene(_world(objects))
    got, want = _both_lists(rtc, hs)
    _assert_same_list(got, want)
    assert len(got[1]) == 6 and len(set(got[0][:, 17])) == 1
    # (without the filter table the filtered cube is listed too)
    got, want = _both_lists(rtc, hs, filters=None)
    _assert_same_list(got, want)
    assert len(got[1]) == 12


def test_cdf_picks_land_on_the_entries_the_checker_names(rtc):
    below_one = float(np.nextafter(1.0, 0.0))
    for scene in (mb.mix(rtc), rtc.HostScene(two_entry_world()), rtc.HostScene(one_entry_world()), rtc.HostScene(mesh_world(257))):
        (rows, cdf), _ = _both_lists(rtc, scene)
        total = cdf[-1]
        draws = [0.0, below_one, 0.5]
        for k in range(len(cdf)):
            u = cdf[k] / total
            draws += [float(np.nextafter(u, 0.0)), min(u, below_one), float(np.nextafter(min(u, below_one), 0.0))]
        for u0 in draws:
            got, want = rtc.diag_emitter_pick(cdf, u0), mb.pick(cdf, u0)
            assert got == want, (u0, got, want)
            assert cdf[got] > u0 * total or got == len(cdf) - 1
            assert got == 0 or not cdf[got - 1] > u0 * total
        assert rtc.diag_emitter_pick(cdf, 0.0) == 0 and rtc.diag_emitter_pick(cdf, below_one) == len(cdf) - 1


# ---- analytic: a point of a floor under a parallel rectangular panel
PANEL_A, PANEL_B, PANEL_H = 1.0, 0.75, 1.25          # half-widths along x and z, height
PANEL_E = np.array([2.0, 1.5, 0.5])
AN_K, AN_KD, AN_G = np.array([0.8, 0.6, 0.4]), 0.9, 0.7
AN_PASSES, AN_SAMPLES = 256, 4


def form_factor(a, b, h):
    """A differential element under the CENTRE of a parallel rectangle 2a x 2b at height h: four times the corner formula
    F = 1 / (2 pi) * (a / sqrt(a^2 + h^2) * atan(b / sqrt(a^2 + h^2)) + b / sqrt(b^2 + h^2) * atan(a / sqrt(b^2 + h^2)))"""
    p, q = math.sqrt(a * a + h * h), math.sqrt(b * b + h * h)
    return 4.0 / (2.0 * math.pi) * (a / p * math.atan(b / p) + b / q * math.atan(a / q))


def panel_scene():
    a, b, h = PANEL_A, PANEL_B, PANEL_H
    quad = {"type": {"group": [{"type": {"triangle": {"p1": [-a, h, -b], "p2": [a, h, -b], "p3": [a, h, b]}}},
                               {"type": {"triangle": {"p1": [-a, h, -b], "p2": [a, h, b], "p3": [-a, h, b]}}}]},
            "material": _emissive(PANEL_E.tolist())}
    floor = {"type": {"plane": {}}, "material": {"pattern": _solid(AN_K), "ambient": 0, "diffuse": AN_KD, "specular": 0}}
    # (looking straight down from between the floor and the panel)
    camera = {"field-of-view": 0.02, "from": [0, 0.5, 0], "to": [0, 0, 0], "up": [0, 0, 1]}
    return _world([floor, quad], indirect={"gain": AN_G, "bounces": 1, "seed": 6}, size=(1, 1), camera=camera)


def _passes(rtc, scene, n, emitters, flags=0, depth=DEPTH):
    hs = rtc.HostScene(scene)
    ck = mb.scene_of(rtc, hs, emitters=emitters, flags=flags)
    cam = hs.camera()
    return np.array([ck.render(cam, depth, sample_pass=p, threads=1)[0] for p in range(n)])


def _mean_and_se(images):
    return images.mean(axis=0), images.std(axis=0, ddof=1) / math.sqrt(len(images))


@pytest.fixture(scope="module")
def panel_runs(rtc):
    em = {"samples": AN_SAMPLES, "seed": 21}
    return {flags: _passes(rtc, panel_scene(), AN_PASSES, em, flags) for flags in (0, mb.NO_PI, mb.NO_COS_E, mb.HALF_AREA)}


def test_a_floor_under_a_panel_gets_the_form_factor(rtc, panel_runs):
    want = (AN_K * AN_KD) * AN_G * PANEL_E * form_factor(PANEL_A, PANEL_B, PANEL_H)
    mean, se = _mean_and_se(panel_runs[0])
    z = (mean[0, 0] - want) / se[0, 0]
    print(f"panel: mean {mean[0, 0]} closed form {want} standard error {se[0, 0]} z {z} relative se {se[0, 0] / want}")
    assert (np.abs(z) <= 4.0).all()
    assert (se[0, 0] / want < 0.02).all()      # (tight enough for the three mistakes below: the nearest is 20 % away)


@pytest.mark.parametrize("flags, name", [(mb.NO_PI, "no-pi"), (mb.NO_COS_E, "no-cos-e"), (mb.HALF_AREA, "half-area")])
def test_each_mistake_misses_the_bound(rtc, panel_runs, flags, name):
    want = (AN_K * AN_KD) * AN_G * PANEL_E * form_factor(PANEL_A, PANEL_B, PANEL_H)
    mean, se = _mean_and_se(panel_runs[flags])
    z = (mean[0, 0] - want) / se[0, 0]
    print(f"panel, {name}: mean {mean[0, 0]} closed form {want} z {z}")
    assert (np.abs(z) > 4.0).all()


def test_the_panels_child_adds_nothing_twice(rtc):
    """every child of the floor point either meets the panel, whose emission its parent's samples counted, or nothing"""
    hs = rtc.HostScene(panel_scene())
    _, c = mb.scene_of(rtc, hs, emitters={"samples": AN_SAMPLES, "seed": 21}).render(hs.camera(), DEPTH)
    assert c["emit_drawn"] == AN_SAMPLES and c["emit_walks"] == AN_SAMPLES and c["emit_blocked"] == 0
    assert c["ind_formed"] == 1 and c["shadow_calls"] == AN_SAMPLES


# ---- equal means: section 27's furnace with a cube
FUR_K, FUR_KD, FUR_G = np.array([0.8, 0.5, 0.2]), 0.9, 1.1
FUR_E = np.array([0.25, 0.5, 1.0])
FUR_PASSES = 512


def cube_furnace_scene(bounces, size=4):
    wall = {"type": {"cube": {}}, "transform": [{"scale": [3, 2.5, 3.5]}],
            "material": {"pattern": _solid(FUR_K), "ambient": 0, "diffuse": FUR_KD, "specular": 0, "emission": FUR_E.tolist()}}
    camera = {"field-of-view": 1.2, "from": [0.3, 0.2, -0.5], "to": [0, 0.4, 1], "up": [0, 1, 0]}
    return _world([wall], indirect={"gain": FUR_G, "bounces": bounces, "seed": 5}, size=(size, size), camera=camera)


def furnace_value(bounces, depth):
    a = (FUR_K * FUR_KD) * FUR_G
    v = FUR_E.copy()
    for _ in range(min(bounces, depth)):
        v = FUR_E + a * v
    return v


@pytest.mark.parametrize("bounces", [1, 2])
def test_cube_furnace_keeps_its_mean(rtc, bounces):
    want = furnace_value(bounces, DEPTH)
    off = _passes(rtc, cube_furnace_scene(bounces), 2, None)
    assert np.abs(off - want).max() <= 1e-15 * want.max() * 4       # (the series, to the last bits, whatever the draws: as before)
    on = _passes(rtc, cube_furnace_scene(bounces), FUR_PASSES, {"samples": 2, "seed": 13})
    # (the sixteen pixels are independent estimates of one value: their mean over passes and pixels)
    per_pass = on.mean(axis=(1, 2))
    mean, se = per_pass.mean(axis=0), per_pass.std(axis=0, ddof=1) / math.sqrt(FUR_PASSES)
    z = (mean - want) / se
    print(f"cube furnace, {bounces} bounces: mean {mean} series {want} standard error {se} z {z}")
    assert (np.abs(z) <= 4.0).all()
    twice = _passes(rtc, cube_furnace_scene(bounces), FUR_PASSES, {"samples": 2, "seed": 13}, flags=mb.NO_SUPPRESS).mean(axis=(1, 2))
    z2 = (twice.mean(axis=0) - want) / (twice.std(axis=0, ddof=1) / math.sqrt(FUR_PASSES))
    print(f"cube furnace, {bounces} bounces, emission counted twice: mean {twice.mean(axis=0)} z {z2}")
    assert (z2 > 4.0).all()


def test_cube_furnace_counts(rtc):
    """every child of a wall meets a wall: all of them are suppressed, and every sample is drawn towards a face"""
    hs = rtc.HostScene(cube_furnace_scene(2))
    _, c = mb.scene_of(rtc, hs, emitters={"samples": 2, "seed": 13}).render(hs.camera(), DEPTH)
    assert c["ind_formed"] == 2 * 16 and c["emit_suppressed"] == 2 * 16 and c["emit_drawn"] == 2 * 2 * 16
    assert c["emit_skip_cos_x"] > 0 and c["emit_blocked"] == 0
    assert c["emit_walks"] == c["shadow_calls"] == c["emit_drawn"] - c["emit_skip_cos_x"] - c["emit_skip_cos_e"] - c["emit_skip_r"]


# ---- variance: a floor lit only by a small panel
def small_panel_scene(size=8):
    s, h = 0.25, 3.0
    quad = {"type": {"group": [{"type": {"triangle": {"p1": [-s, h, -s], "p2": [s, h, -s], "p3": [s, h, s]}}},
                               {"type": {"triangle": {"p1": [-s, h, -s], "p2": [s, h, s], "p3": [-s, h, s]}}}]},
            "material": _emissive([20.0, 20.0, 20.0])}
    camera = {"field-of-view": 1.0, "from": [0, 2.5, 0], "to": [0, 0, 0], "up": [0, 0, 1]}
    return _world([FLOOR, quad], indirect={"gain": 1.0, "bounces": 1, "seed": 3}, size=(size, size), camera=camera)


def test_samples_lower_the_variance_of_a_floor_under_a_small_panel(rtc):
    n = 64
    on = _passes(rtc, small_panel_scene(), n, {"samples": 1, "seed": 5})
    off = _passes(rtc, small_panel_scene(), n, None)
    var_on, var_off = on.var(axis=0, ddof=1).mean(), off.var(axis=0, ddof=1).mean()
    print(f"small panel: per-pixel variance with samples {var_on:.6e}, without {var_off:.6e}, ratio {var_off / var_on:.1f}; "
          f"means {on.mean():.5f} / {off.mean():.5f}")
    assert var_on < var_off
    assert abs(on.mean() - off.mean()) < 4 * math.sqrt(var_off / (n * 64))        # (and the same light: the means agree)


# ---- the fixture
def test_fixture_meets_its_conditions(rtc):
    hs = mb.mix(rtc)
    assert os.path.getsize(mb.EMITTERS_MIX) < 8192
    scene = json.loads(open(mb.EMITTERS_MIX).read())
    assert (scene["camera"]["width"], scene["camera"]["height"]) == (W, H)
    ind = scene["indirect"]
    assert (ind["gain"], ind["bounces"], ind["emitters"]["samples"]) == (0.9, 2, 2)
    assert hs.lights.n_lights == 1 and hs.media()["fog_density"] > 0 and hs.shadow_filters() is not None and hs.environment() is None
    kinds = [next(iter(o["type"])) for o in scene["objects"]]
    assert "group" in kinds and "plane" in kinds and kinds.count("sphere") == 3
    mats = [o["material"] for o in scene["objects"]]
    assert any(m.get("diffuse") == 0.0 and m.get("reflective", 0) > 0 for m in mats)             # the mirror ball
    assert any("shadow-filter" in m and m.get("transparency", 0) > 0 for m in mats)              # the tinted pane
    assert sum("emission" in m for m in mats) == 3                                               # panel, quad, sphere
    rows, cdf = rtc.diag_emitters(hs.desc, hs.indirect()["emission"], hs.shadow_filters()["rgb"])
    assert len(cdf) == 8
    # (the panel is at least 0.5 from every diffuse surface: the ceiling's lower face is at y = 4, the panel's upper at 3.42)
    panel_top = max(rows[k, 1] + max(0.0, rows[k, 4]) + max(0.0, rows[k, 7]) for k in range(6))
    assert 4.0 - panel_top >= 0.5
    # (the quad stands rotated in its group: no edge is parallel to an axis)
    assert (np.abs(rows[6, 3:9]) > 1e-3).sum() >= 5
    img, c = mb.scene_of(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    print({k: c[k] for k in mb.EMIT_COUNTERS})
    for k in ("emit_drawn", "emit_skip_cos_x", "emit_walks", "emit_blocked", "emit_suppressed", "ind_emitted", "t_partial"):
        assert c[k] > 0, k
    bare, cb = mb.scene_of(rtc, hs, emitters=None).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    assert not np.array_equal(img, bare) and c["shadow_calls"] == cb["shadow_calls"] + c["emit_walks"] and c["secondary"] == cb["secondary"]
    assert img.std() > 0.05


# ---- documents and build
def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("key = rtc_mix64(seed ^ 0xC0AC29B7C97C50DD)", "(j << 17) | cur.code", "the first entry with cdf[k] > u0 * W",
                 "Y_i = (origin_i + u * eu_i) + v * ev_i", "where cos_x <= 0, cos_e == 0 or r <= 2e-4", "0 <= t < r - 1e-4",
                 "term.c = (((E.c * q) * ((cos_x * cos_e) / (RTC_PI * r2))) * F.c)",
                 "s.c = s.c + (color.c * material.diffuse) * (gain * (sum.c / samples))", "Nothing counted twice",
                 "+x, -x, +y, -y, +z, -z", "librtc_multi renders without it"):
        assert line in header, line


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 28." in design
    for word in ("rtc_scene_set_emitters", "rtc_render_kernel_emit", "rtc_render_kernel_emit_bigworld", "emitter_kernels", "EmitVisitor",
                 "tests/cpp/emitters_oracle.cpp", "profiles/emitters/disassembly_identity.txt", "emitters_mix.json",
                 "No multiple importance sampling", "librtc_multi"):
        assert word in design, word
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resources rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_render_kernel_emit", "rtc_render_kernel_emit_bigworld"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} | {k['lds_bytes_per_block']} |" in design, name
            assert k["lds_bytes_per_block"] == resources.get("kernels", resources)[name.replace("_emit", "_indir")]["lds_bytes_per_block"]
    for doc, word in (("README.md", "rtc_scene_set_emitters"), ("INTEGRATION.md", "rtc_scene_set_emitters"), ("INTEGRATION.md", "RtcEmitters"),
                      (os.path.join("tools", "README.md"), "--emitters"), (os.path.join("profiles", "HISTORY.md"), "emitter sampling")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)


def test_object_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "emitters", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_kernels_ext.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o",
                "rtc_occlusion.o", "rtc_shadowfilter.o", "rtc_media.o", "rtc_environment.o", "rtc_skylight.o", "rtc_indirect.o", "rtc_accum.o",
                "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_emit", "rtc_render_kernel_emit_bigworld"):
        assert kernel in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_emitters.o", "rtc_emitters.remarks", "libemitters_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_emitters.hip")).read()
    for word in ("#define RTC_EMIT_TU", "#define RTC_INDIR_TU", "#define RTC_SKYL_TU", "#define RTC_ENV_TU", "#define RTC_MEDIA_TU",
                 "#define RTC_SFILT_TU", "#define RTC_OCCL_TU", "#define RTC_GLOSS_TU", "#define RTC_MESHUV_TU", "#define RTC_TORUS_TU",
                 '#include "rtc_kernels.hip"'):
        assert word in unit, word
    kernels = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_kernels.hip")).read()
    assert "static_assert(!EMIT || INDIRECT" in kernels and "static_assert(!EMIT || !COOP" in kernels
    assert kernels.count("trace<CSG, WORLD, EmitVisitor") == 1      # (the one walk of the suns' loop: no call site of its own)
    host = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_host_internal.h")).read()
    assert "kFamilyEmit" in host and "f == kFamilyEmit" in host
