"""Normal perturbation without a GPU: the ABI of rtc_scene_set_bumps and its validation, the loader's
"normal-perturbation" and rtch_scene_bumps, the two fields at points whose answer is derivable by hand, the shading
normal's length, and the checker (tests/cpp/bump_oracle.cpp) against the spot checker it stacks on."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bump_binding as bb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT_MIX = os.path.join(REPO, "tests", "golden", "spot_scenes", "spot_mix.json")
SCENES = os.path.join(REPO, "tests", "golden", "scenes")
SENTINEL = 1 << 16
NONE, NOISE, RIPPLES = 0, 1, 2


def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def _one(rtc, kind=NOISE, amplitude=0.2, octaves=3, persistence=0.8, inverse=None):
    b = rtc.no_bumps(1)
    b["kind"][0], b["amplitude"][0], b["octaves"][0], b["persistence"][0] = kind, amplitude, octaves, persistence
    if inverse is not None:
        b["inverse"][0] = inverse
    return b


# ---- the symbols
def test_symbols_are_exported(rtc):
    assert "rtc_scene_set_bumps" in rtc.RTC_SYMBOLS
    assert "rtch_scene_bumps" in rtc.HOST_SYMBOLS
    assert rtc.hip_lib().rtc_scene_set_bumps is not None
    assert rtc.host_lib().rtch_scene_bumps is not None
    assert C.sizeof(rtc.Bump) == 48
    assert [rtc.Bump.kind.offset, rtc.Bump.amplitude.offset, rtc.Bump.octaves.offset, rtc.Bump.persistence.offset,
            rtc.Bump.inverse.offset] == [8, 16, 24, 32, 40]
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_bumps(rtc_scene *scene, const rtc_bump *bumps);" in text
    assert "#define RTC_ABI_VERSION 3u" in text   # (the description and the ABI version stay as they were)
    assert f"#define RTC_BUMP_MAX_OCTAVES {rtc.BUMP_MAX_OCTAVES}u" in text
    assert "takes the unperturbed branch" in text


# ---- rtc_scene_set_bumps: refused before anything changes
def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    b, _keep = rtc.bump_struct(_one(rtc))
    assert _status(lib, lib.rtc_scene_set_bumps(None, C.byref(b))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_bumps(None, None)) == "InvalidArgument"


def _bad_matrix(v):
    m = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    m[7] = v
    return m


@pytest.mark.parametrize("kw, words", [
    ({"kind": 3}, "kind"),
    ({"kind": 255}, "kind"),
    ({"amplitude": np.nan}, "not finite"),
    ({"amplitude": np.inf}, "not finite"),
    ({"amplitude": -1e-300}, "below 0"),
    ({"kind": RIPPLES, "amplitude": -1.0}, "below 0"),
    ({"octaves": 0}, "octaves"),
    ({"octaves": 17}, "octaves"),
    ({"persistence": np.nan}, "not finite"),
    ({"persistence": -np.inf}, "not finite"),
    ({"inverse": _bad_matrix(np.nan)}, "matrix"),
    ({"kind": RIPPLES, "inverse": _bad_matrix(np.inf)}, "matrix"),
], ids=["kind3", "kind255", "nan-amp", "inf-amp", "neg-amp", "neg-amp-ripples", "octaves0", "octaves17", "nan-persistence",
        "inf-persistence", "nan-matrix", "inf-matrix"])
def test_setter_rejects_an_invalid_entry_and_touches_nothing(rtc, kw, words):
    """The table's own values are checked before its count against the handle: the stand-in's material count reads as
    0xA5A5A5A5, so each of these is refused for its own reason."""
    lib = rtc.hip_lib()
    handle = _stand_in()
    b, _keep = rtc.bump_struct(_one(rtc, **kw))
    st = lib.rtc_scene_set_bumps(C.cast(handle, C.c_void_p), C.byref(b))
    assert _status(lib, st) == "InvalidArgument"
    assert words in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


@pytest.mark.parametrize("n", [0, 1, 7])
def test_setter_rejects_a_wrong_material_count_and_touches_nothing(rtc, n):
    lib = rtc.hip_lib()
    handle = _stand_in()
    bumps = rtc.no_bumps(n)
    bumps["kind"][:] = RIPPLES
    bumps["amplitude"][:] = 0.1
    b, _keep = rtc.bump_struct(bumps)
    st = lib.rtc_scene_set_bumps(C.cast(handle, C.c_void_p), C.byref(b))
    assert _status(lib, st) == "InvalidArgument"
    assert "n_materials" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


def test_bump_kernels_is_an_option(rtc):
    rtc.set_option("bump_kernels", 1)
    rtc.set_option("bump_kernels", 0)


# ---- the fields: values derivable by hand
def test_ripples_by_hand():
    # r = 0.25: v = 2 * 0.25 - 1 = -0.5, h = (4 * -0.5) * (1 - 0.5) = -1, d = h * (q.x / r, 0, q.z / r) = (-1, 0, 0); q.y is not read
    assert np.array_equal(bb.field(RIPPLES, [0.25, 7.0, 0.0]), [-1.0, 0.0, 0.0])
    assert np.array_equal(bb.field(RIPPLES, [0.0, -3.0, 0.75]), [0.0, 0.0, 1.0])   # v = 0.5, h = 2 * 0.5 = 1
    for q in ([0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, -2.0], [3.0, 1.0, 4.0]):   # (r = 5)
        assert np.all(bb.field(RIPPLES, q) == 0.0), q


def test_ripples_are_continuous_across_the_seam():
    below, at = bb.field(RIPPLES, [1.0 - 2.0 ** -40, 0.0, 0.0]), bb.field(RIPPLES, [1.0, 0.0, 0.0])
    # v = 1 - 2^-39 below the seam: h = 4 v (1 - v) = 4 (1 - 2^-39) 2^-39, within 2^-36 of the seam's 0
    assert at[0] == 0.0 and 0.0 < below[0] <= 2.0 ** -36
    assert below[0] == (4.0 * (1.0 - 2.0 ** -39)) * 2.0 ** -39
    above = bb.field(RIPPLES, [1.0 + 2.0 ** -40, 0.0, 0.0])
    assert -2.0 ** -36 <= above[0] < 0.0


def test_ripples_match_a_restatement_bitwise():
    rng = np.random.default_rng(17)
    for q in rng.uniform(-6, 6, (2000, 3)):
        x, z = np.float64(q[0]), np.float64(q[2])
        r = np.sqrt(x * x + z * z)
        v = np.float64(2.0) * (r - np.floor(r)) - np.float64(1.0)
        h = (np.float64(4.0) * v) * (np.float64(1.0) - np.abs(v))
        assert np.array_equal(bb.field(RIPPLES, q), [h * (x / r), 0.0, h * (z / r)])


def test_noise_is_the_oracles_three_octave_noise_calls():
    rng = np.random.default_rng(18)
    for q in list(rng.uniform(-9, 9, (300, 3))) + [[0.0, 0.0, 0.0], [255.5, -256.0, 1e6], [-0.0, 1.0, -1.0]]:
        for octaves, persistence in ((3, 0.8), (1, 0.3), (16, 1.0), (5, -0.5)):
            d = bb.field(NOISE, q, octaves, persistence)
            assert np.array_equal(d, bb.octave_noise3(q, octaves, persistence)), (q, octaves, persistence)
    assert np.all(bb.field(NONE, [0.3, 0.4, 0.5]) == 0.0)
    assert np.any(bb.field(NOISE, [0.3, 0.4, 0.5]) != 0.0)


# ---- the shading normal
def test_shading_normal_is_unit_length():
    rng = np.random.default_rng(19)
    worst = 0.0
    for i in range(600):
        ln = rng.uniform(-2, 2, 3)
        lp = rng.uniform(-3, 3, 3)
        inv_t = np.eye(4)
        inv_t[:3, :3] = rng.uniform(-2, 2, (3, 3))
        kind = NOISE if i % 2 else RIPPLES
        ns = bb.normal(ln, lp, kind, rng.uniform(0.01, 1.5), inverse=None, inv_t=inv_t.ravel(), inside=bool(i % 3 == 0))
        worst = max(worst, abs(float(np.sqrt(ns @ ns)) - 1.0))
    assert worst <= 1e-15, worst


def test_shading_normal_by_hand():
    # ln = (0, 2, 0) -> u = (0, 1, 0); ripples at lp = (0.25, 9, 0): d = (-1, 0, 0); amplitude 1: ln' = (-1, 1, 0)
    ns = bb.normal([0.0, 2.0, 0.0], [0.25, 9.0, 0.0], RIPPLES, 1.0)
    s = 1.0 / np.sqrt(2.0)
    assert np.allclose(ns, [-s, s, 0.0], rtol=0, atol=1e-16)
    assert np.array_equal(bb.normal([0.0, 2.0, 0.0], [0.25, 9.0, 0.0], RIPPLES, 1.0, inside=True), -ns)
    # B scales the field's space: q = 0.5 * lp
    B = [0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0.5, 0]
    assert np.array_equal(bb.normal([0.0, 2.0, 0.0], [0.5, 9.0, 0.0], RIPPLES, 1.0, inverse=B), ns)
    # the unperturbed branch: kind none, amplitude 0 and |ln| == 0 give ng, bit for bit
    ln, lp = [0.3, -0.7, 0.2], [0.11, 0.23, 0.37]
    ng = bb.normal(ln, lp, NONE, 0.5)
    assert np.array_equal(bb.normal(ln, lp, NOISE, 0.0), ng) and np.array_equal(bb.normal(ln, lp, RIPPLES, 0.0), ng)
    assert np.array_equal(bb.normal([0.0, 0.0, 0.0], lp, NOISE, 0.5), [0.0, 0.0, 0.0])
    assert not np.array_equal(bb.normal(ln, lp, NOISE, 0.5), ng)


# ---- the checker against the spot checker it stacks on
def _strip(text):
    scene = json.loads(text)
    for o in scene["objects"]:
        o.get("material", {}).pop("normal-perturbation", None)
    return json.dumps(scene)


def test_no_bump_is_the_spot_checker_bit_for_bit(rtc):
    stripped = rtc.HostScene(_strip(open(bb.BUMP_MIX).read()), bb.BUMP_DIR)
    assert stripped.bumps() is None
    for hs in (stripped, rtc.HostScene.from_file(SPOT_MIX)):
        cam = hs.camera(48, 27)
        n = hs.desc.n_materials
        zero_amp = rtc.no_bumps(n)
        zero_amp["kind"][:] = [NOISE, RIPPLES][0:1] * n
        zero_amp["kind"][::2] = RIPPLES
        want, wc = bb.BumpScene(hs.desc, hs.lights).render_spot(cam, 5, spots=hs.spots(), light_seed=3)
        for bumps in (None, rtc.no_bumps(n), zero_amp):
            got, gc = bb.BumpScene(hs.desc, hs.lights, bumps).render(cam, 5, spots=hs.spots(), light_seed=3)
            assert np.array_equal(got, want) and gc == wc


def test_bumps_change_the_image_and_not_the_primary_rays(rtc):
    hs = bb.mix(rtc)
    cam = hs.camera(48, 27)
    flat, fc = bb.BumpScene(hs.desc, hs.lights).render(cam, 5, spots=hs.spots())
    bumped, bc = bb.BumpScene(hs.desc, hs.lights, hs.bumps()).render(cam, 5, spots=hs.spots())
    assert fc["primary"] == bc["primary"] == 48 * 27
    assert (np.abs(flat - bumped).max(axis=2) > 1e-3).mean() > 0.3


def test_geometric_decisions_of_a_bumped_glass_sphere_are_unchanged(rtc):
    glass = {"type": {"sphere": {}}, "material": {"transparency": 0.9, "reflective": 0.5, "refractive-index": 1.5,
                                                   "normal-perturbation": {"type": "noise", "amplitude": 0.4,
                                                                           "transform": [{"scale": [0.2, 0.2, 0.2]}]}}}
    inner = {"type": {"sphere": {}}, "transform": [{"scale": [0.5, 0.5, 0.5]}], "material": {"transparency": 1.0, "refractive-index": 2.0}}
    cam = {"width": 8, "height": 8, "field-of-view": 1.0, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]}
    text = json.dumps({"camera": cam, "lights": [{"point-light": {"position": [-5, 5, -5], "intensity": [1, 1, 1]}}], "objects": [glass, inner]})
    hs = rtc.HostScene(text)
    bumps = hs.bumps()
    assert bumps is not None and list(bumps["kind"]) == [NOISE, NONE]
    plain, bumped = bb.BumpScene(hs.desc, hs.lights), bb.BumpScene(hs.desc, hs.lights, bumps)
    rng = np.random.default_rng(20)
    changed = 0
    rays = [([0.0, 0.0, -5.0], [0.0, 0.0, 1.0]), ([0.0, 0.0, 0.75], [0.0, 0.0, 1.0]), ([0.0, 0.0, 0.0], [0.0, 1.0, 0.0])]
    for _ in range(200):
        o = rng.uniform(-0.95, 0.95, 3) * rng.choice([1.0, 4.0])
        d = rng.normal(size=3) if np.linalg.norm(o) < 1.0 else -o + rng.uniform(-0.5, 0.5, 3)
        rays.append((o, d / np.linalg.norm(d)))
    for o, d in rays:
        a, b = plain.comps(o, d), bumped.comps(o, d)
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert a["inside"] == b["inside"]
        for k in ("over_point", "under_point"):
            assert np.array_equal(a[k], b[k]), k
        assert a["n1"] == b["n1"] and a["n2"] == b["n2"]
        changed += int(not np.array_equal(a["normal"], b["normal"]))
        assert abs(float(np.sqrt(b["normal"] @ b["normal"])) - 1.0) <= 1e-15
    assert changed > 100   # (hits on the inner, un-bumped sphere keep their normal)


# ---- the loader
def _scene(material):
    cam = {"width": 40, "height": 20, "field-of-view": 1.0, "from": [0, 1.5, -5], "to": [0, 1, 0], "up": [0, 1, 0]}
    return json.dumps({"camera": cam, "lights": [{"point-light": {"position": [0, 4, 0], "intensity": [1, 1, 1]}}],
                       "objects": [{"type": {"plane": {}}, "material": material}]})


def _np(**kw):
    cfg = {"type": "noise", "amplitude": 0.2}
    cfg.update(kw)
    return {"normal-perturbation": {k: v for k, v in cfg.items() if v is not None}}


def test_loader_reads_the_fixture(rtc):
    hs = bb.mix(rtc)
    b = hs.bumps()
    assert hs.desc.n_materials == 7
    assert list(b["kind"]) == [RIPPLES, NOISE, NOISE, RIPPLES, NOISE, NOISE, NONE]
    assert list(b["amplitude"]) == [0.12, 0.35, 0.15, 0.2, 0.25, 0.3, 0.0]
    assert list(b["octaves"]) == [3, 3, 2, 3, 4, 3, 3]
    assert list(b["persistence"]) == [0.8, 0.8, 0.5, 0.8, 0.8, 0.8, 0.8]
    # the plane's field: scale 0.4 then translate (0.3, 0, 1) -> the inverse scales by 2.5 after shifting back
    assert np.allclose(b["inverse"][0], [2.5, 0, 0, -0.75, 0, 2.5, 0, 0, 0, 0, 2.5, -2.5], rtol=0, atol=1e-15)
    assert np.array_equal(b["inverse"][6], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    # both triangles of the OBJ group share the group's bumped material row
    kinds = [hs.desc.leaf_kind[i] for i in range(hs.desc.n_leaves)]
    tri = [i for i, k in enumerate(kinds) if k == 5]
    assert len(tri) == 2 and {hs.desc.leaf_material[i] for i in tri} == {5}


def test_loader_round_trips_every_field(rtc):
    hs = rtc.HostScene(_scene(_np(type="noise", amplitude=0.0625, octaves=16, persistence=-0.25, transform=[{"translate": [1, 2, 3]}])))
    b = hs.bumps()
    assert (b["kind"][0], b["amplitude"][0], b["octaves"][0], b["persistence"][0]) == (NOISE, 0.0625, 16, -0.25)
    assert np.array_equal(b["inverse"][0], [1, 0, 0, -1, 0, 1, 0, -2, 0, 0, 1, -3])
    b = rtc.HostScene(_scene(_np(type="ripples", amplitude=0))).bumps()
    assert (b["kind"][0], b["amplitude"][0]) == (RIPPLES, 0.0)


def test_a_bumped_material_is_a_row_of_its_own(rtc):
    plain = {"diffuse": 0.7}
    objects = [{"type": {"sphere": {}}, "material": plain}, {"type": {"cube": {}}, "material": dict(plain, **_np())},
               {"type": {"plane": {}}, "material": plain}, {"type": {"cone": {}}, "material": dict(plain, **_np())}]
    scene = json.loads(_scene(plain))
    scene["objects"] = objects
    hs = rtc.HostScene(json.dumps(scene))
    assert hs.desc.n_materials == 2
    assert [hs.desc.leaf_material[i] for i in range(4)] == [0, 1, 0, 1]
    assert list(hs.bumps()["kind"]) == [NONE, NOISE]


def test_loader_without_the_key_has_none(rtc):
    assert rtc.HostScene(_scene({"diffuse": 0.5})).bumps() is None


@pytest.mark.parametrize("kw, key", [
    ({"type": None}, "normal-perturbation.type"),
    ({"type": "waves"}, "normal-perturbation.type.waves"),
    ({"type": 3}, "normal-perturbation.type"),
    ({"amplitude": None}, "normal-perturbation.amplitude"),
    ({"amplitude": -0.1}, "normal-perturbation.amplitude"),
    ({"amplitude": "big"}, "normal-perturbation.amplitude"),
    ({"octaves": 0}, "normal-perturbation.octaves"),
    ({"octaves": 17}, "normal-perturbation.octaves"),
    ({"octaves": 2.5}, "normal-perturbation.octaves"),
    ({"type": "ripples", "octaves": 3}, "normal-perturbation.octaves"),
    ({"type": "ripples", "persistence": 0.5}, "normal-perturbation.persistence"),
    ({"persistence": [1]}, "normal-perturbation.persistence"),
    ({"transform": [{"scale": [0, 1, 1]}]}, "normal-perturbation.transform"),
    ({"wavelength": 2}, "normal-perturbation.wavelength"),
], ids=["no-type", "unknown-type", "type-number", "no-amplitude", "neg-amplitude", "amplitude-string", "octaves0", "octaves17",
        "octaves-fraction", "ripples-octaves", "ripples-persistence", "persistence-list", "singular-transform", "unknown-field"])
def test_loader_refuses_a_malformed_entry(rtc, kw, key):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(_np(**kw)))
    assert key in str(e.value)


def test_loader_refuses_an_entry_that_is_no_object(rtc):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene({"normal-perturbation": "noise"}))
    assert "normal-perturbation" in str(e.value)


def test_host_bumps_needs_the_material_count(rtc):
    hs = bb.mix(rtc)
    b = rtc.no_bumps(5)
    dp = C.POINTER(C.c_double)
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_bumps(hs._h, b["kind"].ctypes.data_as(C.POINTER(C.c_uint8)), b["amplitude"].ctypes.data_as(dp),
                                                         b["octaves"].ctypes.data_as(C.POINTER(C.c_uint32)), b["persistence"].ctypes.data_as(dp),
                                                         b["inverse"].ctypes.data_as(dp), 5))


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(SCENES) if f.endswith(".json")))
def test_existing_scenes_load_without_bumps_and_split_no_material_row(rtc, name):
    """A scene without the key loads to the tables it had: no bump, and no two material rows alike - the new part of the
    row's key is empty.  (The tables themselves are held to the oracle's own scene build by tests/test_oracle_scene_cpu.py.)"""
    hs = rtc.HostScene.from_file(name)
    assert hs.bumps() is None
    d = hs.desc
    rows = {(tuple(d.mat_params[7 * i + k] for k in range(7)), d.mat_pattern[i]) for i in range(d.n_materials)}
    assert len(rows) == d.n_materials
