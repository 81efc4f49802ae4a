"""Area lights (the book's bonus chapter "Rendering soft shadows") without a GPU: the checker against the book's
vectors and an independent restatement of the jitter, the loader's "area-light", the ABI of rtc_light_desc and
rtc_scene_create_with_lights' validation, and the point-light scenes' tables, which must not move."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

import area_binding as ab

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")
# (beside the point-light scenes, not among them: the oracle's own scene parser, which every scene there is checked
# against, knows point lights only)
SOFT_SHADOWS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "area_scenes", "soft_shadows.json")


# ---- the book's vectors on the checker
def test_point_on_light_book_vectors():
    uvs = [(0, 0), (1, 0), (0, 1), (2, 0), (3, 1)]
    got = ab.point_on_light((0, 0, 0), (2, 0, 0), 4, (0, 0, 1), 2, uvs)
    assert np.allclose(got, [(0.25, 0, 0.25), (0.75, 0, 0.25), (0.25, 0, 0.75), (1.25, 0, 0.25), (1.75, 0, 0.75)], atol=1e-12)
    got = ab.point_on_light((0, 0, 0), (2, 0, 0), 4, (0, 0, 1), 2, uvs, seq=(0.3, 0.7))
    assert np.allclose(got, [(0.15, 0, 0.35), (0.65, 0, 0.35), (0.15, 0, 0.85), (1.15, 0, 0.35), (1.65, 0, 0.85)], atol=1e-12)


def test_area_light_fields():
    _, info = ab.intensity_at((0, 0, 0), (2, 0, 0), 4, (0, 0, 1), 2, [(0, 0, 0)])
    assert np.allclose(info[0:3], (0.5, 0, 0)) and np.allclose(info[3:6], (0, 0, 0.5))
    assert info[6] == 8 and np.allclose(info[7:10], (1, 0, 0.5))


POINTS = [(0, 0, 2), (1, -1, 2), (1.5, 0, 2), (1.25, 1.25, 3), (0, 0, -2)]
LIGHT = ((-0.5, -0.5, -5), (1, 0, 0), 2, (0, 1, 0), 2)


def test_intensity_at_book_vectors():
    got, _ = ab.intensity_at(*LIGHT, POINTS)
    assert list(got) == [0.0, 0.25, 0.5, 0.75, 1.0]


def test_intensity_at_jittered_book_vectors():
    seq = (0.7, 0.3, 0.9, 0.1, 0.5)
    got = [ab.intensity_at(*LIGHT, [p], seq=seq)[0][0] for p in POINTS]   # (a fresh sequence per point, as the book)
    assert got == [0.0, 0.5, 0.75, 0.75, 1.0]


@pytest.mark.parametrize("pt, want", [((0, 0, -1), 0.9965), ((0, 0.7071, -0.7071), 0.6232)])
def test_lighting_samples_the_area_light(pt, want):
    pt = np.array(pt, dtype=np.float64)
    eyev = np.array((0, 0, -5.0)) - pt
    eyev /= np.linalg.norm(eyev)
    got = ab.lighting(*LIGHT, (0.1, 0.9, 0.0, 200.0), pt, eyev, pt, 1.0)
    assert np.allclose(got, want, atol=1e-4)


def _mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def test_jitter_matches_independent_restatement():
    rng = np.random.default_rng(7)
    n = 100_000
    seed = int(rng.integers(0, 2**63))
    p = rng.integers(0, 3840 * 2160, n, dtype=np.uint64)
    nl = rng.integers(1, 65, n, dtype=np.uint64)
    l = (rng.integers(0, 2**32, n, dtype=np.uint64) % nl).astype(np.uint64)
    k = rng.integers(0, 4096, n, dtype=np.uint64)
    axis = rng.integers(0, 2, n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        c = ((p * nl + l) << np.uint64(32)) | (np.uint64(2) * k + axis)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (c + np.uint64(1))
        want = (_mix(z) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    got = ab.jitter(seed, p, nl, l, k, axis)
    assert np.array_equal(got, want)
    assert got.min() >= 0.0 and got.max() < 1.0


# ---- the loader
def _scene(lights):
    return json.dumps({"camera": {"width": 8, "height": 8, "field-of-view": 1.0, "from": [0, 1, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
                       "lights": lights, "objects": [{"type": {"sphere": {}}}]})


AREA = {"corner": [-1, 2, 4], "uvec": [2, 0, 0], "usteps": 4, "vvec": [0, 2, 0], "vsteps": 2, "intensity": [1.5, 1, 0.5], "jitter": True}


def test_loader_area_light(rtc):
    hs = rtc.HostScene(_scene([{"point-light": {"position": [1, 2, 3], "intensity": [0.1, 0.2, 0.3]}}, {"area-light": AREA},
                               {"point-light": {"position": [4, 5, 6], "intensity": [1, 1, 1]}}]))
    got = hs.lights.to_list()
    assert [l["kind"] for l in got] == ["point", "area", "point"]
    assert got[0] == {"kind": "point", "position": [1, 2, 3], "intensity": [0.1, 0.2, 0.3]}
    assert got[1] == {"kind": "area", "corner": [-1, 2, 4], "uvec": [2, 0, 0], "usteps": 4, "vvec": [0, 2, 0], "vsteps": 2,
                      "intensity": [1.5, 1, 0.5], "jitter": True}
    # the description's point tables: every light, an area light at its centre
    d = hs.desc
    assert d.n_lights == 3
    assert hs.array("light_pos", 3, 3).tolist() == [[1, 2, 3], [0, 3, 4], [4, 5, 6]]
    assert hs.array("light_rgb", 3, 3).tolist() == [[0.1, 0.2, 0.3], [1.5, 1, 0.5], [1, 1, 1]]


def test_loader_jitter_defaults_to_false(rtc):
    a = dict(AREA)
    del a["jitter"]
    assert rtc.HostScene(_scene([{"area-light": a}])).lights.to_list()[0]["jitter"] is False


@pytest.mark.parametrize("patch, name", [({"usteps": 0}, "InvalidData"), ({"vsteps": 0}, "InvalidData"),
                                         ({"usteps": 64, "vsteps": 65}, "Overflow"), ({"colour": 1}, "UnknownField"),
                                         ({"usteps": 1.5}, "InvalidNumber"), ({"jitter": 1}, "UnexpectedToken")])
def test_loader_area_light_errors(rtc, patch, name):
    a = dict(AREA, **patch)
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene([{"area-light": a}]))
    assert name in str(e.value)


@pytest.mark.parametrize("field", ["corner", "uvec", "usteps", "vvec", "vsteps", "intensity"])
def test_loader_area_light_missing_field(rtc, field):
    a = dict(AREA)
    del a[field]
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene([{"area-light": a}]))
    assert "MissingField" in str(e.value)


def test_loader_still_rejects_other_lights(rtc):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene([{"spot-light": {"position": [0, 0, 0]}}]))
    assert "UnknownField" in str(e.value)


def test_soft_shadows_fixture_loads(rtc):
    hs = rtc.HostScene.from_file(SOFT_SHADOWS)
    kinds = [l["kind"] for l in hs.lights.to_list()]
    assert kinds == ["area", "point"]
    assert hs.lights.to_list()[0]["usteps"] == 8 and hs.lights.to_list()[0]["jitter"] is True


# ---- no change to existing scenes: the device tables of every point-light scene, as recorded before area lights
BASE_DIGESTS = {
    "align_check.json": 18069515568222499371, "cover.json": 8942883067295429542, "csg.json": 7472645214263732982,
    "csg_demo.json": 1724942778668725884, "cubes.json": 14000193164708276444, "cylinders.json": 15774039831044925997,
    "dragons.json": 83576001087836655, "earth.json": 3409342367359203742, "fresnel.json": 10927649611100110560,
    "groups.json": 12477662965686356942, "nefertiti.json": 8395596333052403036, "perturb_demo.json": 120839023025213995,
    "reflection_and_refraction.json": 2936459831550145267, "skybox_demo.json": 16409752444319606926,
    "teapot.json": 15411699231746449331, "texture_demo.json": 10805373410918848971, "xyz.json": 9212859777150946457,
}


@pytest.mark.parametrize("name", sorted(BASE_DIGESTS))
def test_point_light_scenes_build_the_same_tables(rtc, name):
    hs = rtc.HostScene.from_file(name)
    assert rtc.build_tables_digest(hs.desc)[0] == BASE_DIGESTS[name]
    assert all(l["kind"] == "point" for l in hs.lights.to_list())


# ---- ABI
def test_light_desc_layout(rtc):
    L = rtc.LightDesc
    P = C.sizeof(C.c_void_p)
    assert [(n, getattr(L, n).offset) for n, _ in L._fields_] == [
        ("n_lights", 0), ("kind", P), ("corner", 2 * P), ("uvec", 3 * P), ("vvec", 4 * P), ("usteps", 5 * P),
        ("vsteps", 6 * P), ("jitter", 7 * P), ("rgb", 8 * P)]
    assert C.sizeof(L) == 9 * P
    header = open(os.path.join(os.path.dirname(SCENES), "..", "..", "include", "rtc.h")).read()
    body = header[header.index("typedef struct rtc_light_desc"):header.index("} rtc_light_desc;")]
    names = [line.split(";")[0].replace("*", " ").split()[-1] for line in body.splitlines()[1:] if ";" in line]
    assert [n for n, _ in L._fields_] == names
    for sym in ("rtc_scene_create_with_lights", "rtc_scene_set_light_seed"):
        assert sym in rtc.RTC_SYMBOLS
        getattr(rtc.hip_lib(), sym)
    assert "rtch_scene_lights" in rtc.HOST_SYMBOLS


def test_create_with_lights_rejects_bad_tables_without_gpu(rtc):
    """Validation of the light table runs on the host before any HIP call."""
    hs = rtc.HostScene.from_file("fresnel.json")
    lib = rtc.hip_lib()
    out = C.c_void_p()
    good = dict(kind="area", corner=(-1, 2, 4), uvec=(2, 0, 0), usteps=4, vvec=(0, 2, 0), vsteps=4, intensity=(1, 1, 1), jitter=True)

    def status(**patch):
        t = rtc.LightDesc.make([dict(good, **patch)])
        return lib.rtc_scene_create_with_lights(C.byref(hs.desc), C.byref(t), C.byref(out)), lib.rtc_last_error()

    assert status(usteps=0) == (1, status(usteps=0)[1]) and b"InvalidArgument" in status(usteps=0)[1]
    assert status(vsteps=0)[0] == 1
    assert status(usteps=64, vsteps=65)[0] == 1
    assert status(corner=(float("nan"), 0, 0))[0] == 1
    assert status(uvec=(float("inf"), 0, 0))[0] == 1
    assert status(intensity=(1, float("nan"), 1))[0] == 1
    t = rtc.LightDesc.make([good])
    t.kind[0] = 7
    assert lib.rtc_scene_create_with_lights(C.byref(hs.desc), C.byref(t), C.byref(out)) == 4
    assert b"Unsupported" in lib.rtc_last_error()
    assert not out.value
