"""Glossy reflection and refraction without a GPU: the sampler, the hash and the child direction of
the checker (tests/cpp/gloss_oracle.cpp) against restatements in Python, the null cases against the mesh-texture checker it
stacks on, determinism across bands and passes, the statistics of one rough pixel, the loader's "roughness" and
rtch_scene_gloss, and rtc_scene_set_gloss's validation through the ABI."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gloss_binding as gb
import meshuv_binding as mb
import test_torus_cpu as ttc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(REPO, "tests", "golden", "scenes")
SENTINEL = 1 << 16
GOLD = 0x9E3779B97F4A7C15
SALT = 0x13198A2E03707344


# ---- the symbols
def test_symbols_are_exported(rtc):
    assert "rtc_scene_set_gloss" in rtc.RTC_SYMBOLS and "rtch_scene_gloss" in rtc.HOST_SYMBOLS
    assert "gloss_kernels" in rtc.KERNEL_OPTIONS
    assert rtc.hip_lib().rtc_scene_set_gloss is not None and rtc.host_lib().rtch_scene_gloss is not None
    assert C.sizeof(rtc.Gloss) == 32
    assert [rtc.Gloss.reflection.offset, rtc.Gloss.transmission.offset, rtc.Gloss.seed.offset] == [8, 16, 24]
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_gloss(rtc_scene *scene, const rtc_gloss *gloss);" in text
    assert "#define RTC_ABI_VERSION 3u" in text   # (the description and the ABI version stay as they were)
    rtc.set_option("gloss_kernels", 1)
    rtc.set_option("gloss_kernels", 0)


# ---- the sampler
def _sampler_py(draws):
    """rtc.h's rule in Python floats (IEEE doubles, one rounding an operation)"""
    for t in range(32):
        a, b, c = (2.0 * float(draws[3 * t + i]) - 1.0 for i in range(3))
        if ((a * a) + (b * b)) + (c * c) <= 1.0:
            return [a, b, c]
    return [0.0, 0.0, 0.0]


def test_sampler_matches_a_restatement_bitwise():
    draws = np.random.default_rng(11).random((500, 96))
    got = gb.sampler(draws)
    want = np.array([_sampler_py(d) for d in draws])
    assert np.array_equal(got, want)
    assert ((got ** 2).sum(axis=1) <= 1.0 + 1e-15).all()
    # the first accepted triple is not always the first triple: some sets reject at least once
    first = 2.0 * draws[:, :3] - 1.0
    assert ((first ** 2).sum(axis=1) > 1.0).any() and (got != first).any()


def test_sampler_without_an_accepted_triple_is_zero():
    corner = np.full((1, 96), 0.99)                 # every triple (0.98, 0.98, 0.98): outside the ball
    assert np.array_equal(gb.sampler(corner), np.zeros((1, 3)))
    last = corner.copy()
    last[0, 93:96] = (0.5, 0.75, 0.25)              # ... but the 32nd
    assert np.array_equal(gb.sampler(last), np.array([[0.0, 0.5, -0.5]]))
    edge = np.full((1, 96), 0.99)
    edge[0, 0:3] = (1.0 - 2.0 ** -53, 0.5, 0.5)    # (a, b, c) = (1 - 2^-52, 0, 0): inside, by <=
    assert np.array_equal(gb.sampler(edge), np.array([[1.0 - 2.0 ** -52, 0.0, 0.0]]))


# ---- J
def _mix64(z):
    z = z.copy()
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _jitter_np(seed, p, g, code, axis):
    with np.errstate(over="ignore"):
        u = np.uint64
        key = _mix64(np.array([seed ^ SALT], dtype=u))[0]
        h = _mix64(key + u(GOLD) * (((p << u(32)) | (g << u(8))) + u(1)))
        z = _mix64(h + u(GOLD) * (((code << u(8)) | axis) + u(1)))
        return (z >> u(11)).astype(np.float64) * 2.0 ** -53


def test_jitter_matches_a_numpy_restatement_bitwise():
    rng = np.random.default_rng(3)
    n = 4000
    p = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    g = rng.integers(0, 1 << 24, n, dtype=np.uint64)
    code = rng.integers(1, 1 << 17, n, dtype=np.uint64)
    axis = rng.integers(0, 96, n, dtype=np.uint64)
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        got = gb.jitter(seed, p, g, code, axis)
        assert np.array_equal(got, _jitter_np(seed, p, g, code, axis))
        assert got.min() >= 0.0 and got.max() < 1.0
        assert abs(got.mean() - 0.5) < 0.02           # (sigma of the mean of 4000 uniforms: 0.0046)
    # every argument matters
    base = gb.jitter(5, [7], [3], [2], [0])[0]
    for other in (gb.jitter(6, [7], [3], [2], [0]), gb.jitter(5, [8], [3], [2], [0]), gb.jitter(5, [7], [4], [2], [0]),
                  gb.jitter(5, [7], [3], [3], [0]), gb.jitter(5, [7], [3], [2], [1])):
        assert other[0] != base


# ---- the child direction
def _draws_for(s):
    """96 draws whose first triple maps to s"""
    d = np.full(96, 0.99)
    d[:3] = (np.asarray(s) + 1.0) / 2.0
    return d


def test_child_direction_is_a_unit_vector():
    rng = np.random.default_rng(8)
    worst = 0.0
    for _ in range(300):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        ng = rng.normal(size=3)
        ng /= np.linalg.norm(ng)
        out, used = gb.child(d, ng, rng.random(), rng.random(96), below=bool(rng.integers(2)))
        worst = max(worst, abs(float(np.sqrt((out * out).sum())) - 1.0))
        if not used:
            assert np.array_equal(out, d)
    assert worst <= 1e-15


def test_side_rule_by_hand():
    ng = [0.0, 1.0, 0.0]
    d = np.array([0.6, 0.8, 0.0])
    # s = (0, -0.5, 0) at roughness 1: e = (0.6, 0.3, 0), above the surface: used
    out, used = gb.child(d, ng, 1.0, _draws_for([0.0, -0.5, 0.0]))
    m = np.sqrt((0.6 * 0.6 + (0.8 + -0.5 * 1.0) * (0.8 + -0.5 * 1.0)) + 0.0)
    assert used and np.array_equal(out, np.array([0.6 / m, (0.8 + -0.5 * 1.0) / m, 0.0 / m]))
    # a grazing d and a draw that pushes it just below the surface: d stays
    graze = np.array([np.sqrt(1.0 - 1e-6), 1e-3, 0.0])
    out, used = gb.child(graze, ng, 1.0, _draws_for([0.0, -0.0011, 0.0]))
    assert not used and np.array_equal(out, graze)
    # ... exactly on the surface (dot == 0.0) falls back too: the rule is > 0.0
    out, used = gb.child([1.0, 0.5, 0.0], ng, 1.0, _draws_for([0.0, -0.5, 0.0]))
    assert not used and np.array_equal(out, [1.0, 0.5, 0.0])
    # the refracted child's rule is the mirror image: below the surface is used, above falls back
    t = np.array([0.6, -0.8, 0.0])
    out, used = gb.child(t, ng, 1.0, _draws_for([0.0, 0.5, 0.0]), below=True)
    assert used and out[1] < 0.0
    out, used = gb.child(t, ng, 1.0, _draws_for([0.0, 0.9, 0.0]), below=True)
    assert not used and np.array_equal(out, t)
    # e == 0: d stays
    out, used = gb.child([0.0, 0.5, 0.0], ng, 1.0, _draws_for([0.0, -0.5, 0.0]))
    assert not used and np.array_equal(out, [0.0, 0.5, 0.0])
    # roughness scales s
    out, used = gb.child(d, ng, 0.5, _draws_for([0.5, 0.0, 0.0]))
    m = np.sqrt(((0.6 + 0.5 * 0.5) * (0.6 + 0.5 * 0.5) + 0.8 * 0.8) + 0.0)
    assert used and np.array_equal(out, np.array([(0.6 + 0.5 * 0.5) / m, 0.8 / m, 0.0 / m]))


# ---- the null cases
def _strip(text):
    """gloss_mix.json without the key"""
    scene = json.loads(text)
    for o in scene["objects"]:
        o["material"].pop("roughness", None)
    return json.dumps(scene)


def _checker(hs, gloss):
    return gb.GlossScene(hs.desc, hs.lights, hs.bumps(), hs.mesh_uvs(), gloss)


@pytest.mark.parametrize("which", ["gloss_mix without the key", "mesh_mix"])
def test_no_gloss_is_the_meshuv_checker_bit_for_bit(rtc, which):
    hs = mb.mix(rtc) if which == "mesh_mix" else rtc.HostScene(_strip(open(gb.GLOSS_MIX).read()), gb.GLOSS_DIR)
    assert hs.gloss() is None
    cam = hs.camera(80, 45)
    n = hs.desc.n_materials
    ck = _checker(hs, None)
    want, wc = ck.render_meshuv(cam, 5, spots=hs.spots(), disp=hs.motion(), light_seed=3)
    for gloss in (None, {"reflection": np.zeros(n), "transmission": np.zeros(n), "seed": 9}, {"reflection": np.zeros(n)}):
        ck.set_gloss(gloss)
        got, c = ck.render(cam, 5, spots=hs.spots(), disp=hs.motion(), light_seed=3)
        assert np.array_equal(got, want)
        assert {k: c[k] for k in wc} == wc and c["used"] == 0 and c["fell_back"] == 0


def test_fixture_exercises_both_branches_of_the_side_rule(rtc):
    hs = gb.mix(rtc)
    g = hs.gloss()
    assert g["seed"] == 0 and g["reflection"].max() == 1.0 and np.count_nonzero(g["transmission"]) >= 2
    ck = _checker(hs, g)
    img, c = ck.render(hs.camera(80, 45), 5, spots=hs.spots())
    print(c)
    assert c["used"] > 0 and c["fell_back"] > 0
    ck.set_gloss(None)
    sharp, c0 = ck.render(hs.camera(80, 45), 5, spots=hs.spots())
    assert c0["primary"] == c["primary"] and not np.array_equal(img, sharp)


# ---- determinism
def test_a_pixel_is_independent_of_the_bands_and_passes_follow_the_hash(rtc):
    hs = gb.mix(rtc)
    cam = hs.camera(80, 45)
    smp = rtc.Sampling(2, 1, 0.0, 1.0, 5)
    ck = _checker(hs, dict(hs.gloss(), seed=3))
    whole, wc = ck.render(cam, 5, smp, hs.spots(), sample_pass=2)
    parts, total = [], 0
    for y0, h in ((0, 7), (7, 20), (27, 18)):
        im, c = ck.render(cam, 5, smp, hs.spots(), sample_pass=2, tile=(0, y0, 80, h), threads=1 + y0 % 3)
        parts.append(im)
        total += c["secondary"]
    assert np.array_equal(np.concatenate(parts, axis=0), whole) and total == wc["secondary"]
    cols = [ck.render(cam, 5, smp, hs.spots(), sample_pass=2, tile=(x0, 0, w, 45))[0] for x0, w in ((0, 33), (33, 47))]
    assert np.array_equal(np.concatenate(cols, axis=1), whole)


def _wall_scene(roughness):
    """One pixel looks straight down at a mirror floor; above it a ceiling that is black for x < 0 and white for x > 0,
    lit by its ambient term alone.  The sharp reflection leaves the floor at x = 0.3: white."""
    cam = {"width": 1, "height": 1, "field-of-view": 0.01, "from": [0.3, 1, 0], "to": [0.3, 0, 0], "up": [0, 0, 1]}
    floor = {"type": {"plane": {}}, "material": {"pattern": {"type": {"solid": [0, 0, 0]}}, "ambient": 0, "diffuse": 0, "specular": 0,
                                                 "reflective": 1.0, "roughness": roughness}}
    wall = {"type": {"plane": {}}, "transform": [{"translate": [0, 3, 0]}],
            "material": {"pattern": {"type": {"stripes": [{"type": {"solid": [1, 1, 1]}}, {"type": {"solid": [0, 0, 0]}}]},
                                     "transform": [{"scale": [1000, 1, 1]}]}, "ambient": 1, "diffuse": 0, "specular": 0}}
    lights = [{"point-light": {"position": [0, 2, 0], "intensity": [1, 1, 1]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": [floor, wall]})


def test_pass_p_is_the_hash_at_global_sample_p_times_s_plus_k(rtc):
    """grid 1, no jitter: pass P of the one pixel scatters with h(p = 0, g = P) and code 2.  The reflection's direction is
    restated from J here; the wall's colour tells which side of x = 0 it lands on."""
    hs = rtc.HostScene(_wall_scene(0.5))
    cam = hs.camera()
    ck = _checker(hs, dict(hs.gloss(), seed=21))
    for P in (0, 1, 5, 40):
        got, _ = ck.render(cam, 5, sample_pass=P)
        draws = _jitter_np(21, np.zeros(96, dtype=np.uint64), np.full(96, P, dtype=np.uint64), np.full(96, 2, dtype=np.uint64),
                           np.arange(96, dtype=np.uint64))
        s = _sampler_py(draws)
        # d = (0, 1, 0) up from (0.3, 0, 0): the ceiling at height 3 is met at x = 0.3 + 3 * ex / ey
        ex, ey = 0.0 + s[0] * 0.5, 1.0 + s[1] * 0.5
        white = 0.3 + 3.0 * ex / ey > 0.0
        assert got[0, 0, 0] == (1.0 if white else 0.0), (P, s)


# ---- statistics
def test_a_rough_mirror_converges_between_the_two_sharp_values(rtc):
    """4096 passes of the one pixel of _wall_scene: each pass is black (0) or white (1); the sharp value is 1 and the wall's
    other half is 0.  The standard error of the mean, s / sqrt(n), halves from 1024 to 4096 passes up to the sampling error of
    s itself.  For a Bernoulli pixel of mean p (q = 1 - p) the variance estimate s^2 over n passes has the relative variance
    (k - 1) / n with the kurtosis k = (1 - 3 p q) / (p q); the first 1024 passes are a subset of the 4096, so
    Var(ln s_1024^2 - ln s_4096^2) = (k - 1) (1 / 1024 - 1 / 4096), and the factor f = se_1024 / se_4096 = 2 s_1024 / s_4096 has
    the standard deviation sqrt((k - 1) * 3 / 4096).  The bound is four of those (about 0.09 at p = 0.7), with p the checker's
    own mean over the 4096 passes.  Observed: f = 2.0097 (seed 1) and 2.0118 (seed 2), 0.0021 apart."""
    hs = rtc.HostScene(_wall_scene(0.5))
    cam = hs.camera()
    factors = []
    for seed in (1, 2):
        ck = _checker(hs, dict(hs.gloss(), seed=seed))
        v = np.array([ck.render(cam, 5, sample_pass=p, threads=1)[0][0, 0, 0] for p in range(4096)])
        assert set(np.unique(v)) == {0.0, 1.0}
        p = v.mean()
        assert 0.5 < p < 1.0                                       # between the two sharp values, on the sharp one's side
        se = lambda x: x.std(ddof=1) / np.sqrt(len(x))
        f = se(v[:1024]) / se(v)
        k = (1.0 - 3.0 * p * (1.0 - p)) / (p * (1.0 - p))
        bound = 4.0 * np.sqrt((k - 1.0) * 3.0 / 4096.0)
        print(f"seed {seed}: mean {p:.4f}, standard error 1024 / 4096 passes: {f:.4f}, bound {bound:.4f}")
        assert abs(f - 2.0) <= bound
        factors.append(f)
    assert abs(factors[0] - factors[1]) <= 2.0 * bound


# ---- the loader
def _scene(material):
    return json.dumps({"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
                       "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
                       "objects": [{"type": {"sphere": {}}, "material": material}]})


def test_loader_round_trips(rtc):
    g = rtc.HostScene(_scene({"reflective": 0.5, "roughness": 0.25})).gloss()
    assert g["reflection"].tolist() == [0.25] and g["transmission"].tolist() == [0.25] and g["seed"] == 0
    g = rtc.HostScene(_scene({"roughness": {"reflection": 0.125, "transmission": 1}})).gloss()
    assert g["reflection"].tolist() == [0.125] and g["transmission"].tolist() == [1.0]
    g = rtc.HostScene(_scene({"roughness": {"transmission": 0.5}})).gloss()
    assert g["reflection"].tolist() == [0.0] and g["transmission"].tolist() == [0.5]
    assert rtc.HostScene(_scene({"diffuse": 0.5})).gloss() is None
    zero = rtc.HostScene(_scene({"roughness": 0})).gloss()          # the key is there, its values are zero
    assert zero is not None and not zero["reflection"].any() and not zero["transmission"].any()
    scene = json.loads(_scene({"roughness": 0.5}))
    scene["camera"]["sampling"] = {"gloss-seed": 77}
    assert rtc.HostScene(json.dumps(scene)).gloss()["seed"] == 77


def test_roughness_is_inherited_overridden_and_a_row_only_when_non_zero(rtc):
    base = {"pattern": {"type": {"solid": [1, 0, 0]}}, "reflective": 0.5}
    objs = [{"type": {"sphere": {}}, "material": dict(base)},
            {"type": {"sphere": {}}, "material": dict(base, roughness=0)},                   # the same row as the first
            {"type": {"group": [{"type": {"sphere": {}}},                                    # inherits 0.3
                                {"type": {"sphere": {}}, "material": {"roughness": {"reflection": 0.6}}}]},   # overrides: (0.6, 0)
             "material": dict(base, roughness=0.3)}]
    scene = json.loads(_scene({}))
    scene["objects"] = objs
    hs = rtc.HostScene(json.dumps(scene))
    g = hs.gloss()
    assert hs.desc.n_materials == 3
    rows = sorted(zip(g["reflection"].tolist(), g["transmission"].tolist()))
    assert rows == [(0.0, 0.0), (0.3, 0.3), (0.6, 0.0)]
    mats = [int(hs.desc.leaf_material[i]) for i in range(hs.desc.n_leaves)]
    assert mats[0] == mats[1] and len(set(mats)) == 3


@pytest.mark.parametrize("value, key", [
    (-0.1, "roughness"), (1.5, "roughness"), ("rough", "roughness"), ([0.1, 0.2], "roughness"), (True, "roughness"),
    ({"reflection": 2}, "roughness.reflection"), ({"reflection": "x"}, "roughness.reflection"),
    ({"transmission": -1e-9}, "roughness.transmission"), ({"transmission": [0.1]}, "roughness.transmission"),
    ({"refraction": 0.1}, "roughness.refraction"),
], ids=["negative", "above-1", "string", "list", "bool", "reflection-2", "reflection-string", "transmission-negative",
        "transmission-list", "unknown-field"])
def test_loader_refuses_a_malformed_entry_by_key(rtc, value, key):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene({"roughness": value}))
    assert key in str(e.value)


def test_loader_refuses_a_malformed_gloss_seed(rtc):
    scene = json.loads(_scene({"roughness": 0.5}))
    scene["camera"]["sampling"] = {"gloss-seed": -1}
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(json.dumps(scene))
    assert "gloss-seed" in str(e.value)


def test_host_gloss_needs_the_material_count(rtc):
    hs = gb.mix(rtc)
    dp = C.POINTER(C.c_double)
    a, b = np.zeros(3), np.zeros(3)
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_gloss(hs._h, a.ctypes.data_as(dp), b.ctypes.data_as(dp), None, None, 3))


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(SCENES) if f.endswith(".json")))
def test_reference_scenes_load_without_gloss_and_with_their_digests(rtc, name):
    """tests/golden/torus_scenes/reference_tables.json: the digests of the 17 scenes' tables (tests/test_torus_cpu.py)."""
    want = json.load(open(os.path.join(REPO, "tests", "golden", "torus_scenes", "reference_tables.json")))
    hs = rtc.HostScene.from_file(name)
    assert hs.gloss() is None
    assert ttc._digest(hs) == want[name]


# ---- rtc_scene_set_gloss: refused before anything changes
def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (tests/test_bump_cpu.py's way)."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    g, _keep = rtc.gloss_struct({"reflection": [0.5], "transmission": [0.5]})
    assert _status(lib, lib.rtc_scene_set_gloss(None, C.byref(g))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_gloss(None, None)) == "InvalidArgument"


@pytest.mark.parametrize("gloss, words", [
    ({"reflection": [0.1, np.nan]}, "not finite"), ({"transmission": [np.inf, 0.0]}, "not finite"),
    ({"reflection": [0.1, 0.2], "transmission": [-np.inf, 0.0]}, "not finite"),
    ({"reflection": [-1e-300, 0.0]}, "outside [0, 1]"), ({"transmission": [0.0, 1.0 + 2.0 ** -52]}, "outside [0, 1]"),
    ({"reflection": [0.0, 2.0], "transmission": [0.5, 0.5]}, "outside [0, 1]"),
], ids=["nan", "inf", "neg-inf", "below-0", "above-1", "two"])
def test_setter_rejects_an_invalid_value_and_touches_nothing(rtc, gloss, words):
    """The table's own values are checked before its count against the handle: the stand-in's material count reads as
    0xA5A5A5A5, so each of these is refused for its own reason."""
    lib = rtc.hip_lib()
    handle = _stand_in()
    g, _keep = rtc.gloss_struct(gloss)
    st = lib.rtc_scene_set_gloss(C.cast(handle, C.c_void_p), C.byref(g))
    assert _status(lib, st) == "InvalidArgument"
    assert words in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


@pytest.mark.parametrize("n", [0, 1, 7])
def test_setter_rejects_a_wrong_material_count_and_touches_nothing(rtc, n):
    lib = rtc.hip_lib()
    handle = _stand_in()
    g, _keep = rtc.gloss_struct({"reflection": np.full(n, 0.5), "transmission": np.zeros(n)})
    st = lib.rtc_scene_set_gloss(C.cast(handle, C.c_void_p), C.byref(g))
    assert _status(lib, st) == "InvalidArgument"
    assert "n_materials" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL
