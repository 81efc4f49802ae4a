"""Indirect light without a GPU: the symbols and the struct, the setter's validation through the ABI on a
stand-in handle, the loader's "indirect" and "emission" and rtch_scene_indirect, the tables with the keys deleted, the checker
(tests/cpp/indirect_oracle.cpp) - its identity with the sky-light checker wherever no child is formed and nothing emits, a
furnace whose value is a geometric series, a floor under an open sky, the two statistical cases of section 25 with the child's
miss in place of the sky light's samples, the counts -, the fixture's conditions, and the documents.

The furnace: 9 x 9, the camera inside a scaled sphere (colour K, diffuse kd, ambient 0, specular 0, emission E), no lights and
no environment.  Every direction of an inward hemisphere meets the same wall, so whatever the draws a ray with k bounces
behind it returns E + a * (the next), a = K * kd * gain per channel: a pixel is E * sum_{k=0..n} a^k, n = min(bounces,
max_depth)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import environment_binding as eb
import indirect_binding as ib
import skylight_binding as sb
import test_skylight_cpu as scpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
W, H, DEPTH = 80, 45, 5
TOL = 1e-12
FIXTURES = {"skylight_mix": sb.SKYLIGHT_MIX, "sky_mix": eb.SKY_MIX, "indirect_mix": ib.INDIRECT_MIX}


# ---- ABI and options
def test_symbols_struct_and_option(rtc):
    assert "rtc_scene_set_indirect" in rtc.RTC_SYMBOLS and "rtch_scene_indirect" in rtc.HOST_SYMBOLS
    assert "indirect_kernels" in rtc.KERNEL_OPTIONS
    assert rtc.hip_lib().rtc_scene_set_indirect is not None and rtc.host_lib().rtch_scene_indirect is not None
    D = rtc.Indirect
    assert C.sizeof(D) == 40
    assert (D.gain.offset, D.bounces.offset, D.seed.offset, D.emission.offset, D.n_materials.offset) == (0, 8, 16, 24, 32)
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_indirect(rtc_scene *scene, const rtc_indirect *indirect);" in text
    for line in ("typedef struct rtc_indirect {", "#define RTC_ABI_VERSION 3u", "#define RTC_INDIRECT_DECORR 0xBE5466CF34E90C6Dull"):
        assert line in text, line
    assert int("BE5466CF34E90C6D", 16) % 2 == 1
    assert "indirect_kernels" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "rtc_scene_set_indirect" in open(os.path.join(REPO, "include", "rtc_multi.h")).read()
    assert "rtch_scene_indirect" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    rtc.set_option("indirect_kernels", 1)
    rtc.set_option("indirect_kernels", 0)
    zig = open(os.path.join(REPO, "integration", "gpu.zig")).read()
    assert "rtc_scene_set_indirect" in zig and "RtcIndirect" in zig


def test_headers_are_still_strict_c99_and_the_binding_matches():
    import test_abi
    test_abi.test_headers_are_valid_c()
    test_abi.test_zig_binding_matches_the_header()


def test_the_key_is_new_and_the_constants_agree():
    """0x452821E638D01377: the word of pi's expansion after the sky light's; the product has it once, the checker once.  The
    decorrelation constant is rtc.h's in the device header, token for token."""
    device = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_device.h")).read()
    assert device.count("0x452821E638D01377") == 1
    assert open(os.path.join(REPO, "tests", "cpp", "indirect_oracle.cpp")).read().count("0x452821E638D01377") == 1
    pi_words = "243F6A8885A308D3 13198A2E03707344 A4093822299F31D0 082EFA98EC4E6C89 452821E638D01377".split()
    assert device.index("0x" + pi_words[3]) < device.index("0x" + pi_words[4])
    assert "#define RTC_INDIRECT_DECORR 0xBE5466CF34E90C6Dull" in device


# ---- rtc_scene_set_indirect: refused on the host before anything changes
def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (tests/test_bump_cpu.py's way)."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    d, _keep = rtc.indirect_struct({"gain": 1.0})
    assert _status(lib, lib.rtc_scene_set_indirect(None, C.byref(d))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_indirect(None, None)) == "InvalidArgument"


def _rows(n=3, **at):
    e = np.zeros((n, 3))
    for (i, c), v in at.items():
        e[i, c] = v
    return e


@pytest.mark.parametrize("table, words", [
    ({"gain": np.nan}, "not finite"),
    ({"gain": np.inf}, "not finite"),
    ({"gain": -np.inf}, "not finite"),
    ({"gain": -1e-300}, "negative"),
    ({"gain": 1.0, "bounces": 17}, "bounces"),
    ({"gain": 0.0, "bounces": 17}, "bounces"),
    ({"gain": 1.0, "bounces": 0xFFFFFFFF}, "bounces"),
    ({"gain": 1.0, "emission": np.array([[0.0, 0.0, 0.0], [0.0, -1e-300, 0.0], [0.0, 0.0, 0.0]])}, "negative"),
    ({"gain": 1.0, "emission": np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, np.nan]])}, "not finite"),
    ({"gain": 0.0, "bounces": 0, "emission": np.array([[np.inf, 0.0, 0.0]])}, "not finite"),
    ({"gain": 1.0, "emission": np.zeros((3, 3))}, "n_materials"),     # (the stand-in's count is its sentinel bytes)
], ids=["gain-nan", "gain-inf", "gain-minus-inf", "gain-negative", "17-bounces", "17-bounces-no-gain", "bounces-wrap", "emission-negative",
        "emission-nan", "emission-inf-alone", "material-count"])
def test_setter_rejects_an_invalid_table_and_touches_nothing(rtc, table, words):
    lib = rtc.hip_lib()
    handle = _stand_in()
    d, _keep = rtc.indirect_struct(table)
    st = lib.rtc_scene_set_indirect(C.cast(handle, C.c_void_p), C.byref(d))
    assert _status(lib, st) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert words in text and "indirect:" in text
    assert bytes(handle) == b"\xa5" * SENTINEL


# ---- the loader
def _solid(c):
    return {"type": {"solid": [float(x) for x in c]}}


def _scene(indirect=None, emission=None):
    material = {"pattern": _solid([0.2, 0.4, 0.6])}
    if emission is not None:
        material["emission"] = emission
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
         "objects": [{"type": {"sphere": {}}, "material": material}]}
    if indirect is not None:
        s["indirect"] = indirect
    return json.dumps(s)


def _table(hs):
    t = hs.indirect()
    return None if t is None else {k: (v.tolist() if k == "emission" else v) for k, v in t.items()}


@pytest.mark.parametrize("indirect, want", [
    (0.5, {"gain": 0.5, "bounces": 1, "seed": 0}),
    (0, {"gain": 0.0, "bounces": 1, "seed": 0}),
    ({}, {"gain": 1.0, "bounces": 1, "seed": 0}),
    ({"bounces": 16}, {"gain": 1.0, "bounces": 16, "seed": 0}),
    ({"bounces": 0}, {"gain": 1.0, "bounces": 0, "seed": 0}),
    ({"gain": 2.5, "bounces": 4, "seed": 9}, {"gain": 2.5, "bounces": 4, "seed": 9}),
    ({"seed": 2 ** 53}, {"gain": 1.0, "bounces": 1, "seed": 2 ** 53}),
], ids=["number", "zero", "defaults", "16-bounces", "no-bounces", "every-key", "seed-2^53"])
def test_loader_reads_the_top_level_key(rtc, indirect, want):
    assert _table(rtc.HostScene(_scene(indirect))) == dict(want, emission=[[0.0, 0.0, 0.0]])


@pytest.mark.parametrize("emission, want", [(0.75, [0.75, 0.75, 0.75]), ([1, 2.5, 0], [1.0, 2.5, 0.0]), (0, [0.0, 0.0, 0.0])],
                         ids=["number", "triple", "zero"])
def test_loader_reads_a_materials_emission(rtc, emission, want):
    assert _table(rtc.HostScene(_scene(None, emission))) == {"gain": 0.0, "bounces": 0, "seed": 0, "emission": [want]}
    assert _table(rtc.HostScene(_scene(0.5, emission))) == {"gain": 0.5, "bounces": 1, "seed": 0, "emission": [want]}


def test_a_file_without_the_keys_has_no_table(rtc):
    assert rtc.HostScene(_scene()).indirect() is None


@pytest.mark.parametrize("indirect, emission, name", [
    ({"gain": 1, "bounce": 2}, None, "UnknownField"),
    ({"strength": 1}, None, "UnknownField"),
    ("on", None, "InvalidData"),
    (True, None, "InvalidData"),
    ([1.0], None, "InvalidData"),
    (-0.5, None, "InvalidData"),
    ({"gain": -1e-9}, None, "InvalidData"),
    ("@1e999@", None, "InvalidData"),
    ({"gain": "1"}, None, "InvalidData"),
    ({"bounces": -1}, None, "InvalidData"),
    ({"bounces": 17}, None, "InvalidData"),
    ({"bounces": 2.5}, None, "InvalidData"),
    ({"bounces": "4"}, None, "InvalidData"),
    ({"seed": -1}, None, "InvalidData"),
    ({"seed": 0.5}, None, "InvalidData"),
    ({"seed": 2 ** 53 + 2}, None, "InvalidData"),
    ({"seed": "x"}, None, "InvalidData"),
    (None, "bright", "InvalidData"),
    (None, -0.1, "InvalidData"),
    (None, [1, -1e-9, 0], "InvalidData"),
    (None, [1, "2", 0], "InvalidData"),
    (None, "@1e999@", "InvalidData"),
    (None, [1, 2], "LengthMismatch"),
], ids=["unknown-key", "unknown-key-alone", "string", "bool", "list", "negative", "gain-negative", "gain-inf", "gain-string", "bounces-negative",
        "17-bounces", "bounces-fraction", "bounces-string", "seed-negative", "seed-fraction", "seed-above-2^53", "seed-string", "emission-string",
        "emission-negative", "emission-entry-negative", "emission-entry-string", "emission-inf", "emission-pair"])
def test_loader_refuses_malformed_keys(rtc, indirect, emission, name):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(indirect, emission).replace('"@1e999@"', "1e999"))     # (a number that reads as +infinity)
    assert e.value.name == name, (e.value.name, str(e.value))


def _without_keys(path):
    scene = json.loads(open(path).read())
    scene.pop("indirect", None)
    for o in scene["objects"]:
        o.get("material", {}).pop("emission", None)
    return json.dumps(scene)


def test_the_keys_add_no_table_row(rtc):
    """The fixture with both keys deleted flattens to the same tables: neither is a row of any of them."""
    import test_environment_cpu as ecpu
    with_keys = ib.mix(rtc)
    bare = rtc.HostScene(_without_keys(ib.INDIRECT_MIX))
    assert with_keys.indirect() is not None and bare.indirect() is None
    assert ecpu._tables(with_keys.desc) == ecpu._tables(bare.desc)
    assert with_keys.sky_light() == bare.sky_light() and np.array_equal(with_keys.media()["absorption"], bare.media()["absorption"])


def test_reference_scenes_and_earlier_fixtures_load_without_a_table(rtc):
    """(their digests are held by the tests that held them: the loader reads two more keys and nothing else)"""
    scenes = os.path.join(REPO, "tests", "golden", "scenes")
    for name in sorted(f for f in os.listdir(scenes) if f.endswith(".json")):
        assert rtc.HostScene.from_file(name).indirect() is None, name
    assert eb.mix(rtc).indirect() is None and sb.mix(rtc).indirect() is None


def test_host_indirect_is_the_table_of_rtch_scene_indirect(rtc):
    hs = ib.mix(rtc)
    n = hs.desc.n_materials
    d, e, present = rtc.Indirect(), np.zeros((n, 3)), C.c_int()
    dp = C.POINTER(C.c_double)
    rtc._check_host(rtc.host_lib().rtch_scene_indirect(hs._h, C.byref(d), e.ctypes.data_as(dp), C.byref(present), n))
    assert present.value == 1 and (d.gain, d.bounces, d.seed, d.n_materials) == (0.9, 2, 7, n)
    assert C.cast(d.emission, C.c_void_p).value == e.ctypes.data
    assert sorted(map(tuple, e[e.any(axis=1)].tolist())) == [(1.6, 1.45, 1.1)]
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_indirect(hs._h, None, e.ctypes.data_as(dp), None, n))
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_indirect(hs._h, C.byref(d), e.ctypes.data_as(dp), None, n + 1))
    other = sb.mix(rtc)
    e2 = np.ones((other.desc.n_materials, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_indirect(other._h, C.byref(d), e2.ctypes.data_as(dp), C.byref(present), other.desc.n_materials))
    assert present.value == 0 and (d.gain, d.bounces, d.seed) == (0.0, 0, 0) and not e2.any()


# ---- identity: where no child is formed and nothing emits the render is the sky-light checker's, bit for bit
def _no_diffuse(path):
    scene = json.loads(_without_keys(path))
    for o in scene["objects"]:
        o.setdefault("material", {})["diffuse"] = 0
    return json.dumps(scene)


IDENTITY_TABLES = {"no-table": None, "gain-0": {"gain": 0.0, "bounces": 4, "seed": 3}, "bounces-0": {"gain": 0.8, "bounces": 0, "seed": 3},
                   "no-diffuse": {"gain": 0.8, "bounces": 4, "seed": 3}}


@pytest.mark.parametrize("case", list(IDENTITY_TABLES))
@pytest.mark.parametrize("fixture", list(FIXTURES))
def test_where_no_child_is_formed_is_the_sky_light_checker_bit_for_bit(rtc, fixture, case):
    path = FIXTURES[fixture]
    hs = rtc.HostScene(_no_diffuse(path)) if case == "no-diffuse" else rtc.HostScene.from_file(path)
    cam = hs.camera(W, H)
    ck = ib.scene_of(rtc, hs, indirect=IDENTITY_TABLES[case])
    got, c = ck.render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    want, cs = ck.render_skyl(cam, DEPTH, spots=hs.spots(), light_seed=3)
    assert np.array_equal(got, want)
    for k in ib.SKYL_ALL:
        assert c[k] == cs[k], k
    for k in ("ind_formed", "ind_suppressed", "ind_miss_sky", "ind_emitted"):
        assert c[k] == 0, k
    if case in ("no-table", "gain-0", "no-diffuse"):
        assert c["ind_no_remaining"] == 0 and c["ind_no_bounces"] == 0
    else:
        assert c["ind_no_bounces"] > 0


def test_a_table_of_zero_rows_is_no_emission(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    ck = ib.scene_of(rtc, hs, indirect={"gain": 0.0, "bounces": 0, "emission": np.zeros((hs.desc.n_materials, 3))})
    assert np.array_equal(ck.render(cam, DEPTH, spots=hs.spots())[0], ck.render_skyl(cam, DEPTH, spots=hs.spots())[0])


# ---- the furnace (shared with tests/test_indirect_gpu.py)
FURNACE_K, FURNACE_KD, FURNACE_G = np.array([0.8, 0.5, 0.2]), 0.9, 1.1
FURNACE_E = np.array([0.25, 0.5, 1.0])
FURNACE_CASES = [(0, 16), (1, 16), (2, 16), (16, 16), (16, 3)]      # (bounces, max_depth)


def furnace_scene(bounces, size=9, gain=FURNACE_G):
    wall = {"type": {"sphere": {}}, "transform": [{"scale": [3, 2.5, 3.5]}],
            "material": {"pattern": _solid(FURNACE_K), "ambient": 0, "diffuse": FURNACE_KD, "specular": 0, "emission": FURNACE_E.tolist()}}
    camera = {"width": size, "height": size, "field-of-view": 1.2, "from": [0.3, 0.2, -0.5], "to": [0, 0.4, 1], "up": [0, 1, 0]}
    return json.dumps({"camera": camera, "lights": [], "objects": [wall], "indirect": {"gain": gain, "bounces": bounces, "seed": 5}})


def furnace_value(bounces, max_depth):
    """E * sum_{k=0..n} a^k, summed from the deepest ray up as the recursion does: v = E + a * v"""
    a = (FURNACE_K * FURNACE_KD) * FURNACE_G
    v = FURNACE_E.copy()
    for _ in range(min(bounces, max_depth)):
        v = FURNACE_E + a * v
    return v


def check_furnace(render, size):
    """for a `render(scene json, depth) -> ([size][size][3], secondary)`: the checker's here, the GPU's in
    tests/test_indirect_gpu.py.  Prints each figure before it asserts."""
    for bounces, depth in FURNACE_CASES:
        img, secondary = render(furnace_scene(bounces, size), depth)
        want = furnace_value(bounces, depth)
        closed = FURNACE_E * sum(((FURNACE_K * FURNACE_KD) * FURNACE_G) ** k for k in range(min(bounces, depth) + 1))
        assert np.abs(want - closed).max() <= 1e-14
        delta = float(np.abs(img - want).max())
        print(f"furnace bounces {bounces} depth {depth}: centre {img[size // 2, size // 2]} derived {want} max |delta| {delta:.3e} secondary {secondary}")
        assert delta <= TOL, (bounces, depth, delta)
        assert secondary == min(bounces, depth) * size * size


def _render(rtc, scene, depth=DEPTH, sample_pass=0, threads=0):
    hs = rtc.HostScene(scene)
    return ib.scene_of(rtc, hs).render(hs.camera(), depth, spots=hs.spots(), sample_pass=sample_pass, threads=threads)


def test_furnace_on_the_checker(rtc):
    def render(scene, depth):
        img, c = _render(rtc, scene, depth)
        return img, c["secondary"]
    check_furnace(render, 9)


def test_furnace_counts(rtc):
    """16 bounces at depth 3: the deepest hit's child is withheld by `remaining`; 2 bounces at depth 16: by `bounces`."""
    _, c = _render(rtc, furnace_scene(16), 3)
    assert (c["ind_formed"], c["ind_no_remaining"], c["ind_no_bounces"], c["ind_max_pending"]) == (3 * 81, 81, 0, 0)
    _, c = _render(rtc, furnace_scene(2), 16)
    assert (c["ind_formed"], c["ind_no_remaining"], c["ind_no_bounces"], c["ind_emitted"]) == (2 * 81, 0, 81, 3 * 81)


# ---- an open sky over section 25's derived floor (shared with tests/test_indirect_gpu.py)
IND_G = 0.6
OPEN_CHILD = (scpu.FLOOR_K * scpu.FLOOR_KD) * (IND_G * scpu.SKY_C)


def open_sky_scene(objects, sky_light=None, bounces=1):
    env = {"color": scpu.SKY_C.tolist()}
    if sky_light is not None:
        env["light"] = {"gain": sky_light, "samples": 2, "seed": 4}
    return json.dumps({"camera": scpu.LOOK_DOWN, "lights": [], "objects": list(objects), "environment": env,
                       "indirect": {"gain": IND_G, "bounces": bounces, "seed": 8}})


def check_open_sky(render):
    """for a `render(scene json, depth) -> ([9][9][3], secondary)`"""
    # ---- no sky light: the child misses and carries the sky: (K * kd) * g * C
    img, secondary = render(open_sky_scene([scpu._floor()]), 5)
    delta = float(np.abs(img - OPEN_CHILD).max())
    print(f"open sky, child alone: centre {img[4, 4]} derived {OPEN_CHILD} max |delta| {delta:.3e}")
    assert delta <= TOL and secondary == 81
    # ---- with a sky light of gain g': the step gathered that sky, the child's miss adds nothing - and is still counted
    img, secondary = render(open_sky_scene([scpu._floor()], sky_light=scpu.GAIN), 5)
    delta = float(np.abs(img - scpu.OPEN).max())
    print(f"open sky, sky light and child: centre {img[4, 4]} derived {scpu.OPEN} max |delta| {delta:.3e}")
    assert delta <= TOL and secondary == 81
    # ---- a mirror floor forms no child: the file without the key renders the same, one reflected ray a pixel
    mirror = {"type": {"plane": {}}, "material": {"pattern": _solid([1, 1, 1]), "ambient": 0, "diffuse": 0, "specular": 0, "reflective": 1}}
    img, secondary = render(open_sky_scene([mirror]), 5)
    assert np.abs(img - scpu.SKY_C).max() <= TOL and secondary == 81


def test_open_sky_on_the_checker(rtc):
    def render(scene, depth):
        img, c = _render(rtc, scene, depth)
        return img, c["secondary"]
    check_open_sky(render)
    _, c = _render(rtc, open_sky_scene([scpu._floor()], sky_light=scpu.GAIN), 5)
    assert (c["ind_suppressed"], c["ind_miss_sky"]) == (81, 0)
    _, c = _render(rtc, open_sky_scene([scpu._floor()]), 5)
    assert (c["ind_suppressed"], c["ind_miss_sky"]) == (0, 81)


# ---- the statistical cases of section 25, the sky light off, bounces 1: the child's miss now carries the sky
def _child_scene(objects, sky, camera, seed):
    return json.dumps({"camera": camera, "lights": [], "objects": list(objects), "environment": sky,
                       "indirect": {"gain": scpu.GAIN, "bounces": 1, "seed": seed}})


def halves_scene():
    return _child_scene([scpu._floor()], scpu.HALVES, scpu._camera((0, 0.5, -0.5), (0, 0, 0), 8), 17)


def ramp_scene():
    return _child_scene([scpu.WALL], scpu.RAMP, scpu.LOOK_AT_WALL, 23)


def _mean_over_passes(rtc, scene):
    hs = rtc.HostScene(scene)
    ck = ib.scene_of(rtc, hs)
    total = np.zeros((8, 8, 3))
    for p in range(scpu.N_PASSES):
        total += ck.render(hs.camera(), DEPTH, spots=hs.spots(), sample_pass=p, threads=1)[0]
    return total / scpu.N_PASSES


def test_half_the_children_of_a_floor_see_the_white_half_of_the_sky(rtc):
    assert abs(scpu.BOUND_HALVES - 0.0156) < 1e-4 and scpu.N_PASSES == 256
    scpu.check_statistical_case("halves", _mean_over_passes(rtc, halves_scene()), 0.5, scpu.BOUND_HALVES)


def test_the_mean_cosine_of_a_walls_children_is_two_thirds(rtc):
    assert abs(scpu.BOUND_RAMP - 0.0074) < 1e-4
    scpu.check_statistical_case("ramp", _mean_over_passes(rtc, ramp_scene()), 2.0 / 3.0, scpu.BOUND_RAMP)


# ---- draws
def test_draws_are_the_tables_own_and_move_with_d(rtc):
    """Another seed moves the image.  With d in the keys the sky-light draws at a diffuse child's hit differ from those the
    same code would get at d = 0: a second bounce changes the image beyond what its own light adds alone - here only that the
    renders differ and the one-bounce render is not above the two-bounce one anywhere."""
    hs = ib.mix(rtc)
    cam = hs.camera(W, H)
    table = hs.indirect()
    a = ib.scene_of(rtc, hs).render(cam, DEPTH, spots=hs.spots())[0]
    b = ib.scene_of(rtc, hs, indirect=dict(table, seed=12)).render(cam, DEPTH, spots=hs.spots())[0]
    one = ib.scene_of(rtc, hs, indirect=dict(table, bounces=1)).render(cam, DEPTH, spots=hs.spots())[0]
    assert not np.array_equal(a, b) and not np.array_equal(a, one)
    assert (a >= one - TOL).all()       # (the same first children: the key of d = 0 is the table's; the second bounce only adds)


# ---- the fixture
def test_fixture_meets_its_conditions(rtc):
    hs = ib.mix(rtc)
    assert os.path.getsize(ib.INDIRECT_MIX) < 8192
    scene = json.loads(open(ib.INDIRECT_MIX).read())
    assert (scene["camera"]["width"], scene["camera"]["height"]) == (W, H)
    e = hs.environment()
    assert e["pattern"] != rtc.ENV_NO_PATTERN and hs.lights.n_lights == 1 and hs.sky_light() is not None
    assert hs.occlusion() is not None and (np.asarray(hs.occlusion()["radius"]) > 0).any()
    assert hs.gloss() is not None and hs.bumps() is not None and hs.media()["fog_density"] > 0
    mats = [o["material"] for o in scene["objects"]]
    assert any(m.get("diffuse") == 0.0 and m.get("reflective", 0) > 0 for m in mats)                                # the mirror ball
    assert any(m.get("reflective", 0) > 0 and m.get("transparency", 0) > 0 and m.get("diffuse", 0) > 0 for m in mats)   # the pane
    assert any("emission" in m for m in mats)
    reds = [m["pattern"]["type"]["solid"] for m in mats if "solid" in m["pattern"]["type"]]
    assert any(r > 4 * g and r > 4 * b for r, g, b in reds) and any(g > 4 * r and g > 4 * b for r, g, b in reds)
    img, c = ib.scene_of(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    print({k: c[k] for k in ib.IND_COUNTERS})
    for k in ("ind_formed", "ind_no_remaining", "ind_no_bounces", "ind_suppressed", "ind_emitted"):
        assert c[k] > 0, k
    assert c["ind_max_pending"] > DEPTH + 2      # (the stack of max_depth + 2 levels would have overflowed)
    assert img.std() > 0.05
    # a red wall throws red onto what stands beside it: the bounce adds more red than blue on the left of the frame
    bare = ib.scene_of(rtc, hs, indirect=dict(hs.indirect(), gain=0.0)).render(hs.camera(W, H), DEPTH, spots=hs.spots())[0]
    added = (img - bare)[:, : W // 4].mean(axis=(0, 1))
    assert added[0] > added[2] > 0.0


# ---- documents and build
def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("s.c = s.c + emission[material].c", "key = rtc_mix64(seed ^ 0x452821E638D01377)", "(d << 17) | cur.code",
                 "weight.c  = cur.weight.c * ((color.c * material.diffuse) * gain)", "remaining = cur.remaining - 1",
                 "key' = key ^ ((uint64_t)d * RTC_INDIRECT_DECORR)", "no pi and no cosine appear", "does not bias the mean",
                 "adds no sky", "librtc_multi renders without it"):
        assert line in header, line


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 27." in design
    for word in ("rtc_scene_set_indirect", "rtc_render_kernel_indir", "rtc_render_kernel_indir_bigworld", "indirect_kernels", "occl_direction",
                 "tests/cpp/indirect_oracle.cpp", "profiles/indirect/disassembly_identity.txt", "indirect_mix.json", "2 * max_depth + 2",
                 "does not bias the mean", "Out of scope"):
        assert word in design, word
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resources rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_render_kernel_indir", "rtc_render_kernel_indir_bigworld"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} | {k['lds_bytes_per_block']} |" in design, name
            assert k["lds_bytes_per_block"] == resources.get("kernels", resources)[name.replace("_indir", "_skyl")]["lds_bytes_per_block"]
    for doc, word in (("README.md", "rtc_scene_set_indirect"), ("INTEGRATION.md", "rtc_scene_set_indirect"), ("INTEGRATION.md", "RtcIndirect"),
                      (os.path.join("tools", "README.md"), "--indirect"), (os.path.join("profiles", "HISTORY.md"), "indirect light")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)


def test_disassembly_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "indirect", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_kernels_ext.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o",
                "rtc_occlusion.o", "rtc_shadowfilter.o", "rtc_media.o", "rtc_environment.o", "rtc_skylight.o", "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_indir", "rtc_render_kernel_indir_bigworld", "rtc_render_kernel_skyl", "rtc_render_kernel_skyl_bigworld"):
        assert kernel in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_indirect.o", "rtc_indirect.remarks", "libindirect_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_indirect.hip")).read()
    for word in ("#define RTC_INDIR_TU", "#define RTC_SKYL_TU", "#define RTC_ENV_TU", "#define RTC_MEDIA_TU", "#define RTC_SFILT_TU",
                 "#define RTC_OCCL_TU", "#define RTC_GLOSS_TU", "#define RTC_MESHUV_TU", "#define RTC_TORUS_TU", '#include "rtc_kernels.hip"'):
        assert word in unit, word
    kernels = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_kernels.hip")).read()
    assert "static_assert(!INDIRECT || SKYL" in kernels and "static_assert(!INDIRECT || !COOP" in kernels
    assert kernels.count("trace<CSG, WORLD, SunVisitor") == 2     # (the environment unit's call and the sky-light unit's: no further walk)
    host = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_host_internal.h")).read()
    assert "ENV, SKYL, INDIR };" in host and "f == Family::SKYL || f == Family::INDIR" in host
