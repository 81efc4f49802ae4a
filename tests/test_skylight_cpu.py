"""The sky light without a GPU: the symbols and the struct, the setter's validation through the ABI on a
stand-in handle, the loader's "light" and rtch_scene_sky_light, the digests and tables with the key deleted, the checker
(tests/cpp/skylight_oracle.cpp) - its identity with the environment checker wherever the step does not run, values derived
by hand on a matte floor under a uniform sky, two statistical cases whose means and bounds are derived, the counts -, the
fixture's conditions, and the documents.

The derived cases: 9 x 9, every camera ray meets a matte floor (colour K, diffuse kd, ambient 0, specular 0) in a world
without lights and suns, so a pixel is the sky-light term alone, (K * kd) * (gain * (L / samples)).  Under a uniform sky C
every sample that is not blocked adds T * C: an open sky gives (K * kd) * (g * C) whatever the directions."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import environment_binding as eb
import skylight_binding as sb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1 << 16
W, H, DEPTH = 80, 45, 5
TOL = 1e-12
HALF_PI = 1.5707963267948966


# ---- ABI and options
def test_symbols_struct_and_option(rtc):
    assert "rtc_scene_set_sky_light" in rtc.RTC_SYMBOLS and "rtch_scene_sky_light" in rtc.HOST_SYMBOLS
    assert "sky_light_kernels" in rtc.KERNEL_OPTIONS
    assert rtc.hip_lib().rtc_scene_set_sky_light is not None and rtc.host_lib().rtch_scene_sky_light is not None
    Y = rtc.SkyLight
    assert C.sizeof(Y) == 24
    assert (Y.gain.offset, Y.samples.offset, Y.seed.offset) == (0, 8, 16)
    assert rtc.SKY_LIGHT_MAX_SAMPLES == 64
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_sky_light(rtc_scene *scene, const rtc_sky_light *sky_light);" in text
    for line in ("#define RTC_SKY_LIGHT_MAX_SAMPLES 64u", "typedef struct rtc_sky_light {", "#define RTC_ABI_VERSION 3u",
                 "Occlusion rays and shadow rays do not see the sky"):
        assert line in text, line
    assert "sky_light_kernels" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "rtc_scene_set_sky_light" in open(os.path.join(REPO, "include", "rtc_multi.h")).read()
    assert "rtch_scene_sky_light" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    rtc.set_option("sky_light_kernels", 1)
    rtc.set_option("sky_light_kernels", 0)
    zig = open(os.path.join(REPO, "integration", "gpu.zig")).read()
    assert "rtc_scene_set_sky_light" in zig and "RtcSkyLight" in zig


def test_headers_are_still_strict_c99_and_the_binding_matches():
    import test_abi
    test_abi.test_headers_are_valid_c()
    test_abi.test_zig_binding_matches_the_header()


def test_the_key_is_new_and_in_one_place():
    """0x082EFA98EC4E6C89: the word of pi's expansion after the camera's, the gloss's and the occlusion's; the product has it
    once, the checker once."""
    device = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_device.h")).read()
    assert device.count("0x082EFA98EC4E6C89") == 1
    assert open(os.path.join(REPO, "tests", "cpp", "skylight_oracle.cpp")).read().count("0x082EFA98EC4E6C89") == 1


# ---- rtc_scene_set_sky_light: refused on the host before anything changes
def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for (tests/test_bump_cpu.py's way)."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    y = rtc.sky_light_struct({"gain": 1.0})
    assert _status(lib, lib.rtc_scene_set_sky_light(None, C.byref(y))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_sky_light(None, None)) == "InvalidArgument"


@pytest.mark.parametrize("light, words", [
    ({"gain": np.nan}, "not finite"),
    ({"gain": np.inf}, "not finite"),
    ({"gain": -np.inf}, "not finite"),
    ({"gain": -1e-300}, "negative"),
    ({"gain": 1.0, "samples": 0}, "samples"),
    ({"gain": 1.0, "samples": 65}, "samples"),
    ({"gain": 0.0, "samples": 65}, "samples"),
    ({"gain": 1.0, "samples": 0xFFFFFFFF}, "samples"),
], ids=["gain-nan", "gain-inf", "gain-minus-inf", "gain-negative", "no-samples", "65-samples", "65-samples-no-gain", "samples-wrap"])
def test_setter_rejects_an_invalid_table_and_touches_nothing(rtc, light, words):
    lib = rtc.hip_lib()
    handle = _stand_in()
    y = rtc.sky_light_struct(light)
    st = lib.rtc_scene_set_sky_light(C.cast(handle, C.c_void_p), C.byref(y))
    assert _status(lib, st) == "InvalidArgument"
    text = lib.rtc_last_error().decode()
    assert words in text and "sky light:" in text
    assert bytes(handle) == b"\xa5" * SENTINEL


# ---- the loader
def _solid(c):
    return {"type": {"solid": [float(x) for x in c]}}


def _scene(environment=None):
    s = {"camera": {"width": 8, "height": 8, "field-of-view": 1, "from": [0, 0, -5], "to": [0, 0, 0], "up": [0, 1, 0]},
         "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
         "objects": [{"type": {"sphere": {}}, "material": {"pattern": _solid([0.2, 0.4, 0.6])}}]}
    if environment is not None:
        s["environment"] = environment
    return json.dumps(s)


SKY = {"color": [0.2, 0.4, 0.8]}


@pytest.mark.parametrize("light, want", [
    (0.5, {"gain": 0.5, "samples": 1, "seed": 0}),
    (0, {"gain": 0.0, "samples": 1, "seed": 0}),
    ({}, {"gain": 1.0, "samples": 1, "seed": 0}),
    ({"samples": 64}, {"gain": 1.0, "samples": 64, "seed": 0}),
    ({"gain": 2.5, "samples": 4, "seed": 9}, {"gain": 2.5, "samples": 4, "seed": 9}),
    ({"seed": 2 ** 53}, {"gain": 1.0, "samples": 1, "seed": 2 ** 53}),
], ids=["number", "zero", "defaults", "64-samples", "every-key", "seed-2^53"])
def test_loader_reads_the_key(rtc, light, want):
    assert rtc.HostScene(_scene(dict(SKY, light=light))).sky_light() == want
    # ... and a pattern alone is a sky
    stripes = {"pattern": {"type": {"stripes": [_solid([1, 0, 0]), _solid([0, 0, 1])]}}, "color": [0, 0, 0], "light": light}
    assert rtc.HostScene(_scene(stripes)).sky_light() == want


@pytest.mark.parametrize("environment, name", [
    (dict(SKY, light={"gain": 1, "sample": 2}), "UnknownField"),
    (dict(SKY, light={"strength": 1}), "UnknownField"),
    (dict(SKY, light="on"), "InvalidData"),
    (dict(SKY, light=True), "InvalidData"),
    (dict(SKY, light=[1.0]), "InvalidData"),
    (dict(SKY, light=-0.5), "InvalidData"),
    (dict(SKY, light={"gain": -1e-9}), "InvalidData"),
    (dict(SKY, light="@1e999@"), "InvalidData"),
    (dict(SKY, light={"gain": "1"}), "InvalidData"),
    (dict(SKY, light={"samples": 0}), "InvalidData"),
    (dict(SKY, light={"samples": 65}), "InvalidData"),
    (dict(SKY, light={"samples": 2.5}), "InvalidData"),
    (dict(SKY, light={"samples": "4"}), "InvalidData"),
    (dict(SKY, light={"seed": -1}), "InvalidData"),
    (dict(SKY, light={"seed": "x"}), "InvalidData"),
    ({"light": 1.0}, "InvalidData"),
    ({"color": [0, 0, 0], "light": 1.0}, "InvalidData"),
    ({"suns": [{"direction": [0, -1, 0], "intensity": [1, 1, 1]}], "light": {"samples": 4}}, "InvalidData"),
], ids=["unknown-key", "unknown-key-alone", "string", "bool", "list", "negative", "gain-negative", "gain-inf", "gain-string", "no-samples",
        "65-samples", "samples-fraction", "samples-string", "seed-negative", "seed-string", "no-sky", "sky-of-zero", "suns-alone"])
def test_loader_refuses_a_malformed_light(rtc, environment, name):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(environment).replace('"@1e999@"', "1e999"))     # (a number that reads as +infinity)
    assert e.value.name == name, (e.value.name, str(e.value))


def test_the_key_adds_no_table_row(rtc):
    """A file with the key deleted flattens to the same tables: the light is no row of any of them."""
    import test_environment_cpu as ecpu
    scene = json.loads(open(sb.SKYLIGHT_MIX).read())
    with_light = rtc.HostScene(json.dumps(scene))
    del scene["environment"]["light"]
    bare = rtc.HostScene(json.dumps(scene))
    assert with_light.sky_light() == {"gain": 0.8, "samples": 4, "seed": 11} and bare.sky_light() is None
    assert ecpu._tables(with_light.desc) == ecpu._tables(bare.desc)
    a, b = with_light.environment(), bare.environment()
    assert a["rgb"] == b["rgb"] and a["pattern"] == b["pattern"] and np.array_equal(a["sun_direction"], b["sun_direction"])


def test_reference_scenes_and_earlier_fixtures_load_without_a_sky_light(rtc):
    """(their digests are held by the tests that held them: the loader reads one more key of "environment" and nothing else)"""
    scenes = os.path.join(REPO, "tests", "golden", "scenes")
    for name in sorted(f for f in os.listdir(scenes) if f.endswith(".json")):
        assert rtc.HostScene.from_file(name).sky_light() is None, name
    assert eb.mix(rtc).sky_light() is None and eb.box(rtc).sky_light() is None


def test_host_sky_light_is_the_table_of_rtch_scene_sky_light(rtc):
    hs = sb.mix(rtc)
    y, present = rtc.SkyLight(), C.c_int()
    rtc._check_host(rtc.host_lib().rtch_scene_sky_light(hs._h, C.byref(y), C.byref(present)))
    assert present.value == 1 and (y.gain, y.samples, y.seed) == (0.8, 4, 11)
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_sky_light(hs._h, None, None))
    rtc._check_host(rtc.host_lib().rtch_scene_sky_light(eb.mix(rtc)._h, C.byref(y), C.byref(present)))
    assert present.value == 0 and (y.gain, y.samples, y.seed) == (0.0, 1, 0)


# ---- identity: wherever the step does not run the render is the environment checker's, bit for bit
def _no_diffuse(path):
    scene = json.loads(open(path).read())
    for o in scene["objects"]:
        o.setdefault("material", {})["diffuse"] = 0
    return json.dumps(scene)


@pytest.mark.parametrize("case", ["no-table", "gain-0", "no-diffuse", "no-sky"])
@pytest.mark.parametrize("fixture", ["sky_mix", "skylight_mix"])
def test_where_the_step_does_not_run_is_the_environment_checker_bit_for_bit(rtc, fixture, case):
    path = eb.SKY_MIX if fixture == "sky_mix" else sb.SKYLIGHT_MIX
    hs = rtc.HostScene(_no_diffuse(path)) if case == "no-diffuse" else rtc.HostScene.from_file(path)
    cam = hs.camera(W, H)
    light = {"no-table": None, "gain-0": {"gain": 0.0, "samples": 4, "seed": 3}}.get(case, {"gain": 0.8, "samples": 4, "seed": 3})
    env = hs.environment()
    if case == "no-sky":
        env = dict(env, rgb=[0.0, 0.0, 0.0], pattern=rtc.ENV_NO_PATTERN)    # the suns stay
    ck = sb.scene_of(rtc, hs, sky_light=light, environment=env)
    got, c = ck.render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    want, ce = ck.render_env(cam, DEPTH, spots=hs.spots(), light_seed=3)
    assert np.array_equal(got, want)
    for k in sb.ENV_ALL:
        assert c[k] == ce[k], k
    for k in ("sky_clear", "sky_partial", "sky_blocked", "sky_deep"):
        assert c[k] == 0, k
    hits = c["primary"] + c["secondary"] - (c["miss_camera"] + c["miss_reflected"] + c["miss_refracted"] + c["miss_dark"])
    assert c["sky_skipped"] == (hits if case == "no-diffuse" else 0)


# ---- the checker against derived values (shared with tests/test_skylight_gpu.py)
SKY_C = np.array([0.25, 0.5, 0.75])
FLOOR_K, FLOOR_KD, GAIN = np.array([0.8, 0.5, 0.2]), 0.9, 1.5
FILTER_F = 0.5
OPEN = (FLOOR_K * FLOOR_KD) * (GAIN * SKY_C)


def _camera(frm, to, size=9):
    return {"width": size, "height": size, "field-of-view": 0.5, "from": list(frm), "to": list(to), "up": [0, 1, 0]}


LOOK_DOWN = _camera((0, 0.5, -0.5), (0, 0, 0))    # below the plane at height 1; every ray of the frame meets the floor


def _matte(k, kd):
    return {"pattern": _solid(k), "ambient": 0, "diffuse": kd, "specular": 0}


def _floor(**kw):
    return {"type": {"plane": {}}, "material": dict(_matte(FLOOR_K, FLOOR_KD), **kw)}


def derived_scene(objects, samples=1, sky=None, camera=LOOK_DOWN, gain=GAIN, seed=0):
    env = dict(sky if sky is not None else {"color": SKY_C.tolist()}, light={"gain": gain, "samples": samples, "seed": seed})
    return json.dumps({"camera": camera, "lights": [], "objects": list(objects), "environment": env})


def without_light(scene):
    s = json.loads(scene)
    del s["environment"]["light"]
    return json.dumps(s)


def check_derived_cases(render):
    """The derived values, for a `render(scene json, depth) -> ([9][9][3], shadow_calls)`: the checker's here, the GPU's in
    tests/test_skylight_gpu.py.  Prints each figure before it asserts."""
    def frame(name, out, want):
        delta = float(np.abs(out[0] - want).max())
        print(f"{name}: centre {out[0][4, 4]} derived {np.asarray(want)} max |delta| {delta:.3e}")
        assert delta <= TOL, (name, delta)

    # ---- an open sky: every sample is clear and adds C; L / samples = C for 1, 2 and 4 (sums of equal terms, exact)
    for n in (1, 2, 4):
        frame(f"open sky, {n} samples", render(derived_scene([_floor()], n), 5), OPEN)
    # ---- an opaque plane at height 1: a direction of the upper hemisphere has d.y > 0 (e = ng + u, |u| = 1: e.y = 1 + u.y
    # is 0 only at u = -ng, where the rule falls back to ng) and meets it: T = 0, nothing is added
    lid = {"type": {"plane": {}}, "transform": [{"translate": [0, 1, 0]}], "material": _matte([0.3, 0.3, 0.3], 0.5)}
    for n in (1, 4):
        img, _ = render(derived_scene([_floor(), lid], n), 5)
        print(f"opaque lid, {n} samples: max", float(np.abs(img).max()))
        assert not img.any()
    # ---- that plane filtering (f, f, f): a plane has one entry, every sample crosses it once
    lid["material"]["shadow-filter"] = [FILTER_F] * 3
    frame("filtering lid", render(derived_scene([_floor(), lid], 4), 5), FILTER_F * OPEN)
    # ---- a filtering sphere of radius 5 around the camera and the floor points: a ray that starts inside a sphere has its
    # two entries on either side of its origin, t1 < 0 < t2, and only the exit has et >= 0: one factor, not two
    ball = {"type": {"sphere": {}}, "transform": [{"scale": [5, 5, 5]}], "material": dict(_matte([0.3, 0.3, 0.3], 0.5), **{"shadow-filter": [FILTER_F] * 3})}
    frame("filtering sphere around", render(derived_scene([_floor(), ball], 4), 5), FILTER_F * OPEN)
    # ---- a mirror floor (diffuse 0) at depth 0 has no reflected ray and no diffuse term: nothing, and nothing is counted
    mirror = {"type": {"plane": {}}, "material": {"pattern": _solid([1, 1, 1]), "ambient": 0, "diffuse": 0, "specular": 0, "reflective": 1}}
    img, calls = render(derived_scene([mirror], 4), 0)
    assert not img.any() and calls == 0
    # ... and at depth 5 it shows the sky and still gathers nothing
    img, calls = render(derived_scene([mirror], 4), 5)
    print("mirror floor, depth 5: max |delta|", float(np.abs(img - SKY_C).max()))
    assert np.abs(img - SKY_C).max() <= TOL and calls == 0
    # ---- shadow_calls: `samples` more per hit with diffuse != 0 than the same file without the key (81 hits, no lights)
    for n in (1, 4, 64):
        scene = derived_scene([_floor(), lid], n)
        _, with_light = render(scene, 5)
        _, bare = render(without_light(scene), 5)
        print(f"{n} samples: shadow_calls {with_light} against {bare}")
        assert bare == 0 and with_light == 81 * n


def _render(rtc, scene, depth=DEPTH, sample_pass=0):
    hs = rtc.HostScene(scene)
    img, c = sb.scene_of(rtc, hs).render(hs.camera(), depth, spots=hs.spots(), sample_pass=sample_pass)
    return img, c["shadow_calls"]


def test_derived_cases_on_the_checker(rtc):
    check_derived_cases(lambda scene, depth: _render(rtc, scene, depth))


def test_every_pass_of_the_open_sky_is_the_derived_value(rtc):
    """The draws change with the pass; under a uniform sky the value does not."""
    for p in (1, 2, 7, 255):
        img, _ = _render(rtc, derived_scene([_floor()], 2), 5, sample_pass=p)
        assert np.abs(img - OPEN).max() <= TOL, p


# ---- the statistical cases: 8 x 8, 256 passes, one sample a hit: N = 16384 rays
N_PASSES, N_RAYS = 256, 8 * 8 * 256
HALVES = {"pattern": {"type": {"stripes": [_solid([1, 1, 1]), _solid([0, 0, 0])]}}}      # white for x in [0, 1), black for x in [-1, 0)
RAMP = {"pattern": {"type": {"gradient": [_solid([0, 0, 0]), _solid([1, 1, 1])]}}}       # the fraction of x: x itself on [0, 1)
BOUND_HALVES = 4 * np.sqrt(0.25 / N_RAYS)            # Bernoulli(1/2): variance 1/4; four standard errors: 0.0156
BOUND_RAMP = 4 * np.sqrt((1.0 / 18.0) / N_RAYS)      # E[cos] = 2/3, E[cos^2] = 1/2: variance 1/18; four standard errors: 0.0074
WALL = {"type": {"plane": {}}, "transform": [{"rotate-z": -HALF_PI}], "material": _matte(FLOOR_K, FLOOR_KD)}   # its normal is +x
LOOK_AT_WALL = _camera((0.7, 0, 0), (0, 0, 0), 8)


def halves_scene():
    return derived_scene([_floor()], 1, HALVES, _camera((0, 0.5, -0.5), (0, 0, 0), 8), seed=17)


def ramp_scene():
    return derived_scene([WALL], 1, RAMP, LOOK_AT_WALL, seed=23)


def check_statistical_case(name, mean_image, want, bound):
    """mean_image: the mean over the passes, [8][8][3]; every channel is K * kd * g times the same draw"""
    scale = FLOOR_K * FLOOR_KD * GAIN
    per_channel = mean_image.mean(axis=(0, 1)) / scale
    print(f"{name}: mean {per_channel} derived {want} bound {bound:.4f}")
    assert np.abs(per_channel - per_channel[0]).max() <= 1e-9          # one draw lights all three channels
    assert abs(per_channel[0] - want) <= bound, (name, per_channel[0])


def _mean_over_passes(rtc, scene):
    hs = rtc.HostScene(scene)
    ck = sb.scene_of(rtc, hs)
    total = np.zeros((8, 8, 3))
    for p in range(N_PASSES):
        total += ck.render(hs.camera(), DEPTH, spots=hs.spots(), sample_pass=p, threads=1)[0]
    return total / N_PASSES


def test_half_the_rays_of_a_floor_see_the_white_half_of_the_sky(rtc):
    """By the symmetry of the rule in x a ray's sky value is Bernoulli(1/2)."""
    assert abs(BOUND_HALVES - 0.0156) < 1e-4
    check_statistical_case("halves", _mean_over_passes(rtc, halves_scene()), 0.5, BOUND_HALVES)


def test_the_mean_cosine_of_a_walls_rays_is_two_thirds(rtc):
    """Under a sky whose value is x a ray of a wall with normal +x sees its own cosine; the density is cos / pi:
    E[cos] = int cos^2 / pi = 2/3, E[cos^2] = 1/2."""
    assert abs(BOUND_RAMP - 0.0074) < 1e-4
    check_statistical_case("ramp", _mean_over_passes(rtc, ramp_scene()), 2.0 / 3.0, BOUND_RAMP)


# ---- counts and draws
def test_counts_with_the_sky_light(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    img1, c1 = sb.scene_of(rtc, hs).render(cam, DEPTH, spots=hs.spots())
    img0, c0 = sb.scene_of(rtc, hs, sky_light=None).render(cam, DEPTH, spots=hs.spots())
    for k in sb.ENV_ALL:
        if k != "shadow_calls":
            assert c1[k] == c0[k], k
    hits = c1["primary"] + c1["secondary"] - (c1["miss_camera"] + c1["miss_reflected"] + c1["miss_refracted"] + c1["miss_dark"])
    assert c1["shadow_calls"] == c0["shadow_calls"] + 4 * (hits - c1["sky_skipped"])
    assert c1["sky_clear"] + c1["sky_partial"] + c1["sky_blocked"] == 4 * (hits - c1["sky_skipped"])
    assert (img1 >= img0 - TOL).all() and not np.array_equal(img1, img0)       # the sky only adds light


def test_draws_are_the_tables_own(rtc):
    """Another seed moves the image; the occlusion step's seed moves the occlusion alone: with no radius, nothing."""
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    light = hs.sky_light()
    a = sb.scene_of(rtc, hs).render(cam, DEPTH, spots=hs.spots())[0]
    b = sb.scene_of(rtc, hs, sky_light=dict(light, seed=12)).render(cam, DEPTH, spots=hs.spots())[0]
    assert not np.array_equal(a, b)
    ck = sb.SkyScene(hs.desc, hs.lights, bumps=hs.bumps(), uvs=hs.mesh_uvs(), gloss=hs.gloss(), occlusion=None,
                     filters=hs.shadow_filters(), media=hs.media(), environment=hs.environment(), sky_light=light)
    c = ck.render(cam, DEPTH, spots=hs.spots())[0]
    occl = dict(hs.occlusion(), radius=np.zeros(hs.desc.n_materials), seed=99)
    ck2 = sb.SkyScene(hs.desc, hs.lights, bumps=hs.bumps(), uvs=hs.mesh_uvs(), gloss=hs.gloss(), occlusion=occl,
                      filters=hs.shadow_filters(), media=hs.media(), environment=hs.environment(), sky_light=light)
    assert np.array_equal(ck2.render(cam, DEPTH, spots=hs.spots())[0], c)


# ---- the fixture
def test_fixture_meets_its_conditions(rtc):
    hs = sb.mix(rtc)
    assert os.path.getsize(sb.SKYLIGHT_MIX) < 8192
    e = hs.environment()
    assert e["pattern"] != rtc.ENV_NO_PATTERN and len(e["sun_rgb"]) == 1 and hs.lights.n_lights == 1
    assert hs.sky_light() == {"gain": 0.8, "samples": 4, "seed": 11}
    assert hs.occlusion() is not None and (np.asarray(hs.occlusion()["radius"]) > 0).any()
    assert hs.shadow_filters() is not None and hs.bumps() is not None
    kinds = [int(hs.desc.leaf_kind[i]) for i in range(hs.desc.n_leaves)]
    assert rtc.RTC_TORUS in kinds and rtc.RTC_PLANE in kinds and rtc.RTC_CUBE in kinds
    scene = json.loads(open(sb.SKYLIGHT_MIX).read())
    assert any(o.get("casts-shadow") is False for o in scene["objects"])
    assert any(o["material"].get("diffuse") == 0.0 and o["material"].get("reflective", 0) > 0 for o in scene["objects"])
    img, c = sb.scene_of(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    print({k: c[k] for k in sb.SKY_COUNTERS})
    for k in sb.SKY_COUNTERS:
        assert c[k] > 0, k
    assert img.std() > 0.05


# ---- documents and build
def test_header_states_the_contract():
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("L = (0.0, 0.0, 0.0)", "for k = 0 .. samples - 1:", "if T != (0, 0, 0):", "L.c = L.c + T.c * E.c", "G.c = gain * (L.c / double(samples))",
                 "s.c = s.c + (color.c * material.diffuse) * G.c", "key = rtc_mix64(seed ^ 0x082EFA98EC4E6C89)", "(k << 17) | code",
                 "not the bumped shading normal", "no pi and no cosine appear", "adds `samples` to shadow_calls and to shadow_traced",
                 "Sky-light rays are a third kind", "librtc_multi renders without it"):
        assert line in header, line


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 25." in design
    for word in ("rtc_scene_set_sky_light", "rtc_render_kernel_skyl", "rtc_render_kernel_skyl_bigworld", "sky_light_kernels", "pattern_at_shared",
                 "occl_direction", "SunVisitor", "tests/cpp/skylight_oracle.cpp", "profiles/skylight/disassembly_identity.txt",
                 "profiles/skylight/times_1080p_depth5.txt", "skylight_mix.json", "Out of scope"):
        assert word in design, word
    path = os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")
    if os.path.exists(path):   # (a built tree: DESIGN's resources rows of the new kernels are the build's)
        resources = json.load(open(path))
        for name in ("rtc_render_kernel_skyl", "rtc_render_kernel_skyl_bigworld"):
            k = resources.get("kernels", resources)[name]
            assert f"| `{name}` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} | {k['lds_bytes_per_block']} |" in design, name
            assert k["lds_bytes_per_block"] == resources.get("kernels", resources)[name.replace("_skyl", "_env")]["lds_bytes_per_block"]
    hs_counts = [w for w in ("sky_clear", "sky_partial", "sky_blocked", "sky_skipped", "sky_deep") if w not in design]
    assert not hs_counts, hs_counts
    for doc, word in (("README.md", "rtc_scene_set_sky_light"), ("INTEGRATION.md", "rtc_scene_set_sky_light"), ("INTEGRATION.md", "RtcSkyLight"),
                      (os.path.join("tools", "README.md"), "--sky-light"), (os.path.join("profiles", "HISTORY.md"), "sky light")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)


def test_disassembly_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "skylight", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_kernels_ext.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_meshuv.o", "rtc_gloss.o",
                "rtc_occlusion.o", "rtc_shadowfilter.o", "rtc_media.o", "rtc_environment.o", "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_skyl", "rtc_render_kernel_skyl_bigworld", "rtc_render_kernel_env", "rtc_render_kernel_env_bigworld"):
        assert kernel in text


def test_build_wires_the_new_unit():
    make = open(os.path.join(REPO, "Makefile")).read()
    for word in ("rtc_skylight.o", "rtc_skylight.remarks", "libskylight_oracle.so"):
        assert word in make, word
    unit = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_skylight.hip")).read()
    for word in ("#define RTC_SKYL_TU", "#define RTC_ENV_TU", "#define RTC_MEDIA_TU", "#define RTC_SFILT_TU", "#define RTC_OCCL_TU",
                 "#define RTC_GLOSS_TU", "#define RTC_MESHUV_TU", "#define RTC_TORUS_TU", '#include "rtc_kernels.hip"'):
        assert word in unit, word
    kernels = open(os.path.join(REPO, "ray-tracer-challenge_amd", "csrc", "rtc_kernels.hip")).read()
    assert "static_assert(!SKYL || ENV" in kernels
    assert kernels.count("pattern_at_shared(") == 3   # its definition and two call sites: the miss and the sky light
