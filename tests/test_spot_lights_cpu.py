"""Spot lights without a GPU: the ABI of rtc_scene_set_spots and its validation, the loader's "spot-light" and
rtch_scene_spots, the cone's factor against an independent restatement, and the checker (tests/cpp/spot_oracle.cpp)
against the motion checker it stacks on and against two scenes whose answer is known analytically."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import camera_binding as cb
import spot_binding as sb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT_MIX = os.path.join(REPO, "tests", "golden", "spot_scenes", "spot_mix.json")
SENTINEL = 1 << 16


def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


def _one(cone=1, axis=(0.0, -1.0, 0.0), ci=0.9, co=0.8):
    return {"cone": [cone], "axis": [list(axis)], "cos_inner": [ci], "cos_outer": [co]}


# ---- the symbols
def test_symbols_are_exported(rtc):
    assert "rtc_scene_set_spots" in rtc.RTC_SYMBOLS
    assert "rtch_scene_spots" in rtc.HOST_SYMBOLS
    assert rtc.hip_lib().rtc_scene_set_spots is not None
    assert rtc.host_lib().rtch_scene_spots is not None
    assert C.sizeof(rtc.Spot) == 40
    assert [rtc.Spot.cone.offset, rtc.Spot.axis.offset, rtc.Spot.cos_inner.offset, rtc.Spot.cos_outer.offset] == [8, 16, 24, 32]
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_spots(rtc_scene *scene, const rtc_spot *spots);" in text
    assert "#define RTC_ABI_VERSION 3u" in text   # (the description and the ABI version stay as they were)
    assert "a spot light makes no isShadowed call at a point outside its cone" in text


# ---- rtc_scene_set_spots: refused before anything changes
def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    sp, _keep = rtc.spot_struct(_one())
    assert _status(lib, lib.rtc_scene_set_spots(None, C.byref(sp))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_spots(None, None)) == "InvalidArgument"


@pytest.mark.parametrize("spots, words", [
    (_one(cone=2), "cone flag"),
    (_one(cone=255), "cone flag"),
    (_one(axis=(np.nan, -1.0, 0.0)), "not finite"),
    (_one(axis=(0.0, -np.inf, 0.0)), "not finite"),
    (_one(ci=np.nan), "not finite"),
    (_one(co=-np.inf), "not finite"),
    (_one(axis=(0.0, 0.0, 0.0)), "magnitude"),
    (_one(axis=(1e200, 1e200, 0.0)), "magnitude"),     # (finite components, an infinite magnitude)
    (_one(axis=(1e-200, 0.0, 0.0)), "magnitude"),      # (its square underflows: magnitude zero)
    (_one(ci=1.5, co=0.5), "-1 to 1"),
    (_one(ci=0.5, co=-1.0000000000000002), "-1 to 1"),
    (_one(ci=0.5, co=0.6), "above cos_inner"),
    (_one(ci=0.5, co=np.nextafter(0.5, 1.0)), "above cos_inner"),
], ids=["flag2", "flag255", "nan-axis", "inf-axis", "nan-inner", "inf-outer", "zero-axis", "huge-axis", "tiny-axis", "inner>1",
        "outer<-1", "outer>inner", "outer>inner-1ulp"])
def test_setter_rejects_an_invalid_entry_and_touches_nothing(rtc, spots, words):
    """The table's own values are checked before its count against the handle: the stand-in's light count reads as
    0xA5A5A5A5, so each of these is refused for its own reason.  (A cone on an area light is refused on a real handle, in
    test_spot_lights_gpu.py.)"""
    lib = rtc.hip_lib()
    handle = _stand_in()
    sp, _keep = rtc.spot_struct(spots)
    st = lib.rtc_scene_set_spots(C.cast(handle, C.c_void_p), C.byref(sp))
    assert _status(lib, st) == "InvalidArgument"
    assert words in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


@pytest.mark.parametrize("n_lights", [0, 1, 7])
def test_setter_rejects_a_wrong_light_count_and_touches_nothing(rtc, n_lights):
    lib = rtc.hip_lib()
    handle = _stand_in()
    spots = {"cone": np.ones(n_lights, dtype=np.uint8), "axis": np.tile([0.0, -1.0, 0.0], (n_lights, 1)),
             "cos_inner": np.full(n_lights, 0.9), "cos_outer": np.full(n_lights, 0.8)}
    sp, _keep = rtc.spot_struct(spots)
    st = lib.rtc_scene_set_spots(C.cast(handle, C.c_void_p), C.byref(sp))
    assert _status(lib, st) == "InvalidArgument"
    assert "n_lights" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


def test_spot_kernels_is_an_option(rtc):
    rtc.set_option("spot_kernels", 1)
    rtc.set_option("spot_kernels", 0)


# ---- the loader
def _scene(light, objects=None):
    cam = {"width": 40, "height": 20, "field-of-view": 1.0, "from": [0, 1.5, -5], "to": [0, 1, 0], "up": [0, 1, 0]}
    return json.dumps({"camera": cam, "lights": [light], "objects": objects or [{"type": {"plane": {}}}]})


def _spot(**kw):
    cfg = {"position": [0, 4, 0], "intensity": [1, 1, 1], "to": [0, 0, 0], "outer-angle": 0.5}
    cfg.update(kw)
    return {"spot-light": {k: v for k, v in cfg.items() if v is not None}}


def test_loader_reads_the_fixture(rtc):
    hs = rtc.HostScene.from_file(SPOT_MIX)
    sp = hs.spots()
    L = hs.lights
    assert L.n_lights == 4
    assert [L.kind[i] for i in range(4)] == [rtc.RTC_LIGHT_POINT] * 3 + [rtc.RTC_LIGHT_AREA]
    # a spot is reported as the point light it is: its position and intensity
    assert [L.corner[k] for k in range(3)] == [-2, 5, -2] and [L.rgb[k] for k in range(3)] == [0.9, 0.8, 0.7]
    assert list(sp["cone"]) == [1, 1, 0, 0]
    assert np.array_equal(sp["axis"][0], [1.0, -5.0, 2.5])            # "to" - position
    assert np.array_equal(sp["axis"][1], [-0.6, -1.0, 0.7])           # "direction"
    assert sp["cos_inner"][0] == sp["cos_outer"][0] == math.cos(0.45)  # (no inner-angle: a hard edge)
    assert sp["cos_inner"][1] == math.cos(0.25) and sp["cos_outer"][1] == math.cos(0.5)


def test_loader_without_spots_has_none(rtc):
    assert rtc.HostScene(_scene({"point-light": {"position": [0, 4, 0], "intensity": [1, 1, 1]}})).spots() is None


def test_loader_reads_the_extreme_angles(rtc):
    sp = rtc.HostScene(_scene(_spot(**{"outer-angle": math.pi, "inner-angle": 0}))).spots()
    assert sp["cos_outer"][0] == -1.0 and sp["cos_inner"][0] == 1.0


@pytest.mark.parametrize("kw, key", [
    ({"colour": [1, 1, 1]}, "spot-light.colour"),
    ({"direction": [0, -1, 0]}, "spot-light"),                 # both "to" and "direction"
    ({"to": None}, "spot-light"),                              # neither
    ({"to": [0, 4, 0]}, "spot-light.to"),                      # to == position
    ({"to": None, "direction": [0, 0, 0]}, "spot-light.direction"),
    ({"outer-angle": 0}, "spot-light.outer-angle"),
    ({"outer-angle": -0.2}, "spot-light.outer-angle"),
    ({"outer-angle": 3.2}, "spot-light.outer-angle"),
    ({"outer-angle": None}, "spot-light.outer-angle"),
    ({"inner-angle": 0.6}, "spot-light.inner-angle"),
    ({"inner-angle": -0.1}, "spot-light.inner-angle"),
    ({"to": [0, 1]}, "to"),
    ({"to": None, "outer-angle": None}, "UnknownField: light.spot-light"),   # no cone at all
    ({"intensity": None}, "spot-light.intensity"),
], ids=["unknown", "both", "neither", "to-is-position", "zero-direction", "outer0", "outer-neg", "outer>pi", "no-outer",
        "inner>outer", "inner-neg", "short-to", "no-cone", "no-intensity"])
def test_loader_refuses_a_malformed_spot_light(rtc, kw, key):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(_spot(**kw)))
    assert key in str(e.value)


def test_host_spots_needs_the_light_count(rtc):
    hs = rtc.HostScene.from_file(SPOT_MIX)
    z = np.zeros(16)
    c = np.zeros(5, dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_spots(hs._h, c.ctypes.data_as(C.POINTER(C.c_uint8)), z.ctypes.data_as(dp),
                                                         z.ctypes.data_as(dp), z.ctypes.data_as(dp), 5))


# ---- the cone's factor: an independent restatement, bit for bit
def _factor(c, ci, co):
    c, ci, co = np.float64(c), np.float64(ci), np.float64(co)
    if c >= ci:
        return np.float64(1.0)
    if c <= co:
        return np.float64(0.0)
    s = (c - co) / (ci - co)
    return (s * s) * (np.float64(3.0) - np.float64(2.0) * s)


def _operands():
    up, down = (lambda x: np.nextafter(x, 2.0)), (lambda x: np.nextafter(x, -2.0))
    out = []
    for ci, co in [(0.9, 0.8), (math.cos(0.25), math.cos(0.5)), (0.5, 0.5), (1.0, -1.0), (-0.3, -0.9), (1.0, 1.0), (-1.0, -1.0),
                   (0.7, down(0.7))]:
        for c in (ci, co, up(ci), down(ci), up(co), down(co), (ci + co) / 2, -1.0, 1.0, 0.0):
            out.append((c, ci, co))
        w = ci - co
        for t in (1e-15, 1e-9, 1e-3, 0.25, 0.5, 0.75, 1 - 1e-3, 1 - 1e-9, 1 - 1e-15):   # s near 0 and near 1
            out.append((co + t * w, ci, co))
    rng = np.random.default_rng(16)
    for _ in range(2000):
        a, b = np.sort(rng.uniform(-1, 1, 2))
        out.append((rng.uniform(-1, 1), b, a))
    return out


def test_factor_matches_a_restatement_bitwise():
    ops = _operands()
    got = np.array([sb.factor(*o) for o in ops])
    want = np.array([_factor(*o) for o in ops])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all((got >= 0.0) & (got <= 1.0))


def test_factor_edges():
    assert sb.factor(0.9, 0.9, 0.8) == 1.0 and sb.factor(0.8, 0.9, 0.8) == 0.0
    assert sb.factor(0.5, 0.5, 0.5) == 1.0 and sb.factor(np.nextafter(0.5, 0.0), 0.5, 0.5) == 0.0
    assert 0.0 < sb.factor(np.nextafter(0.8, 1.0), 0.9, 0.8) < 1e-20
    assert 1.0 - 1e-12 < sb.factor(np.nextafter(0.9, 0.0), 0.9, 0.8) <= 1.0   # (one ulp inside: the smoothstep's own 1)


# ---- the checker
def test_checker_without_cones_is_the_motion_checker(rtc):
    hs = rtc.HostScene.from_file(SPOT_MIX)
    cam = hs.camera(48, 27)
    S = sb.SpotScene(hs.desc, hs.lights)
    for smp in (None, cb.sampling(2, True, aperture=0.05, focal_distance=5.0, seed=3)):
        disp = np.zeros((hs.desc.n_roots, 3))
        disp[1] = (0.4, 0.0, 0.2)
        got, c, edge = S.render(cam, 5, smp, spots=sb.no_cones(hs.lights.n_lights), disp=disp, light_seed=7)
        want, cw = S.render_motion(cam, 5, smp, disp=disp, light_seed=7)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert c == cw and not edge.any()


def _top_camera(rtc, w, h):
    """straight down from (0, 10, 0) onto the floor"""
    return rtc.make_camera(w, h, 1.2, (0, 10, 0), (0, 0, 0), (0, 0, 1))


def _floor_points(cam):
    """the floor point (y = 0) of every pixel's centred ray (Camera.rayForPixel)"""
    inv = np.array(cam.inv_view[:]).reshape(4, 4)
    xs = (np.arange(cam.hsize) + 0.5) * cam.pixel_size
    ys = (np.arange(cam.vsize) + 0.5) * cam.pixel_size
    wx, wy = np.meshgrid(cam.half_width - xs, cam.half_height - ys)
    pix = np.stack([wx, wy, -np.ones_like(wx), np.ones_like(wx)], -1) @ inv.T
    origin = inv @ np.array([0.0, 0.0, 0.0, 1.0])
    d = pix[..., :3] - origin[:3]
    t = -origin[1] / d[..., 1]
    return origin[:3] + d * t[..., None]


FLOOR = [{"type": {"plane": {}}, "material": {"pattern": {"type": {"solid": [1, 1, 1]}}, "ambient": 0.1, "diffuse": 0.9, "specular": 0}}]


def test_hard_spot_straight_down_lights_its_disc_only(rtc):
    height, outer = 4.0, 0.5
    hs = rtc.HostScene(_scene({"spot-light": {"position": [0, height, 0], "intensity": [1, 1, 1], "direction": [0, -1, 0],
                                              "outer-angle": outer}}, FLOOR))
    cam = _top_camera(rtc, 64, 48)
    img, counters, edge = sb.SpotScene(hs.desc, hs.lights).render(cam, 5, spots=hs.spots())
    p = _floor_points(cam)
    angle = np.arctan2(np.hypot(p[..., 0], p[..., 2]), height)
    outside, inside = angle > outer + 0.01, angle < outer - 0.01
    assert outside.sum() > 100 and inside.sum() > 100
    assert np.all(img[outside] == 0.1)            # ambient alone, to the bit
    assert np.all(img[inside] > 0.1 + 1e-3)
    assert counters["shadow_calls"] < cam.hsize * cam.vsize
    assert not edge[outside | inside].any()


def test_a_cone_around_everything_is_the_point_light(rtc):
    objects = FLOOR + [{"type": {"sphere": {}}, "transform": [{"translate": [0.5, 1, 0.3]}],
                        "material": {"pattern": {"type": {"solid": [0.8, 0.3, 0.2]}}, "reflective": 0.3}}]
    light = {"point-light": {"position": [0, 50, 0], "intensity": [1, 1, 1]}}
    hs = rtc.HostScene(_scene(light, objects))
    cam = _top_camera(rtc, 48, 36)
    S = sb.SpotScene(hs.desc, hs.lights)
    plain, cp, _ = S.render(cam, 5)
    for ci, co in [(math.cos(1.2), math.cos(1.3)), (-1.0, -1.0)]:
        spots = {"cone": [1], "axis": [[0, -1, 0]], "cos_inner": [ci], "cos_outer": [co]}
        got, c, _ = S.render(cam, 5, spots=spots)
        assert np.array_equal(got.view(np.uint64), plain.view(np.uint64))
        assert c == cp


def test_a_narrow_spot_makes_fewer_shadow_calls(rtc):
    hs = rtc.HostScene.from_file(SPOT_MIX)
    cam = hs.camera(48, 27)
    S = sb.SpotScene(hs.desc, hs.lights)
    spotted, c1, _ = S.render(cam, 5, spots=hs.spots())
    plain, c0, _ = S.render(cam, 5)
    assert c1["primary"] == c0["primary"] and c1["secondary"] == c0["secondary"]
    assert c1["shadow_calls"] < c0["shadow_calls"]
    assert spotted.sum() < plain.sum()


def test_checker_refuses_a_cone_on_an_area_light(rtc):
    hs = rtc.HostScene.from_file(SPOT_MIX)
    spots = sb.no_cones(4)
    spots["cone"][3] = 1
    spots["axis"][3] = (0, -1, 0)
    with pytest.raises(RuntimeError):
        sb.SpotScene(hs.desc, hs.lights).render(hs.camera(8, 8), 5, spots=spots)
