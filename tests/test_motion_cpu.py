"""Motion blur without a GPU: the ABI of rtc_scene_set_motion and its validation, the loader's "motion" and
rtch_scene_motion, the shutter-time hash against an independent restatement, the fixture scene, and the checker
(tests/cpp/motion_oracle.cpp) against the static checkers and against a static sphere moved by its transform."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import camera_binding as cb
import motion_binding as mb
import progressive_binding as pb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION_MIX = os.path.join(REPO, "tests", "golden", "motion_scenes", "motion_mix.json")
SOFT_SHADOWS = os.path.join(REPO, "tests", "golden", "area_scenes", "soft_shadows.json")
SENTINEL = 1 << 16
M64 = (1 << 64) - 1


def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


# ---- the symbols
def test_symbols_are_exported(rtc):
    assert "rtc_scene_set_motion" in rtc.RTC_SYMBOLS
    assert "rtch_scene_motion" in rtc.HOST_SYMBOLS
    assert rtc.hip_lib().rtc_scene_set_motion is not None
    assert rtc.host_lib().rtch_scene_motion is not None
    assert C.sizeof(rtc.Motion) == 16 and rtc.Motion.displacement.offset == 8
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "int rtc_scene_set_motion(rtc_scene *scene, const rtc_motion *motion);" in text
    assert "#define RTC_ABI_VERSION 3u" in text   # (the description and the ABI version stay as they were)


# ---- rtc_scene_set_motion: refused before anything changes
def test_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    d = (C.c_double * 3)(1.0, 0.0, 0.0)
    m = rtc.Motion(1, C.cast(d, C.POINTER(C.c_double)))
    assert _status(lib, lib.rtc_scene_set_motion(None, C.byref(m))) == "InvalidArgument"
    assert _status(lib, lib.rtc_scene_set_motion(None, None)) == "InvalidArgument"


@pytest.mark.parametrize("n_roots", [0, 1, 7, 1 << 20])
def test_setter_rejects_a_wrong_root_count_and_touches_nothing(rtc, n_roots):
    """The stand-in's root count reads as 0xA5A5A5A5: no count below it matches.  (Non-finite values and NULL are tested
    on a real handle in test_motion_gpu.py.)"""
    lib = rtc.hip_lib()
    handle = _stand_in()
    d = np.zeros((max(n_roots, 1), 3))
    m = rtc.Motion(n_roots, d.ctypes.data_as(C.POINTER(C.c_double)))
    st = lib.rtc_scene_set_motion(C.cast(handle, C.c_void_p), C.byref(m))
    assert _status(lib, st) == "InvalidArgument"
    assert "n_roots" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


# ---- the loader
def _scene(objects):
    cam = {"width": 40, "height": 20, "field-of-view": 1.0, "from": [0, 1.5, -5], "to": [0, 1, 0], "up": [0, 1, 0]}
    return json.dumps({"camera": cam, "lights": [{"point-light": {"position": [-10, 10, -10], "intensity": [1, 1, 1]}}],
                       "objects": objects})


SPHERE = {"type": {"sphere": {}}}


def test_loader_reads_motion_of_top_level_objects(rtc):
    hs = rtc.HostScene(_scene([SPHERE, dict(SPHERE, motion=[0.5, -1, 2.25]), {"type": {"group": [SPHERE]}, "motion": [0, 0, 3]}]))
    assert np.array_equal(hs.motion(), [[0, 0, 0], [0.5, -1, 2.25], [0, 0, 3]])
    assert np.array_equal(rtc.HostScene(_scene([SPHERE])).motion(), [[0, 0, 0]])


def test_loader_reads_the_fixture(rtc):
    hs = rtc.HostScene.from_file(MOTION_MIX)
    m = hs.motion()
    assert m.shape == (hs.desc.n_roots, 3) == (5, 3)
    moving = [r for r in range(5) if np.any(m[r] != 0)]
    assert moving == [1, 2, 3, 4]
    roots = hs.array("roots", hs.desc.n_roots)
    child_node = 1 << 31
    # a moving sphere, a moving group, a moving csg unit (a node), and the glass sphere
    assert roots[1] & child_node == 0 and roots[2] & child_node and roots[3] & child_node


@pytest.mark.parametrize("objects", [
    [{"type": {"group": [dict(SPHERE, motion=[1, 0, 0])]}}],
    [{"type": {"csg": {"operation": "union", "left": dict(SPHERE, motion=[1, 0, 0]), "right": SPHERE}}}],
    [{"type": {"group": [{"type": {"group": [dict(SPHERE, motion=[0, 1, 0])]}}]}}],
])
def test_loader_refuses_motion_below_the_top_level(rtc, objects):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(objects))
    assert e.value.name == "InvalidData"
    assert '"motion"' in str(e.value)


def test_loader_refuses_motion_in_a_definition(rtc):
    scene = json.loads(_scene([{"type": {"from-definition": "ball"}}]))
    scene["shape-definitions"] = [{"name": "ball", "value": dict(SPHERE, motion=[1, 0, 0])}]
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(json.dumps(scene))
    assert '"motion"' in str(e.value)


@pytest.mark.parametrize("motion", [[1, 0], [1, 0, 0, 0], "fast", [1, "0", 0]])
def test_loader_refuses_a_malformed_motion(rtc, motion):
    with pytest.raises(rtc.RtcError):
        rtc.HostScene(_scene([dict(SPHERE, motion=motion)]))


def test_host_motion_needs_the_root_count(rtc):
    hs = rtc.HostScene(_scene([SPHERE, SPHERE]))
    out = np.zeros(9)
    with pytest.raises(rtc.RtcError):
        rtc._check_host(rtc.host_lib().rtch_scene_motion(hs._h, out.ctypes.data_as(C.POINTER(C.c_double)), 3))


# ---- the shutter time: an independent restatement of DESIGN.md section 14
def _mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _time(seed, p, g):
    key = _mix(seed ^ 0x243F6A8885A308D3)
    c = ((p << 32) | (g << 8) | 255) & M64
    return (_mix((key + 0x9E3779B97F4A7C15 * (c + 1)) & M64) >> 11) * 2.0 ** -53


def test_time_hash_vectors():
    cases = [(0, 0, 0), (0, 1, 0), (7, 12345, 3), (1 << 40, 1920 * 1080 - 1, 15), (M64, 77, (1 << 24) - 1)]
    got = [float(mb.shutter_time(s, [p], [g])[0]) for s, p, g in cases]
    want = [_time(s, p, g) for s, p, g in cases]
    assert got == want
    assert all(0.0 <= t < 1.0 for t in got)
    # the camera hash on its own axis: not the sub-pixel offsets' or the lens's value
    assert got[2] != float(cb.camera_hash(7, [12345], [3], [0])[0])
    assert got[2] == float(cb.camera_hash(7, [12345], [3], [255])[0])


# ---- the checker
@pytest.mark.parametrize("name", [MOTION_MIX, SOFT_SHADOWS])
def test_time_zero_or_no_displacement_is_the_static_checker_bitwise(rtc, name):
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(48, 27)
    want, _ = cb.CameraScene(hs.desc, hs.lights).render(cam, 5)
    ms = mb.MotionScene(hs.desc, hs.lights)
    disp = np.tile([0.7, -0.3, 0.4], (hs.desc.n_roots, 1))
    assert np.array_equal(ms.render_at(cam, 0.0, disp), want)
    assert np.array_equal(ms.render_at(cam, 0.63, None), want)
    moved = ms.render_at(cam, 0.63, disp)
    assert not np.array_equal(moved, want)


def test_no_displacement_is_the_pass_checker_bitwise(rtc):
    hs = rtc.HostScene.from_file(MOTION_MIX)
    cam = hs.camera(40, 24)
    smp = cb.sampling(2, True, seed=9)
    for p in (0, 2):
        want, wc = pb.PassScene(hs.desc, hs.lights).render(cam, 5, smp, p)
        got, gc = mb.MotionScene(hs.desc, hs.lights).render(cam, 5, smp, None, p)
        assert np.array_equal(got, want) and gc == wc


def test_moved_sphere_is_the_translated_sphere(rtc):
    """A sphere moved by D and sampled at time t is, within 1e-12, a static sphere whose transform is translate(t D) M:
    the shifted ray is the plain geometric meaning."""
    objects = [{"type": {"plane": {}}, "material": {"pattern": {"type": {"checkers": [
                   {"type": {"solid": [1, 1, 1]}}, {"type": {"solid": [0.2, 0.2, 0.2]}}]}}}},
               {"type": {"sphere": {}}, "transform": [{"scale": [0.8, 0.6, 0.7]}, {"translate": [-0.3, 1, 0.2]}],
                "material": {"pattern": {"type": {"stripes": [{"type": {"solid": [1, 0, 0]}}, {"type": {"solid": [0, 0, 1]}}]},
                                         "transform": [{"scale": [0.1, 0.1, 0.1]}]}, "reflective": 0.3}}]
    text = _scene(objects)
    hs, moved_hs = rtc.HostScene(text), rtc.HostScene(text)
    cam = hs.camera(64, 40)
    D, t = np.array([0.6, 0.25, -0.4]), 0.37
    disp = np.array([[0, 0, 0], D])
    got = mb.MotionScene(hs.desc, hs.lights).render_at(cam, t, disp)
    # the same sphere, its transform translated by t D: inverse' = inverse . translate(-t D)
    leaf = int(moved_hs.array("roots", 2)[1])
    x = int(moved_hs.array("leaf_xform", moved_hs.desc.n_leaves)[leaf])
    assert list(moved_hs.array("leaf_xform", moved_hs.desc.n_leaves)).count(x) == 1
    inv = moved_hs.array("xf_inv", moved_hs.desc.n_xforms, 16)
    inv_t = moved_hs.array("xf_inv_t", moved_hs.desc.n_xforms, 16)
    T = np.eye(4)
    T[:3, 3] = -t * D
    m = inv[x].reshape(4, 4) @ T
    inv[x] = m.reshape(16)
    inv_t[x] = m.T.reshape(16)
    want, _ = cb.CameraScene(moved_hs.desc, moved_hs.lights).render(cam, 5)
    static, _ = cb.CameraScene(hs.desc, hs.lights).render(cam, 5)
    assert float(np.abs(got - want).max()) <= 1e-12
    assert float(np.abs(got - static).max()) > 0.1   # (the sphere did move)


def test_motion_blurs_along_the_path(rtc):
    """Many samples of a small sphere moving across black: pixels it crosses only mid-shutter are partly lit, pixels
    away from its path are black."""
    objects = [{"type": {"sphere": {}}, "transform": [{"scale": [0.3, 0.3, 0.3]}, {"translate": [-1.5, 1, 0]}], "motion": [3, 0, 0],
                "material": {"pattern": {"type": {"solid": [1, 1, 1]}}, "ambient": 1, "diffuse": 0, "specular": 0}}]
    hs = rtc.HostScene(_scene(objects))
    cam = hs.camera(40, 20)
    img, _ = mb.MotionScene(hs.desc, hs.lights).render(cam, 5, cb.sampling(4, True, seed=1), hs.motion())
    row = img[cam.vsize // 2 - 1, :, 0]
    mid = row[cam.hsize // 2 - 2:cam.hsize // 2 + 2]
    assert np.all((mid > 0.0) & (mid < 1.0))
    assert np.all(img[:2] == 0.0) and np.all(img[-2:] == 0.0)
