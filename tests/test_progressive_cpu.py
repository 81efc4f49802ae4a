"""Progressive rendering without a GPU: the ABI of rtc_scene_set_sample_pass and rtc_scene_accumulate_device and their
validation, the loader's "passes", the pass's hash keys against an independent restatement, and the checker
(tests/cpp/progressive_oracle.cpp) against the camera-sampling checker and an edge's analytic coverage."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import camera_binding as cb
import progressive_binding as pb
import test_sampling_cpu as sampling_cpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = os.path.join(REPO, "tests", "golden", "scenes", "cover.json")
SOFT_SHADOWS = os.path.join(REPO, "tests", "golden", "area_scenes", "soft_shadows.json")
SENTINEL = 1 << 16


def _stand_in():
    """A stand-in handle: a block of sentinel bytes, which no GPU is needed for."""
    return (C.c_uint8 * SENTINEL)(*([0xA5] * SENTINEL))


def _status(lib, st):
    return lib.rtc_status_name(st).decode()


# ---- the symbols
def test_symbols_are_exported(rtc):
    assert {"rtc_scene_set_sample_pass", "rtc_scene_accumulate_device"} <= set(rtc.RTC_SYMBOLS)
    assert "rtch_scene_passes" in rtc.HOST_SYMBOLS
    assert rtc.hip_lib().rtc_scene_set_sample_pass is not None
    assert rtc.hip_lib().rtc_scene_accumulate_device is not None
    assert rtc.host_lib().rtch_scene_passes is not None
    # frame, n_pixels, passes (+ 4 bytes of padding), sum, sumsq, mean, rgba, noise
    assert C.sizeof(rtc.Accum) == 64
    assert (rtc.Accum.n_pixels.offset, rtc.Accum.passes.offset, rtc.Accum.sum.offset, rtc.Accum.noise.offset) == (8, 16, 24, 56)
    text = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "#define RTC_SAMPLING_INDEX_LIMIT 16777216u" in text
    assert rtc.RTC_SAMPLING_INDEX_LIMIT == 1 << 24


# ---- rtc_scene_set_sample_pass
def test_pass_setter_rejects_a_null_handle(rtc):
    lib = rtc.hip_lib()
    for p in (0, 1, 65535, 65536):
        assert _status(lib, lib.rtc_scene_set_sample_pass(None, p)) == "InvalidArgument"


@pytest.mark.parametrize("p", [65536, 1 << 24, (1 << 32) - 1])
def test_pass_setter_rejects_and_touches_nothing(rtc, p):
    """Passes past the limit at any grid (the stand-in's sample count reads as far more than one) are refused before the
    handle changes.  (grid 16's edge, 65535 accepted and 65536 refused, is tested on a real handle in
    test_progressive_gpu.py.)"""
    lib = rtc.hip_lib()
    handle = _stand_in()
    st = lib.rtc_scene_set_sample_pass(C.cast(handle, C.c_void_p), p)
    assert _status(lib, st) == "InvalidArgument"
    assert "sample pass" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


# ---- rtc_scene_accumulate_device: every invalid argument is refused before the device is touched
FAKE = 0x7F0000001000   # (never dereferenced: validation comes first)
GOOD = dict(frame=FAKE, n_pixels=100, passes=3, sum=FAKE + 0x1000, sumsq=FAKE + 0x2000, mean=None, rgba=None,
            noise=FAKE + 0x3000)
BAD = [dict(frame=None), dict(sum=None), dict(n_pixels=0), dict(n_pixels=(1 << 40) + 1), dict(passes=0),
       dict(sumsq=None), dict(passes=1), dict(passes=1, sumsq=None)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_accumulate_rejects_each_invalid_argument(rtc, bad):
    lib = rtc.hip_lib()
    v = dict(GOOD)
    v.update(bad)
    a = rtc.Accum(v["frame"], v["n_pixels"], v["passes"], v["sum"], v["sumsq"], v["mean"], v["rgba"], v["noise"])
    handle = _stand_in()
    st = lib.rtc_scene_accumulate_device(C.cast(handle, C.c_void_p), C.byref(a), None)
    assert _status(lib, st) == "InvalidArgument"
    assert "accumulate" in lib.rtc_last_error().decode()
    assert bytes(handle) == b"\xa5" * SENTINEL


def test_accumulate_rejects_null_handle_and_struct(rtc):
    lib = rtc.hip_lib()
    v = GOOD
    a = rtc.Accum(v["frame"], v["n_pixels"], v["passes"], v["sum"], v["sumsq"], v["mean"], v["rgba"], v["noise"])
    assert _status(lib, lib.rtc_scene_accumulate_device(None, C.byref(a), None)) == "InvalidArgument"
    handle = _stand_in()
    assert _status(lib, lib.rtc_scene_accumulate_device(C.cast(handle, C.c_void_p), None, None)) == "InvalidArgument"
    assert bytes(handle) == b"\xa5" * SENTINEL


# ---- the loader
def _scene(sampling=None):
    cam = {"width": 40, "height": 20, "field-of-view": 1.0, "from": [0, 1.5, -5], "to": [0, 1, 0], "up": [0, 1, 0]}
    if sampling is not None:
        cam["sampling"] = sampling
    return json.dumps({"camera": cam, "lights": [{"point-light": {"position": [-10, 10, -10], "intensity": [1, 1, 1]}}],
                       "objects": [{"type": {"sphere": {}}}]})


def test_loader_passes_default_to_one(rtc):
    for sampling in (None, {}, {"grid": 3, "jitter": True}):
        assert rtc.HostScene(_scene(sampling)).passes() == 1


def test_loader_reads_passes(rtc):
    hs = rtc.HostScene(_scene({"grid": 2, "jitter": True, "seed": 3, "passes": 16}))
    assert hs.passes() == 16
    assert hs.sampling().grid == 2 and hs.sampling().seed == 3
    assert rtc.HostScene(_scene({"passes": 1 << 24})).passes() == 1 << 24            # grid 1: the whole index range
    assert rtc.HostScene(_scene({"grid": 16, "passes": 65536})).passes() == 65536     # grid 16: passes 0 .. 65535


@pytest.mark.parametrize("sampling, error", [
    ({"passes": 0}, "InvalidData"), ({"passes": (1 << 24) + 1}, "InvalidData"), ({"grid": 16, "passes": 65537}, "InvalidData"),
    ({"grid": 4, "passes": (1 << 20) + 1}, "InvalidData"), ({"passes": 2.5}, "InvalidNumber"), ({"passes": -1}, "Overflow"),
    ({"passes": "4"}, "UnexpectedToken"), ({"passes": True}, "UnexpectedToken"),
])
def test_loader_rejects(rtc, sampling, error):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene(sampling))
    assert e.value.name == error


# ---- the pass's keys: an independent restatement of DESIGN.md section 13
M64 = (1 << 64) - 1


def test_pass_hash_vectors():
    """Sample k of pass P (S samples a pass) hashes the global index P * S + k; pass 0 is the camera hash of section 12."""
    cases = [(0, 0, 0, 1, 0, 0), (7, 1920 * 540 + 960, 3, 4, 1, 1), (2 ** 64 - 1, 2 ** 31 + 5, 65535, 256, 255, 63),
             (123456789, 3, 1, 1, 0, 2), (5, 77, (1 << 24) - 1, 1, 0, 0)]
    for seed, p, P, S, k, axis in cases:
        g = P * S + k
        assert g < 1 << 24
        got = pb.pass_hash(seed, p, P, S, k, axis)
        assert got == sampling_cpu._j(seed, p, g, axis)
        if P == 0:
            assert got == cb.camera_hash(seed, [p], [k], [axis])[0]
    # passes give other draws for the same pixel, sample and axis ...
    draws = {pb.pass_hash(9, 1000, P, 4, 3, 0) for P in range(64)}
    assert len(draws) == 64
    # ... and the same draw as the sample of the same global index at another split of the index
    assert pb.pass_hash(9, 1000, 2, 4, 3, 0) == pb.pass_hash(9, 1000, 11, 1, 0, 0)


def test_area_key_vectors():
    """An area light's jitter of sample k of pixel p at pass P is keyed on (P * N + p) * S + k, u64, wrapping."""
    cases = [(0, 1920 * 1080, 5, 1, 0), (0, 1920 * 1080, 5, 4, 3), (1, 1920 * 1080, 5, 4, 3), (65535, 3840 * 2160, 3840 * 2160 - 1, 256, 255),
             ((1 << 24) - 1, 1 << 40, (1 << 40) - 1, 1, 0), (1 << 20, (1 << 44) + 3, 17, 16, 9)]
    for P, N, p, S, k in cases:
        assert pb.area_key(P, N, p, S, k) == ((P * N + p) * S + k) & M64
    assert pb.area_key(0, 100, 42, 4, 3) == 42 * 4 + 3           # pass 0: section 12's key
    assert pb.area_key((1 << 20), (1 << 44) + 3, 17, 16, 9) != ((1 << 20) * ((1 << 44) + 3) + 17) * 16 + 9   # (it wrapped)


# ---- the checker
@pytest.mark.parametrize("name, smp, light_seed", [
    (COVER, cb.sampling(2, True, aperture=0.05, focal_distance=4.0, seed=12), 0),
    (SOFT_SHADOWS, cb.sampling(1, False), 9),
    (SOFT_SHADOWS, cb.sampling(2, True, seed=1), 9),
])
def test_pass_zero_is_the_camera_checker_bitwise(rtc, name, smp, light_seed):
    hs = rtc.HostScene.from_file(name)
    cam = hs.camera(48, 27)
    chk = pb.PassScene(hs.desc, hs.lights)
    want, wc = chk.render_camera_checker(cam, 5, smp, light_seed=light_seed)
    got, c = chk.render(cam, 5, smp, 0, light_seed=light_seed)
    assert np.array_equal(got, want) and c == wc
    other, c1 = chk.render(cam, 5, smp, 1, light_seed=light_seed)
    assert not np.array_equal(other, want)              # pass 1 draws other samples ...
    assert c1["primary"] == c["primary"]                # ... as many of them


def test_default_sampling_without_jitter_repeats_its_image(rtc):
    """Under the default sampling with no jittered area light every pass renders the same image."""
    hs = rtc.HostScene.from_file(COVER)
    cam = hs.camera(32, 18)
    chk = pb.PassScene(hs.desc, hs.lights)
    first, _ = chk.render(cam, 5, None, 0)
    for P in (1, 7):
        assert np.array_equal(chk.render(cam, 5, None, P)[0], first)


def test_passes_over_an_edge_approach_its_coverage(rtc):
    """One jittered sample a pass over a slanted edge: the mean of 64 passes approaches each pixel's analytic coverage
    (the area of the pixel on the slab's side of the edge), where one pass is a staircase of 0 and 1."""
    hs = rtc.HostScene(sampling_cpu._edge_scene())
    cam = hs.camera()
    chk = pb.PassScene(hs.desc, hs.lights)
    smp = cb.sampling(1, True, seed=5)
    n = 64
    frames = [chk.render(cam, 5, smp, P)[0][:, :, 0] for P in range(n)]
    mean = frames[0].copy()
    for f in frames[1:]:
        mean = mean + f
    mean = mean / n
    # coverage: inside iff cos(t) * (9 wx - (10 + e)) + sin(t) * 9 wy >= -10 - linear in the pixel's (u, v) - on a 512 x 512 grid
    cos_t, sin_t = math.cos(sampling_cpu.EDGE_THETA), math.sin(sampling_cpu.EDGE_THETA)
    u = (np.arange(512) + 0.5) / 512
    cover = np.zeros((cam.vsize, cam.hsize))
    for y in range(cam.vsize):
        for x in range(cam.hsize):
            wx = cam.half_width - (x + u[None, :]) * cam.pixel_size
            wy = cam.half_height - (y + u[:, None]) * cam.pixel_size
            cover[y, x] = np.mean(cos_t * (9 * wx - (10 + sampling_cpu.EDGE_E)) + sin_t * 9 * wy >= -10)
    partial = (cover > 0.01) & (cover < 0.99)
    assert partial.sum() >= 5
    assert set(np.unique(frames[0])) <= {0.0, 1.0}
    err1 = np.abs(frames[0] - cover)[partial].mean()
    err64 = np.abs(mean - cover)[partial].mean()
    assert err64 < 0.06 and err64 < err1 / 3, (err1, err64)
    assert np.abs(mean - cover).max() < 0.25
    assert np.all(mean[cover == 0.0] == 0.0) and np.all(mean[cover == 1.0] == 1.0)
