"""ctypes binding of the spot-light checker (tests/build/libspot_oracle.so, tests/cpp/spot_oracle.cpp).  TEST
INFRASTRUCTURE.

The checker is the motion-blur checker with cones on point lights: same (desc, light table, camera, depth, light seed,
rtc_sampling, sample pass, displacements, spots) as rtc_scene_create_with_lights + rtc_scene_set_sampling +
rtc_scene_set_sample_pass + rtc_scene_set_motion + rtc_scene_set_spots + rtc_render -> the same [h][w][3] f64 image, the
same primary, secondary and shadow_calls counts, and per pixel whether a hard-edged cone was met within 1e-9 of its
cosine (where one rounding of the hit point decides between lit and unlit).
"""
import ctypes as C
import importlib
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT_SO = os.path.join(REPO, "tests", "build", "libspot_oracle.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        rtc = importlib.import_module("ray-tracer-challenge_amd")
        l = C.CDLL(SPOT_SO)
        l.area_last_error.restype = C.c_char_p
        l.area_scene_create.argtypes = [C.POINTER(rtc.SceneDesc), C.POINTER(rtc.LightDesc), C.POINTER(C.c_void_p)]
        l.area_scene_destroy.argtypes = [C.c_void_p]
        l.area_scene_destroy.restype = None
        l.motion_render.argtypes = ([C.c_void_p, C.POINTER(rtc.Camera), C.c_uint32, C.c_uint64, C.POINTER(rtc.Sampling), C.c_uint32,
                                     C.c_void_p, C.c_uint32] + [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p])
        l.spot_render.argtypes = ([C.c_void_p, C.POINTER(rtc.Camera), C.c_uint32, C.c_uint64, C.POINTER(rtc.Sampling), C.c_uint32,
                                   C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] * 6 + [C.c_void_p] * 3)
        l.spot_kat_factor.argtypes = [C.c_double, C.c_double, C.c_double]
        l.spot_kat_factor.restype = C.c_double
        _lib = l
    return _lib


def no_cones(n_lights):
    """Every flag 0: the lights as they are."""
    return {"cone": np.zeros(n_lights, dtype=np.uint8), "axis": np.zeros((n_lights, 3)), "cos_inner": np.ones(n_lights),
            "cos_outer": np.ones(n_lights)}


class SpotScene:
    def __init__(self, desc, lights):
        self._s = C.c_void_p()
        self._keep = (desc, lights)
        self.n_roots = desc.n_roots
        self.n_lights = lights.n_lights
        if lib().area_scene_create(C.byref(desc), C.byref(lights), C.byref(self._s)) != 0:
            raise RuntimeError("spot checker: " + lib().area_last_error().decode())

    def render(self, cam, max_depth=5, smp=None, spots=None, disp=None, sample_pass=0, light_seed=0, tile=None, threads=0):
        """-> ([h][w][3] f64, {"primary", "secondary", "shadow_calls"}, [h][w] bool hard-edge mask); smp: an rtc.Sampling
        (None: the default); spots: a dict as GpuScene.set_spots takes (None: no cones); disp: (n_roots, 3) (None: static)"""
        x0, y0, w, h = tile if tile else (0, 0, cam.hsize, cam.vsize)
        d = np.zeros((self.n_roots, 3)) if disp is None else np.ascontiguousarray(disp, dtype=np.float64)
        assert d.shape == (self.n_roots, 3)
        sp = no_cones(self.n_lights) if spots is None else spots
        cone = np.ascontiguousarray(sp["cone"], dtype=np.uint8)
        axis = np.ascontiguousarray(sp["axis"], dtype=np.float64)
        ci = np.ascontiguousarray(sp["cos_inner"], dtype=np.float64)
        co = np.ascontiguousarray(sp["cos_outer"], dtype=np.float64)
        out = np.zeros((h, w, 3), dtype=np.float64)
        edge = np.zeros((h, w), dtype=np.uint8)
        counters = np.zeros(3, dtype=np.uint64)
        smp_p = C.byref(smp) if smp is not None else None
        if lib().spot_render(self._s, C.byref(cam), max_depth, light_seed, smp_p, sample_pass, d.ctypes.data, self.n_roots,
                             cone.ctypes.data, axis.ctypes.data, ci.ctypes.data, co.ctypes.data, len(cone), x0, y0, w, h, threads,
                             out.ctypes.data, counters.ctypes.data, edge.ctypes.data) != 0:
            raise RuntimeError("spot checker: " + lib().area_last_error().decode())
        return out, dict(zip(["primary", "secondary", "shadow_calls"], (int(c) for c in counters))), edge.astype(bool)

    def render_motion(self, cam, max_depth=5, smp=None, disp=None, sample_pass=0, light_seed=0, threads=0):
        """the included motion checker's own render (motion_render), for the no-cone identity"""
        d = np.zeros((self.n_roots, 3)) if disp is None else np.ascontiguousarray(disp, dtype=np.float64)
        out = np.zeros((cam.vsize, cam.hsize, 3), dtype=np.float64)
        counters = np.zeros(3, dtype=np.uint64)
        smp_p = C.byref(smp) if smp is not None else None
        if lib().motion_render(self._s, C.byref(cam), max_depth, light_seed, smp_p, sample_pass, d.ctypes.data, self.n_roots,
                               0, 0, cam.hsize, cam.vsize, threads, out.ctypes.data, counters.ctypes.data) != 0:
            raise RuntimeError("spot checker: " + lib().area_last_error().decode())
        return out, dict(zip(["primary", "secondary", "shadow_calls"], (int(c) for c in counters)))

    def close(self):
        if self._s:
            lib().area_scene_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def factor(c, cos_inner, cos_outer):
    return lib().spot_kat_factor(c, cos_inner, cos_outer)
