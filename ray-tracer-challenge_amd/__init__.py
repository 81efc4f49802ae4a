"""ray-tracer-challenge_amd — MI355X-native render path for SinclaM/ray-tracer-challenge.

Python is only the harness language here (tests, bench, multi-GPU driver): this
module is a ctypes binding of the two product libraries

  lib/librtc_hip.so   HIP kernels behind the C ABI of include/rtc.h
                      (replaces Camera.render, reference src/raytracer/camera.zig:80-125)
  lib/librtc_host.so  C++ host side: scene JSON / OBJ loaders, Camera/World/Canvas
                      mirror (reference src/parsing/*.zig, src/raytracer/canvas.zig)

There is no CPU implementation of the render path in this package: `GpuScene`
needs the HIP library and a GPU, and raises `RtcError` otherwise.  The package
directory name contains a hyphen, so import it with
`importlib.import_module("ray-tracer-challenge_amd")`.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (RTC_LIB_DIR: a diagnostic build of the three libraries somewhere else - tools/variants.py; the product is lib/)
LIB_DIR = os.environ.get("RTC_LIB_DIR", os.path.join(_HERE, "lib"))
REPO_ROOT = os.path.dirname(_HERE)
# Where HostScene.from_file looks for a scene given by name, and for the OBJ / PNG files a scene names.  The harness
# (tests, bench.py) uses the copies of the reference's scene and data files kept as fixtures under tests/golden/ (the
# reference tree does not exist on the GPU box); another host points these at its own directories.
SCENE_DIR = os.environ.get("RTC_SCENE_DIR", os.path.join(REPO_ROOT, "tests", "golden", "scenes"))
DATA_DIR = os.environ.get("RTC_DATA_DIR", os.path.join(REPO_ROOT, "tests", "golden", "data"))

RTC_CHILD_NODE_BIT = 0x80000000
RTC_MAT_STRIDE = 7
REFERENCE_DEPTH = 5  # camera.zig:118

_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)


class RtcError(RuntimeError):
    """An rtc_status != RTC_OK; `.name` is the Zig-style error name."""

    def __init__(self, name, message):
        super().__init__(message or name)
        self.name = name


class SceneDesc(C.Structure):
    """struct rtc_scene_desc (include/rtc.h)."""

    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_xforms", C.c_uint32), ("xf_inv", _dp), ("xf_inv_t", _dp),
        ("n_leaves", C.c_uint32), ("leaf_kind", _u8p), ("leaf_xform", _u32p), ("leaf_material", _u32p),
        ("leaf_shadow", _u8p), ("leaf_id", _u32p), ("leaf_geom", _u32p),
        ("n_cyls", C.c_uint32), ("cyl_min", _dp), ("cyl_max", _dp), ("cyl_closed", _u8p),
        ("n_tris", C.c_uint32), ("tri_p1", _dp), ("tri_e1", _dp), ("tri_e2", _dp),
        ("tri_n1", _dp), ("tri_n2", _dp), ("tri_n3", _dp),
        ("n_materials", C.c_uint32), ("mat_params", _dp), ("mat_pattern", _u32p),
        ("n_patterns", C.c_uint32), ("pat_kind", _u8p), ("pat_inv", _dp), ("pat_rgb", _dp),
        ("pat_a", _u32p), ("pat_b", _u32p),
        ("n_nodes", C.c_uint32), ("node_min", _dp), ("node_max", _dp), ("node_first", _u32p), ("node_count", _u32p),
        ("node_op", _u8p),
        ("n_children", C.c_uint32), ("children", _u32p),
        ("n_roots", C.c_uint32), ("roots", _u32p),
        ("n_lights", C.c_uint32), ("light_pos", _dp), ("light_rgb", _dp),
        ("n_texmaps", C.c_uint32), ("tex_mapping", _u8p), ("tex_uv", _u32p),
        ("n_uvs", C.c_uint32), ("uv_kind", _u8p), ("uv_size", _dp), ("uv_sub", _u32p), ("uv_image", _u32p),
        ("uv_interp", _u8p),
        ("n_images", C.c_uint32), ("img_width", _u32p), ("img_height", _u32p), ("img_offset", C.POINTER(C.c_uint64)),
        ("img_rgb", C.POINTER(C.c_float)),
    ]


class Camera(C.Structure):
    """struct rtc_camera (include/rtc.h)."""

    _fields_ = [("hsize", C.c_uint32), ("vsize", C.c_uint32),
                ("half_width", C.c_double), ("half_height", C.c_double), ("pixel_size", C.c_double),
                ("inv_view", C.c_double * 16)]


class Stats(C.Structure):
    """struct rtc_stats (include/rtc.h)."""

    _fields_ = [("primary", C.c_uint64), ("secondary", C.c_uint64), ("shadow_calls", C.c_uint64),
                ("shadow_traced", C.c_uint64), ("overflow", C.c_uint64)]


RTC_LIGHT_POINT = 0
RTC_LIGHT_AREA = 1
RTC_AREA_MAX_SAMPLES = 4096


class LightDesc(C.Structure):
    """struct rtc_light_desc (include/rtc.h): World.lights of both kinds, in order."""

    _fields_ = [("n_lights", C.c_uint32), ("kind", C.POINTER(C.c_uint8)), ("corner", C.POINTER(C.c_double)),
                ("uvec", C.POINTER(C.c_double)), ("vvec", C.POINTER(C.c_double)), ("usteps", C.POINTER(C.c_uint32)),
                ("vsteps", C.POINTER(C.c_uint32)), ("jitter", C.POINTER(C.c_uint8)), ("rgb", C.POINTER(C.c_double))]

    @classmethod
    def make(cls, lights):
        """From a list of dicts {"kind": "point", "position", "intensity"} / {"kind": "area", "corner", "uvec", "usteps",
        "vvec", "vsteps", "intensity", "jitter"}; the arrays are kept alive by the structure."""
        n = len(lights)
        arrays = {
            "kind": np.array([RTC_LIGHT_AREA if l["kind"] == "area" else RTC_LIGHT_POINT for l in lights], dtype=np.uint8),
            "corner": np.array([l["corner"] if l["kind"] == "area" else l["position"] for l in lights], dtype=np.float64).reshape(n, 3),
            "uvec": np.array([l.get("uvec", (0, 0, 0)) for l in lights], dtype=np.float64).reshape(n, 3),
            "vvec": np.array([l.get("vvec", (0, 0, 0)) for l in lights], dtype=np.float64).reshape(n, 3),
            "usteps": np.array([l.get("usteps", 1) for l in lights], dtype=np.uint32),
            "vsteps": np.array([l.get("vsteps", 1) for l in lights], dtype=np.uint32),
            "jitter": np.array([1 if l.get("jitter", False) else 0 for l in lights], dtype=np.uint8),
            "rgb": np.array([l["intensity"] for l in lights], dtype=np.float64).reshape(n, 3),
        }
        d = cls()
        d.n_lights = n
        for name, arr in arrays.items():
            arr = np.ascontiguousarray(arr)
            arrays[name] = arr
            setattr(d, name, arr.ctypes.data_as(dict(cls._fields_)[name]))
        d._arrays = arrays
        return d

    def to_list(self):
        """The table as the dicts make() takes."""
        out = []
        for i in range(self.n_lights):
            rgb = [self.rgb[3 * i + k] for k in range(3)]
            corner = [self.corner[3 * i + k] for k in range(3)]
            if self.kind[i] == RTC_LIGHT_AREA:
                out.append({"kind": "area", "corner": corner, "uvec": [self.uvec[3 * i + k] for k in range(3)],
                            "usteps": self.usteps[i], "vvec": [self.vvec[3 * i + k] for k in range(3)],
                            "vsteps": self.vsteps[i], "intensity": rgb, "jitter": bool(self.jitter[i])})
            else:
                out.append({"kind": "point", "position": corner, "intensity": rgb})
        return out


class Sampling(C.Structure):
    """struct rtc_sampling (include/rtc.h): camera samples per pixel - anti-aliasing and focal blur."""

    _fields_ = [("grid", C.c_uint32), ("jitter", C.c_uint32), ("aperture", C.c_double), ("focal_distance", C.c_double),
                ("seed", C.c_uint64)]

    def to_dict(self):
        return {"grid": self.grid, "jitter": bool(self.jitter), "aperture": self.aperture,
                "focal_distance": self.focal_distance, "seed": self.seed}


class Accum(C.Structure):
    """struct rtc_accum (include/rtc.h): one pass into running sums on the device (rtc_scene_accumulate_device); device
    pointers as integers, 0 for an optional output that is not wanted."""

    _fields_ = [("frame", C.c_void_p), ("n_pixels", C.c_size_t), ("passes", C.c_uint32), ("sum", C.c_void_p),
                ("sumsq", C.c_void_p), ("mean", C.c_void_p), ("rgba", C.c_void_p), ("noise", C.c_void_p)]


RTC_SAMPLING_INDEX_LIMIT = 1 << 24   # (pass + 1) * grid * grid may not exceed it (include/rtc.h)


class Adaptive(C.Structure):
    """struct rtc_adaptive (include/rtc.h): adaptive sampling's setting - tile_w x tile_h tiles take sample passes until
    min_passes, then until max_passes while their noise is above `threshold`."""

    _fields_ = [("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("min_passes", C.c_uint32), ("max_passes", C.c_uint32),
                ("threshold", C.c_double)]

    @classmethod
    def make(cls, threshold, max_passes, min_passes=4, tile=16):
        tw, th = (tile, tile) if isinstance(tile, int) else tile
        return cls(tw, th, min_passes, max_passes, threshold)

    def to_dict(self):
        return {"tile_w": self.tile_w, "tile_h": self.tile_h, "min_passes": self.min_passes, "max_passes": self.max_passes,
                "threshold": self.threshold}


class AdaptiveState(C.Structure):
    """struct rtc_adaptive_state (include/rtc.h): a run's device buffers as integers (0: an optional one not wanted), and
    `round`, a host field."""

    _fields_ = [("sum", C.c_void_p), ("sumsq", C.c_void_p), ("mean", C.c_void_p), ("rgba", C.c_void_p), ("tile_passes", C.c_void_p),
                ("tile_noise", C.c_void_p), ("active", C.c_void_p), ("n_active", C.c_void_p), ("max_noise", C.c_void_p),
                ("round", C.c_uint32)]


DENOISE_MAX_RADIUS = 10   # RTC_DENOISE_MAX_RADIUS
DENOISE_MAX_PATCH = 3     # RTC_DENOISE_MAX_PATCH
DENOISE_EPS = 1e-10       # RTC_DENOISE_EPS


class DenoiseSetting(C.Structure):
    """struct rtc_denoise_setting (include/rtc.h): the denoiser's search radius, patch radius, strength and the share of the
    variance it takes out of a distance.  make() fills the defaults the scene loader uses."""

    _fields_ = [("radius", C.c_uint32), ("patch", C.c_uint32), ("strength", C.c_double), ("cancel", C.c_double)]

    @classmethod
    def make(cls, radius=7, patch=2, strength=0.45, cancel=1.0):
        return cls(radius, patch, strength, cancel)

    def to_dict(self):
        return {"radius": self.radius, "patch": self.patch, "strength": self.strength, "cancel": self.cancel}


class Denoise(C.Structure):
    """struct rtc_denoise (include/rtc.h): one call of rtc_denoise_device; device pointers as integers, 0 for tile_passes
    (then `passes` holds for every pixel) or for rgba when it is not wanted."""

    _fields_ = [("mean", C.c_void_p), ("sumsq", C.c_void_p), ("hsize", C.c_uint32), ("vsize", C.c_uint32), ("passes", C.c_uint32),
                ("tile_passes", C.c_void_p), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("setting", DenoiseSetting),
                ("out", C.c_void_p), ("rgba", C.c_void_p)]


FILM_MAX_RADIUS = 32      # RTC_FILM_MAX_RADIUS
FILM_EPS = 1e-10          # RTC_FILM_EPS
FILM_CURVES = {"linear": 0, "reinhard": 1, "aces": 2, "hable": 3}     # RTC_FILM_CURVE_*
FILM_TRANSFERS = {"linear": 0, "srgb": 1, "gamma": 2}                 # RTC_FILM_TRANSFER_*


class FilmSetting(C.Structure):
    """struct rtc_film_setting (include/rtc.h): the film stage's exposure, bloom, tone curve and transfer function.  make()
    fills the defaults the scene loader uses; curve and transfer are numbers or the names of FILM_CURVES / FILM_TRANSFERS;
    bloom=True is the loader's "bloom": true."""

    _fields_ = [("exposure", C.c_double), ("auto_key", C.c_double), ("bloom_radius", C.c_uint32), ("bloom_sigma", C.c_double),
                ("bloom_threshold", C.c_double), ("bloom_intensity", C.c_double), ("curve", C.c_uint32), ("white", C.c_double),
                ("transfer", C.c_uint32), ("gamma", C.c_double)]

    @classmethod
    def make(cls, exposure=1.0, auto_key=0.0, bloom_radius=0, bloom_sigma=4.0, bloom_threshold=1.0, bloom_intensity=0.0, curve="aces",
             white=4.0, transfer="srgb", gamma=2.2, bloom=False):
        if bloom:
            bloom_radius, bloom_sigma, bloom_threshold, bloom_intensity = 12, 4.0, 1.0, 0.15
        return cls(exposure, auto_key, bloom_radius, bloom_sigma, bloom_threshold, bloom_intensity, FILM_CURVES.get(curve, curve), white,
                   FILM_TRANSFERS.get(transfer, transfer), gamma)

    def to_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class Film(C.Structure):
    """struct rtc_film (include/rtc.h): one call of rtc_film_device; device pointers as integers, 0 for scratch where
    film_scratch_bytes() is 0 and for rgba or scale_out when they are not wanted."""

    _fields_ = [("in_", C.c_void_p), ("hsize", C.c_uint32), ("vsize", C.c_uint32), ("setting", FilmSetting), ("scratch", C.c_void_p),
                ("out", C.c_void_p), ("rgba", C.c_void_p), ("scale_out", C.c_void_p)]


ROBUST_MAX_BUCKETS = 15   # RTC_ROBUST_MAX_BUCKETS


class RobustSetting(C.Structure):
    """struct rtc_robust_setting (include/rtc.h): robust accumulation's bucket count M (odd, 3 .. 15) and the gain on the
    Gini coefficient (0 keeps every bucket, a large gain is the plain median).  make() fills the defaults the scene loader
    uses."""

    _fields_ = [("buckets", C.c_uint32), ("gain", C.c_double)]

    @classmethod
    def make(cls, buckets=5, gain=1.0):
        return cls(buckets, gain)

    def to_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class Robust(C.Structure):
    """struct rtc_robust (include/rtc.h): one call of rtc_robust_device; device pointers as integers, 0 for sumsq_out,
    rejected_out or rgba when they are not wanted."""

    _fields_ = [("sums", C.c_void_p), ("n_pixels", C.c_size_t), ("passes", C.c_uint32), ("setting", RobustSetting),
                ("mean_out", C.c_void_p), ("sumsq_out", C.c_void_p), ("rejected_out", C.c_void_p), ("rgba", C.c_void_p)]


class Motion(C.Structure):
    """struct rtc_motion (include/rtc.h): a world-space displacement over the shutter per World.objects entry."""

    _fields_ = [("n_roots", C.c_uint32), ("displacement", C.POINTER(C.c_double))]


class Spot(C.Structure):
    """struct rtc_spot (include/rtc.h): a cone per World.lights entry (flag 0: the light as it is)."""

    _fields_ = [("n_lights", C.c_uint32), ("cone", C.POINTER(C.c_uint8)), ("axis", C.POINTER(C.c_double)),
                ("cos_inner", C.POINTER(C.c_double)), ("cos_outer", C.POINTER(C.c_double))]


def spot_struct(spots):
    """(Spot, the arrays it points into) of a dict of "cone", "axis", "cos_inner", "cos_outer" (GpuScene.set_spots); the
    arrays must outlive the struct's use."""
    cone = np.ascontiguousarray(spots["cone"], dtype=np.uint8)
    axis = np.ascontiguousarray(spots["axis"], dtype=np.float64)
    ci = np.ascontiguousarray(spots["cos_inner"], dtype=np.float64)
    co = np.ascontiguousarray(spots["cos_outer"], dtype=np.float64)
    n = cone.shape[0]
    if cone.ndim != 1 or axis.shape != (n, 3) or ci.shape != (n,) or co.shape != (n,):
        raise ValueError(f"spots: cone {cone.shape}, axis {axis.shape}, cos_inner {ci.shape}, cos_outer {co.shape}")
    sp = Spot(n, cone.ctypes.data_as(C.POINTER(C.c_uint8)), axis.ctypes.data_as(C.POINTER(C.c_double)),
              ci.ctypes.data_as(C.POINTER(C.c_double)), co.ctypes.data_as(C.POINTER(C.c_double)))
    return sp, (cone, axis, ci, co)


BUMP_NONE, BUMP_NOISE, BUMP_RIPPLES = 0, 1, 2  # RTC_BUMP_*
# leaf kinds (rtc.h); RTC_TORUS: a ring torus, its major and minor radius in cyl_min / cyl_max
RTC_SPHERE, RTC_PLANE, RTC_CUBE, RTC_CYLINDER, RTC_TRIANGLE, RTC_SMOOTH_TRIANGLE, RTC_CONE, RTC_TORUS = range(8)
# the options that select a kernel family on a handle that does not need it (set_option; tests and tools/time_scenes.py)
KERNEL_OPTIONS = ("sampling_kernels", "motion_kernels", "spot_kernels", "bump_kernels", "torus_kernels", "meshuv_kernels", "gloss_kernels",
                  "occlusion_kernels", "shadow_filter_kernels", "media_kernels", "environment_kernels", "sky_light_kernels",
                  "indirect_kernels", "emitter_kernels", "mis_kernels")
MAX_EMITTERS, EMITTER_MAX_SAMPLES, EMITTER_ROW = 4096, 16, 18  # RTC_MAX_EMITTERS, RTC_EMITTER_MAX_SAMPLES; rtc_diag_emitters' row
SKY_LIGHT_MAX_SAMPLES = 64  # RTC_SKY_LIGHT_MAX_SAMPLES
ENV_NO_PATTERN, ENV_SPHERE, ENV_CUBE, ENV_MAX_SUNS = 0xFFFFFFFF, 0, 1, 16  # RTC_ENV_*
NO_MEDIUM = 0xFFFFFFFF  # RTC_NO_MEDIUM: a ray in the atmosphere
# texture mappings (rtc.h); RTC_TEX_MESH: (u, v) from the hit triangle's texture row
RTC_TEX_SPHERICAL, RTC_TEX_PLANAR, RTC_TEX_CYLINDRICAL, RTC_TEX_CUBIC, RTC_TEX_MESH = range(5)
BUMP_MAX_OCTAVES = 16  # RTC_BUMP_MAX_OCTAVES


class MeshUvs(C.Structure):
    """struct rtc_mesh_uvs (include/rtc.h): a texture row (a1, b1, a2, b2, a3, b3) per triangle, in tri_* order."""
    _fields_ = [("n_tris", C.c_uint32), ("uv", C.POINTER(C.c_double))]


class Gloss(C.Structure):
    """struct rtc_gloss (include/rtc.h): a (reflection, transmission) roughness per material row, and the draws' seed."""

    _fields_ = [("n_materials", C.c_uint32), ("reflection", C.POINTER(C.c_double)), ("transmission", C.POINTER(C.c_double)),
                ("seed", C.c_uint64)]


def gloss_struct(gloss):
    """(Gloss, the arrays it points into) of a dict of "reflection" and "transmission" ((n,) each; one may be missing or None:
    all zeros) and an optional "seed" (GpuScene.set_gloss); the arrays must outlive the struct's use."""
    r, t = gloss.get("reflection"), gloss.get("transmission")
    r = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
    t = None if t is None else np.ascontiguousarray(t, dtype=np.float64)
    if r is None and t is None:
        raise ValueError("gloss: neither reflection nor transmission")
    n = (r if r is not None else t).shape[0]
    for a in (r, t):
        if a is not None and a.shape != (n,):
            raise ValueError(f"gloss: an array of shape {a.shape}, ({n},) expected")
    g = Gloss(n, r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None,
              t.ctypes.data_as(C.POINTER(C.c_double)) if t is not None else None, int(gloss.get("seed", 0)))
    return g, (r, t)


OCCLUSION_MAX_SAMPLES = 64  # RTC_OCCLUSION_MAX_SAMPLES


class Occlusion(C.Structure):
    """struct rtc_occlusion (include/rtc.h): an occlusion radius per material row, the rays per hit and the draws' seed."""

    _fields_ = [("n_materials", C.c_uint32), ("radius", C.POINTER(C.c_double)), ("samples", C.c_uint32), ("seed", C.c_uint64)]


def occlusion_struct(occlusion):
    """(Occlusion, the array it points into) of a dict of "radius" ((n,); None: all zeros, with "n_materials"), and optional
    "samples" (1) and "seed" (0) (GpuScene.set_occlusion); the array must outlive the struct's use."""
    r = occlusion.get("radius")
    if r is None:
        n = int(occlusion["n_materials"])
    else:
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.ndim != 1:
            raise ValueError(f"occlusion: a radius array of shape {r.shape}, (n,) expected")
        n = r.shape[0]
    o = Occlusion(n, r.ctypes.data_as(C.POINTER(C.c_double)) if r is not None else None, int(occlusion.get("samples", 1)),
                  int(occlusion.get("seed", 0)))
    return o, r


class ShadowFilters(C.Structure):
    """struct rtc_shadow_filters (include/rtc.h): three doubles per material row, the share of a light's red, green and blue
    that an entry of the material lets through."""

    _fields_ = [("n_materials", C.c_uint32), ("rgb", C.POINTER(C.c_double))]


def shadow_filters_struct(filters):
    """(ShadowFilters, the array it points into) of a dict of "rgb" ((n, 3); None: all zeros, with "n_materials")
    (GpuScene.set_shadow_filters); the array must outlive the struct's use."""
    rgb = filters.get("rgb")
    if rgb is None:
        n = int(filters["n_materials"])
    else:
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        if rgb.ndim != 2 or rgb.shape[1] != 3:
            raise ValueError(f"shadow filters: an rgb array of shape {rgb.shape}, (n, 3) expected")
        n = rgb.shape[0]
    f = ShadowFilters(n, rgb.ctypes.data_as(C.POINTER(C.c_double)) if rgb is not None else None)
    return f, rgb


class Media(C.Structure):
    """struct rtc_media (include/rtc.h): three doubles per material row, what a unit of world distance inside the material
    absorbs of red, green and blue, and the one atmosphere - a fog's density and colour."""

    _fields_ = [("n_materials", C.c_uint32), ("absorption", C.POINTER(C.c_double)), ("fog_density", C.c_double),
                ("fog_color", C.c_double * 3)]


def media_struct(media):
    """(Media, the array it points into) of a dict of "absorption" ((n, 3); None: all zeros, with "n_materials"),
    "fog_density" (0) and "fog_color" ((0, 0, 0)) (GpuScene.set_media); the array must outlive the struct's use."""
    a = media.get("absorption")
    if a is None:
        n = int(media["n_materials"])
    else:
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"media: an absorption array of shape {a.shape}, (n, 3) expected")
        n = a.shape[0]
    color = [float(x) for x in media.get("fog_color", (0.0, 0.0, 0.0))]
    if len(color) != 3:
        raise ValueError(f"media: a fog colour of {len(color)} values, 3 expected")
    m = Media(n, a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None, float(media.get("fog_density", 0.0)),
              (C.c_double * 3)(*color))
    return m, a


class Environment(C.Structure):
    """struct rtc_environment (include/rtc.h): the sky - a colour, with a pattern row the factor on that pattern's colour at a
    missed ray's direction - and the suns, directional lights: the way each one's light travels and its intensity."""

    _fields_ = [("rgb", C.c_double * 3), ("pattern", C.c_uint32), ("projection", C.c_uint32), ("n_suns", C.c_uint32),
                ("sun_direction", C.POINTER(C.c_double)), ("sun_rgb", C.POINTER(C.c_double))]


def environment_struct(env):
    """(Environment, the arrays it points into) of a dict of "rgb" ((0, 0, 0)), "pattern" (ENV_NO_PATTERN), "projection"
    (ENV_SPHERE), "sun_direction" and "sun_rgb" ((n, 3) each; none: no suns) (GpuScene.set_environment); the arrays must
    outlive the struct's use."""
    rgb = [float(x) for x in env.get("rgb", (0.0, 0.0, 0.0))]
    if len(rgb) != 3:
        raise ValueError(f"environment: a colour of {len(rgb)} values, 3 expected")
    d = np.ascontiguousarray(env.get("sun_direction", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
    c = np.ascontiguousarray(env.get("sun_rgb", np.zeros((0, 3))), dtype=np.float64).reshape(-1, 3)
    if d.shape != c.shape:
        raise ValueError(f"environment: {d.shape[0]} sun directions and {c.shape[0]} intensities")
    n = d.shape[0]
    e = Environment((C.c_double * 3)(*rgb), int(env.get("pattern", ENV_NO_PATTERN)), int(env.get("projection", ENV_SPHERE)), n,
                    d.ctypes.data_as(C.POINTER(C.c_double)) if n else None, c.ctypes.data_as(C.POINTER(C.c_double)) if n else None)
    return e, (d, c)


class SkyLight(C.Structure):
    """struct rtc_sky_light (include/rtc.h): the factor on the sky that `samples` hemisphere rays gather at every diffuse hit."""

    _fields_ = [("gain", C.c_double), ("samples", C.c_uint32), ("seed", C.c_uint64)]


def sky_light_struct(light):
    """SkyLight of a dict of "gain" (1.0), "samples" (1) and "seed" (0) (GpuScene.set_sky_light)"""
    return SkyLight(float(light.get("gain", 1.0)), int(light.get("samples", 1)), int(light.get("seed", 0)))


class Indirect(C.Structure):
    """struct rtc_indirect (include/rtc.h): the factor on a diffuse child's weight, the most diffuse bounces on one lineage,
    the draws' seed, and three doubles per material row that the material emits by itself (NULL: none)."""

    _fields_ = [("gain", C.c_double), ("bounces", C.c_uint32), ("seed", C.c_uint64), ("emission", C.POINTER(C.c_double)),
                ("n_materials", C.c_uint32)]


def indirect_struct(indirect):
    """(Indirect, the array it points into) of a dict of "gain" (1.0), "bounces" (1), "seed" (0) and "emission" ((n, 3);
    None: no rows) (GpuScene.set_indirect); the array must outlive the struct's use."""
    e = indirect.get("emission")
    n = 0
    if e is not None:
        e = np.ascontiguousarray(e, dtype=np.float64)
        if e.ndim != 2 or e.shape[1] != 3:
            raise ValueError(f"indirect: an emission array of shape {e.shape}, (n, 3) expected")
        n = e.shape[0]
    d = Indirect(float(indirect.get("gain", 1.0)), int(indirect.get("bounces", 1)), int(indirect.get("seed", 0)),
                 e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None, int(indirect.get("n_materials", n)))
    return d, e


class Emitters(C.Structure):
    """struct rtc_emitters (include/rtc.h): the samples per hit towards the handle's emissive surfaces and the draws' seed."""

    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint64)]


def emitters_struct(emitters):
    """Emitters of a dict of "samples" (1) and "seed" (0) (GpuScene.set_emitters)"""
    return Emitters(int(emitters.get("samples", 1)), int(emitters.get("seed", 0)))


def diag_emitters(desc, emission, filters=None):
    """rtc_diag_emitters: (rows (n, EMITTER_ROW), cdf (n,)) - the emitter list rtc_scene_set_emitters derives for a SceneDesc,
    an emission table (n_materials, 3) or None and a filter table (n_materials, 3) or None; no device is needed."""
    e = None if emission is None else np.ascontiguousarray(emission, dtype=np.float64)
    f = None if filters is None else np.ascontiguousarray(filters, dtype=np.float64)
    ep = e.ctypes.data_as(_dp) if e is not None else None
    fp = f.ctypes.data_as(_dp) if f is not None else None
    n = C.c_uint32()
    _check_hip(hip_lib().rtc_diag_emitters(C.byref(desc), ep, fp, 0, None, None, C.byref(n)))
    rows, cdf = np.zeros((n.value, EMITTER_ROW)), np.zeros(n.value)
    _check_hip(hip_lib().rtc_diag_emitters(C.byref(desc), ep, fp, n.value, rows.ctypes.data_as(_dp), cdf.ctypes.data_as(_dp), C.byref(n)))
    return rows, cdf


def diag_emitter_pick(cdf, u0):
    """rtc_diag_emitter_pick: the entry the kernels' binary search picks for the draw u0 from the CDF"""
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    k = C.c_uint32()
    lib = hip_lib()
    lib.rtc_diag_emitter_pick.argtypes = [_dp, C.c_uint32, C.c_double, C.POINTER(C.c_uint32)]
    _check_hip(lib.rtc_diag_emitter_pick(cdf.ctypes.data_as(_dp), len(cdf), float(u0), C.byref(k)))
    return int(k.value)


def diag_mis_weights(samples, q, cos_s, cos_e, r):
    """rtc_diag_mis_weights: (w_e, w_b), the balance heuristic's weights of rtc_scene_set_emitter_mis for one direction, by the
    kernels' own expression: `samples` emitter samples per hit, the entry's q, the cosine at the shaded point, the cosine at
    the emitter and the distance; (0, 1) where a skip rule of the sample step holds"""
    w_e, w_b = C.c_double(), C.c_double()
    lib = hip_lib()
    lib.rtc_diag_mis_weights.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, _dp, _dp]
    _check_hip(lib.rtc_diag_mis_weights(int(samples), float(q), float(cos_s), float(cos_e), float(r), C.byref(w_e), C.byref(w_b)))
    return float(w_e.value), float(w_b.value)


class Bump(C.Structure):
    """struct rtc_bump (include/rtc.h): a bump per material row (kind BUMP_NONE: the material as it is)."""

    _fields_ = [("n_materials", C.c_uint32), ("kind", C.POINTER(C.c_uint8)), ("amplitude", C.POINTER(C.c_double)),
                ("octaves", C.POINTER(C.c_uint32)), ("persistence", C.POINTER(C.c_double)), ("inverse", C.POINTER(C.c_double))]


def no_bumps(n_materials):
    """Every kind BUMP_NONE, with PerturbInfo's defaults and identity transforms: a dict as GpuScene.set_bumps takes."""
    inv = np.zeros((n_materials, 12))
    inv[:, [0, 5, 10]] = 1.0
    return {"kind": np.zeros(n_materials, dtype=np.uint8), "amplitude": np.zeros(n_materials),
            "octaves": np.full(n_materials, 3, dtype=np.uint32), "persistence": np.full(n_materials, 0.8), "inverse": inv}


def bump_struct(bumps):
    """(Bump, the arrays it points into) of a dict of "kind", "amplitude", "octaves", "persistence", "inverse"
    (GpuScene.set_bumps); the arrays must outlive the struct's use."""
    kind = np.ascontiguousarray(bumps["kind"], dtype=np.uint8)
    amp = np.ascontiguousarray(bumps["amplitude"], dtype=np.float64)
    octv = np.ascontiguousarray(bumps["octaves"], dtype=np.uint32)
    per = np.ascontiguousarray(bumps["persistence"], dtype=np.float64)
    inv = np.ascontiguousarray(bumps["inverse"], dtype=np.float64)
    n = kind.shape[0]
    if kind.ndim != 1 or amp.shape != (n,) or octv.shape != (n,) or per.shape != (n,) or inv.shape != (n, 12):
        raise ValueError(f"bumps: kind {kind.shape}, amplitude {amp.shape}, octaves {octv.shape}, persistence {per.shape}, inverse {inv.shape}")
    b = Bump(n, kind.ctypes.data_as(C.POINTER(C.c_uint8)), amp.ctypes.data_as(C.POINTER(C.c_double)),
             octv.ctypes.data_as(C.POINTER(C.c_uint32)), per.ctypes.data_as(C.POINTER(C.c_double)), inv.ctypes.data_as(C.POINTER(C.c_double)))
    return b, (kind, amp, octv, per, inv)


# (include/rtc.h: what a host binds ...)
RTC_SYMBOLS = ["rtc_scene_create", "rtc_scene_clone", "rtc_scene_destroy", "rtc_render", "rtc_render_rgba8", "rtc_render_device",
               "rtc_render_tiles_device", "rtc_assemble_tiles_device", "rtc_render_tile_list_device", "rtc_get_tile_costs",
               "rtc_assign_tiles", "rtc_assemble_tile_list_device", "rtc_assemble_tile_list_rgba8_device", "rtc_scatter_tile_list_device",
               "rtc_scatter_tile_list_rgba8_device", "rtc_scene_synchronize", "rtc_get_stats", "rtc_last_error", "rtc_status_name",
               "rtc_grow_csg_lists", "rtc_canvas_register", "rtc_canvas_unregister", "rtc_rgba8_device",
               "rtc_scene_create_with_lights", "rtc_scene_set_light_seed", "rtc_scene_set_sampling",
               "rtc_scene_set_sample_pass", "rtc_scene_accumulate_device", "rtc_scene_set_motion",
               "rtc_scene_adaptive_begin_device", "rtc_scene_adaptive_accumulate_device", "rtc_scene_adaptive_step", "rtc_render_adaptive",
               "rtc_scene_set_spots", "rtc_scene_set_bumps", "rtc_scene_set_mesh_uvs", "rtc_scene_set_gloss",
               "rtc_scene_set_occlusion", "rtc_scene_set_shadow_filters", "rtc_scene_set_media", "rtc_scene_set_environment",
               "rtc_scene_set_sky_light", "rtc_scene_set_indirect", "rtc_scene_set_emitters", "rtc_scene_set_emitter_mis", "rtc_denoise_device",
               "rtc_render_denoised", "rtc_film_scratch_bytes", "rtc_film_device", "rtc_render_filmed", "rtc_robust_device",
               "rtc_render_robust"]
# (... and include/rtc_diag.h: diagnostics and tuning, for the tests, bench.py and tools/)
RTC_DIAG_SYMBOLS = ["rtc_set_option", "rtc_last_kernel_name", "rtc_get_schedule", "rtc_get_chunk_times", "rtc_diag_build_tables", "rtc_diag_root_boxes", "rtc_diag_root_spheres", "rtc_diag_emitters", "rtc_diag_emitter_pick", "rtc_diag_mis_weights",
                    "rtc_diag_root_flags", "rtc_diag_denoise_tile", "rtc_diag_film_tile", "rtc_diag_robust_grid"]
HOST_SYMBOLS = ["rtch_last_error", "rtch_scene_load", "rtch_scene_free", "rtch_scene_desc", "rtch_scene_camera",
                "rtch_camera_rotate", "rtch_camera_move", "rtch_camera_make", "rtch_canvas_ppm", "rtch_canvas_rgba8", "rtch_scene_render", "rtch_set_loader_threads",
                "rtch_scene_lights", "rtch_scene_sampling", "rtch_scene_passes", "rtch_scene_motion", "rtch_scene_adaptive",
                "rtch_scene_spots", "rtch_scene_bumps", "rtch_scene_mesh_uvs", "rtch_scene_gloss", "rtch_scene_occlusion",
                "rtch_scene_shadow_filters", "rtch_scene_media", "rtch_scene_environment", "rtch_scene_sky_light",
                "rtch_scene_indirect", "rtch_scene_emitters", "rtch_scene_emitter_mis", "rtch_scene_denoise", "rtch_scene_film", "rtch_scene_robust"]

MULTI_SYMBOLS = ["rtc_multi_create", "rtc_multi_destroy", "rtc_multi_render", "rtc_multi_render_rgba8", "rtc_multi_render_device", "rtc_multi_render_rgba8_device",
                 "rtc_multi_synchronize", "rtc_multi_stream", "rtc_multi_get_stats", "rtc_multi_balance", "rtc_multi_last_error"]
RTC_MULTI_VIRTUAL = 1

_hip = None
_host = None
_multi = None


def _one_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64 (same SONAME as ROCm's, other file).
    A process that loads librtc_hip.so first (bound to /opt/rocm's copy) and torch later ends up with TWO
    HIP/HSA runtimes driving one GPU, and stream handles passed between them belong to the wrong one.  When
    torch is installed its copy is mapped first, so that the loader resolves our DT_NEEDED to it and one
    runtime serves both (what happens anyway when torch is imported before this package)."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for name in ("libamdhip64.so",):
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", name)
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def hip_lib():
    """librtc_hip.so; raises if the library has not been built (no fallback)."""
    global _hip
    if _hip is None:
        path = os.path.join(LIB_DIR, "librtc_hip.so")
        if not os.path.exists(path):
            raise RtcError("LibraryMissing", f"{path} not built: run `make` or __graft_entry__.build()")
        _one_hip_runtime()
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        lib.rtc_last_error.restype = C.c_char_p
        lib.rtc_status_name.restype = C.c_char_p
        lib.rtc_status_name.argtypes = [C.c_int]
        lib.rtc_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        lib.rtc_scene_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        lib.rtc_scene_create_with_lights.argtypes = [C.POINTER(SceneDesc), C.POINTER(LightDesc), C.POINTER(C.c_void_p)]
        lib.rtc_scene_set_light_seed.argtypes = [C.c_void_p, C.c_uint64]
        lib.rtc_scene_set_sampling.argtypes = [C.c_void_p, C.POINTER(Sampling)]
        lib.rtc_scene_set_sample_pass.argtypes = [C.c_void_p, C.c_uint32]
        lib.rtc_scene_accumulate_device.argtypes = [C.c_void_p, C.POINTER(Accum), C.c_void_p]
        lib.rtc_scene_set_motion.argtypes = [C.c_void_p, C.POINTER(Motion)]
        lib.rtc_scene_adaptive_begin_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Adaptive), C.POINTER(AdaptiveState),
                                                        C.c_void_p]
        lib.rtc_scene_adaptive_accumulate_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Adaptive),
                                                             C.POINTER(AdaptiveState), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        lib.rtc_scene_adaptive_step.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.POINTER(Adaptive), C.POINTER(AdaptiveState),
                                                C.POINTER(C.c_uint32), C.c_void_p]
        lib.rtc_scene_set_spots.argtypes = [C.c_void_p, C.POINTER(Spot)]
        lib.rtc_scene_set_bumps.argtypes = [C.c_void_p, C.POINTER(Bump)]
        lib.rtc_scene_set_mesh_uvs.argtypes = [C.c_void_p, C.POINTER(MeshUvs)]
        lib.rtc_scene_set_gloss.argtypes = [C.c_void_p, C.POINTER(Gloss)]
        lib.rtc_scene_set_occlusion.argtypes = [C.c_void_p, C.POINTER(Occlusion)]
        lib.rtc_scene_set_shadow_filters.argtypes = [C.c_void_p, C.POINTER(ShadowFilters)]
        lib.rtc_scene_set_media.argtypes = [C.c_void_p, C.POINTER(Media)]
        lib.rtc_scene_set_environment.argtypes = [C.c_void_p, C.POINTER(Environment)]
        lib.rtc_scene_set_sky_light.argtypes = [C.c_void_p, C.POINTER(SkyLight)]
        lib.rtc_scene_set_indirect.argtypes = [C.c_void_p, C.POINTER(Indirect)]
        lib.rtc_scene_set_emitters.argtypes = [C.c_void_p, C.POINTER(Emitters)]
        lib.rtc_scene_set_emitter_mis.argtypes = [C.c_void_p, C.c_uint32]
        lib.rtc_diag_emitters.argtypes = [C.POINTER(SceneDesc), _dp, _dp, C.c_uint32, _dp, _dp, C.POINTER(C.c_uint32)]
        lib.rtc_render_adaptive.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.POINTER(Adaptive), C.c_void_p, C.c_void_p]
        lib.rtc_denoise_device.argtypes = [C.POINTER(Denoise), C.c_void_p]
        lib.rtc_render_denoised.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.POINTER(Adaptive),
                                            C.POINTER(DenoiseSetting), C.c_void_p, C.c_void_p]
        lib.rtc_diag_denoise_tile.argtypes = [_u32p, _u32p]
        lib.rtc_film_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(FilmSetting)]
        lib.rtc_film_scratch_bytes.restype = C.c_size_t
        lib.rtc_film_device.argtypes = [C.POINTER(Film), C.c_void_p]
        lib.rtc_render_filmed.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.POINTER(Adaptive),
                                          C.POINTER(DenoiseSetting), C.POINTER(FilmSetting), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.rtc_diag_film_tile.argtypes = [_u32p, _u32p, _u32p]
        lib.rtc_robust_device.argtypes = [C.POINTER(Robust), C.c_void_p]
        lib.rtc_render_robust.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.POINTER(RobustSetting),
                                          C.POINTER(DenoiseSetting), C.POINTER(FilmSetting), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        lib.rtc_diag_robust_grid.argtypes = [_u32p, _u32p]
        lib.rtc_scene_destroy.argtypes = [C.c_void_p]
        lib.rtc_scene_destroy.restype = None
        lib.rtc_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32] + [C.c_uint32] * 4 + [C.c_void_p]
        lib.rtc_render_rgba8.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32] + [C.c_uint32] * 4 + [C.c_void_p]
        lib.rtc_render_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
        lib.rtc_render_tiles_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32] + [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p]
        lib.rtc_assemble_tiles_device.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p]
        lib.rtc_render_tile_list_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.c_uint32, _u32p, C.c_uint32,
                                                    C.c_void_p, C.c_void_p]
        lib.rtc_get_tile_costs.argtypes = [C.c_void_p, _dp, C.c_uint32]
        lib.rtc_assign_tiles.argtypes = [_dp, C.c_uint32, C.c_uint32, _u32p, _u32p]
        lib.rtc_assemble_tile_list_device.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
        lib.rtc_assemble_tile_list_rgba8_device.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
        lib.rtc_scene_synchronize.argtypes = [C.c_void_p]
        lib.rtc_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        lib.rtc_grow_csg_lists.argtypes = [C.c_void_p]
        lib.rtc_last_kernel_name.argtypes = [C.c_void_p]
        lib.rtc_last_kernel_name.restype = C.c_char_p
        lib.rtc_get_schedule.argtypes = [C.c_void_p, _u32p, C.c_size_t, _u32p]
        lib.rtc_get_chunk_times.argtypes = [C.c_void_p, C.POINTER(Camera), _u32p, _u32p, C.c_size_t, _u32p]
        lib.rtc_canvas_register.argtypes = [C.c_void_p, C.c_size_t]
        lib.rtc_canvas_unregister.argtypes = [C.c_void_p]
        lib.rtc_rgba8_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.rtc_set_option.argtypes = [C.c_char_p, C.c_double]
        lib.rtc_diag_build_tables.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        _hip = lib
    return _hip


def host_lib():
    """librtc_host.so (links librtc_hip.so)."""
    global _host
    if _host is None:
        hip_lib()
        path = os.path.join(LIB_DIR, "librtc_host.so")
        if not os.path.exists(path):
            raise RtcError("LibraryMissing", f"{path} not built: run `make` or __graft_entry__.build()")
        lib = C.CDLL(path)
        lib.rtch_last_error.restype = C.c_char_p
        lib.rtch_scene_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        lib.rtch_scene_free.argtypes = [C.c_void_p]
        lib.rtch_scene_free.restype = None
        lib.rtch_set_loader_threads.argtypes = [C.c_uint32]
        lib.rtch_set_loader_threads.restype = None
        lib.rtch_scene_desc.argtypes = [C.c_void_p]
        lib.rtch_scene_desc.restype = C.POINTER(SceneDesc)
        lib.rtch_scene_lights.argtypes = [C.c_void_p]
        lib.rtch_scene_lights.restype = C.POINTER(LightDesc)
        lib.rtch_scene_sampling.argtypes = [C.c_void_p, C.POINTER(Sampling)]
        lib.rtch_scene_passes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.rtch_scene_motion.argtypes = [C.c_void_p, _dp, C.c_uint32]
        lib.rtch_scene_spots.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), _dp, _dp, _dp, C.c_uint32]
        lib.rtch_scene_bumps.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), _dp, C.POINTER(C.c_uint32), _dp, _dp, C.c_uint32]
        lib.rtch_scene_mesh_uvs.argtypes = [C.c_void_p, _dp, C.c_uint32]
        lib.rtch_scene_gloss.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_uint32]
        lib.rtch_scene_occlusion.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_uint32]
        lib.rtch_scene_shadow_filters.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_int), C.c_uint32]
        lib.rtch_scene_media.argtypes = [C.c_void_p, _dp, _dp, C.POINTER(C.c_int), C.c_uint32]
        lib.rtch_scene_environment.argtypes = [C.c_void_p, C.POINTER(Environment), _dp, _dp, C.POINTER(C.c_int)]
        lib.rtch_scene_sky_light.argtypes = [C.c_void_p, C.POINTER(SkyLight), C.POINTER(C.c_int)]
        lib.rtch_scene_indirect.argtypes = [C.c_void_p, C.POINTER(Indirect), _dp, C.POINTER(C.c_int), C.c_uint32]
        lib.rtch_scene_emitters.argtypes = [C.c_void_p, C.POINTER(Emitters), C.POINTER(C.c_int)]
        lib.rtch_scene_emitter_mis.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.rtch_scene_adaptive.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(Adaptive)]
        lib.rtch_scene_denoise.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(DenoiseSetting)]
        lib.rtch_scene_film.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(FilmSetting)]
        lib.rtch_scene_robust.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(RobustSetting)]
        lib.rtch_scene_camera.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Camera)]
        lib.rtch_camera_rotate.argtypes = [C.c_void_p, C.c_double]
        lib.rtch_camera_move.argtypes = [C.c_void_p, C.c_double]
        lib.rtch_camera_make.argtypes = [C.c_uint32, C.c_uint32, C.c_double, _dp, _dp, _dp, C.POINTER(Camera)]
        lib.rtch_canvas_ppm.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
        lib.rtch_canvas_ppm.restype = C.c_size_t
        lib.rtch_canvas_rgba8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.rtch_canvas_rgba8.restype = None
        lib.rtch_scene_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _host = lib
    return _host


def multi_lib():
    """librtc_multi.so (links librtc_hip.so and RCCL): the single-process multi-GPU render of include/rtc_multi.h."""
    global _multi
    if _multi is None:
        hip_lib()
        path = os.path.join(LIB_DIR, "librtc_multi.so")
        if not os.path.exists(path):
            raise RtcError("LibraryMissing", f"{path} not built: run `make` or __graft_entry__.build()")
        lib = C.CDLL(path)
        lib.rtc_multi_last_error.restype = C.c_char_p
        lib.rtc_multi_create.argtypes = [C.POINTER(SceneDesc), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        lib.rtc_multi_destroy.argtypes = [C.c_void_p]
        lib.rtc_multi_destroy.restype = None
        lib.rtc_multi_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_void_p]
        lib.rtc_multi_render_rgba8.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.c_void_p]
        lib.rtc_multi_render_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.POINTER(C.c_void_p)]
        lib.rtc_multi_render_rgba8_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_uint32, C.POINTER(C.c_void_p)]
        lib.rtc_multi_synchronize.argtypes = [C.c_void_p]
        lib.rtc_multi_stream.argtypes = [C.c_void_p]
        lib.rtc_multi_stream.restype = C.c_void_p
        lib.rtc_multi_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        lib.rtc_multi_balance.argtypes = [C.c_void_p, _u32p, _dp]
        _multi = lib
    return _multi


class MultiGpu:
    """rtc_multi: one process, n GPUs, one gather per frame (include/rtc_multi.h)."""

    def __init__(self, desc, n_gpus, virtual=False, frames=1):
        """frames: frame slots (RTC_MULTI_FRAMES): render_device hands the frames to them in turn."""
        self.n = n_gpus
        self._m = C.c_void_p()
        flags = (RTC_MULTI_VIRTUAL if virtual else 0) | ((frames & 15) << 8)
        self._check(multi_lib().rtc_multi_create(C.byref(desc), n_gpus, flags, C.byref(self._m)))

    @staticmethod
    def _check(status):
        if status != 0:
            raise RtcError(hip_lib().rtc_status_name(status).decode(), multi_lib().rtc_multi_last_error().decode())

    def render(self, cam, max_depth=REFERENCE_DEPTH, out=None):
        if out is None:
            out = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        self._check(multi_lib().rtc_multi_render(self._m, C.byref(cam), max_depth, out.ctypes.data))
        return out

    def render_rgba8(self, cam, max_depth=REFERENCE_DEPTH, out=None):
        """The RGBA8 framebuffer of lib.zig:146-153, clamped on GPU 0; [vsize][hsize][4] u8 (host)."""
        if out is None:
            out = np.empty((cam.vsize, cam.hsize, 4), dtype=np.uint8)
        self._check(multi_lib().rtc_multi_render_rgba8(self._m, C.byref(cam), max_depth, out.ctypes.data))
        return out

    def render_device(self, cam, max_depth=REFERENCE_DEPTH):
        """Enqueues the frame and returns the device pointer (GPU 0) of its [vsize][hsize][3] f64 canvas; nothing is
        copied or waited for (synchronize(), or work enqueued on stream(), orders behind it)."""
        ptr = C.c_void_p()
        self._check(multi_lib().rtc_multi_render_device(self._m, C.byref(cam), max_depth, C.byref(ptr)))
        return ptr.value

    def render_rgba8_device(self, cam, max_depth=REFERENCE_DEPTH):
        """render_device for the RGBA8 framebuffer: the ranks clamp their tiles, 4 bytes per pixel are gathered."""
        ptr = C.c_void_p()
        self._check(multi_lib().rtc_multi_render_rgba8_device(self._m, C.byref(cam), max_depth, C.byref(ptr)))
        return ptr.value

    def synchronize(self):
        self._check(multi_lib().rtc_multi_synchronize(self._m))

    def stream(self):
        return multi_lib().rtc_multi_stream(self._m)

    def stats(self):
        st = Stats()
        self._check(multi_lib().rtc_multi_get_stats(self._m, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def balance(self):
        tiles = np.zeros(self.n, dtype=np.uint32)
        ratio = C.c_double()
        self._check(multi_lib().rtc_multi_balance(self._m, tiles.ctypes.data_as(_u32p), C.byref(ratio)))
        return tiles, ratio.value

    def close(self):
        if self._m:
            multi_lib().rtc_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_host(status):
    if status != 0:
        msg = host_lib().rtch_last_error().decode()
        raise RtcError(msg.split(":")[0], msg)


def _check_hip(status):
    if status != 0:
        lib = hip_lib()
        raise RtcError(lib.rtc_status_name(status).decode(), lib.rtc_last_error().decode())


class HostScene:
    """parseScene (reference src/parsing/scene.zig:612-661) + flattening, on the host."""

    def __init__(self, scene_json, data_dir=DATA_DIR):
        if isinstance(scene_json, str):
            scene_json = scene_json.encode()
        self._h = C.c_void_p()
        _check_host(host_lib().rtch_scene_load(scene_json, data_dir.encode(), C.byref(self._h)))
        self.desc = host_lib().rtch_scene_desc(self._h).contents
        self.desc._owner = self   # the tables behind `desc` are this object's: HostScene(...).desc alone must keep them alive
        self.lights = host_lib().rtch_scene_lights(self._h).contents  # World.lights of both kinds (rtc_light_desc)
        self.lights._owner = self

    @classmethod
    def from_file(cls, name, data_dir=DATA_DIR):
        path = name if os.path.exists(name) else os.path.join(SCENE_DIR, name)
        with open(path, "rb") as f:
            return cls(f.read(), data_dir)

    def camera(self, width=0, height=0):
        cam = Camera()
        _check_host(host_lib().rtch_scene_camera(self._h, width, height, C.byref(cam)))
        return cam

    def sampling(self):
        """The camera's "sampling" of the scene file (rtch_scene_sampling), or the defaults: a Sampling."""
        s = Sampling()
        _check_host(host_lib().rtch_scene_sampling(self._h, C.byref(s)))
        return s

    def passes(self):
        """The camera's "sampling": {"passes": n} of the scene file (rtch_scene_passes; 1 when absent)."""
        n = C.c_uint32()
        _check_host(host_lib().rtch_scene_passes(self._h, C.byref(n)))
        return n.value

    def motion(self):
        """The top-level objects' "motion" of the scene file (rtch_scene_motion): an (n_roots, 3) array, zero for a root
        without one."""
        n = self.desc.n_roots
        out = np.zeros((n, 3), dtype=np.float64)
        _check_host(host_lib().rtch_scene_motion(self._h, out.ctypes.data_as(_dp), n))
        return out

    def spots(self):
        """The scene file's "spot-light" entries (rtch_scene_spots), in World.lights order: a dict of "cone" (n,) uint8,
        "axis" (n, 3), "cos_inner" and "cos_outer" (n,) - what GpuScene.set_spots takes -, or None without a cone."""
        n = self.lights.n_lights
        out = {"cone": np.zeros(n, dtype=np.uint8), "axis": np.zeros((n, 3)), "cos_inner": np.zeros(n), "cos_outer": np.zeros(n)}
        _check_host(host_lib().rtch_scene_spots(self._h, out["cone"].ctypes.data_as(C.POINTER(C.c_uint8)), out["axis"].ctypes.data_as(_dp),
                                                out["cos_inner"].ctypes.data_as(_dp), out["cos_outer"].ctypes.data_as(_dp), n))
        return out if out["cone"].any() else None

    def bumps(self):
        """The materials' "normal-perturbation" entries (rtch_scene_bumps), in mat_* order: a dict of "kind" (n,) uint8,
        "amplitude" (n,), "octaves" (n,) uint32, "persistence" (n,) and "inverse" (n, 12) - what GpuScene.set_bumps takes -,
        or None when no material has one."""
        n = self.desc.n_materials
        out = no_bumps(n)
        _check_host(host_lib().rtch_scene_bumps(self._h, out["kind"].ctypes.data_as(C.POINTER(C.c_uint8)), out["amplitude"].ctypes.data_as(_dp),
                                                out["octaves"].ctypes.data_as(C.POINTER(C.c_uint32)), out["persistence"].ctypes.data_as(_dp),
                                                out["inverse"].ctypes.data_as(_dp), n))
        return out if out["kind"].any() else None

    def mesh_uvs(self):
        """The triangles' texture rows (rtch_scene_mesh_uvs), in tri_* order: an (n_tris, 6) array of (a1, b1, a2, b2, a3, b3)
        - what GpuScene.set_mesh_uvs takes -, or None when no triangle has texture coordinates."""
        n = self.desc.n_tris
        out = np.zeros((n, 6))
        _check_host(host_lib().rtch_scene_mesh_uvs(self._h, out.ctypes.data_as(_dp), n))
        return out if out.any() else None

    def gloss(self):
        """The materials' "roughness" entries (rtch_scene_gloss), in mat_* order, and the camera's "gloss-seed": a dict of
        "reflection" (n,), "transmission" (n,) and "seed" - what GpuScene.set_gloss takes -, or None when no material of the
        file has the key."""
        n = self.desc.n_materials
        out = {"reflection": np.zeros(n), "transmission": np.zeros(n)}
        seed, present = C.c_uint64(), C.c_int()
        _check_host(host_lib().rtch_scene_gloss(self._h, out["reflection"].ctypes.data_as(_dp), out["transmission"].ctypes.data_as(_dp),
                                                C.byref(seed), C.byref(present), n))
        out["seed"] = seed.value
        return out if present.value else None

    def occlusion(self):
        """The materials' "ambient-occlusion" radii (rtch_scene_occlusion), in mat_* order, and the camera's
        "occlusion-samples" and "occlusion-seed": a dict of "radius" (n,), "samples" and "seed" - what
        GpuScene.set_occlusion takes -, or None when no material of the file has the key."""
        n = self.desc.n_materials
        out = {"radius": np.zeros(n)}
        samples, seed, present = C.c_uint32(), C.c_uint64(), C.c_int()
        _check_host(host_lib().rtch_scene_occlusion(self._h, out["radius"].ctypes.data_as(_dp), C.byref(samples), C.byref(seed),
                                                    C.byref(present), n))
        out["samples"], out["seed"] = samples.value, seed.value
        return out if present.value else None

    def shadow_filters(self):
        """The materials' "shadow-filter" rows (rtch_scene_shadow_filters), in mat_* order: a dict of "rgb" (n, 3) - what
        GpuScene.set_shadow_filters takes -, or None when no material of the file has the key."""
        n = self.desc.n_materials
        out = {"rgb": np.zeros((n, 3))}
        present = C.c_int()
        _check_host(host_lib().rtch_scene_shadow_filters(self._h, out["rgb"].ctypes.data_as(_dp), C.byref(present), n))
        return out if present.value else None

    def media(self):
        """The materials' "absorption" rows, in mat_* order, and the scene's "atmosphere" (rtch_scene_media): a dict of
        "absorption" (n, 3), "fog_density" and "fog_color" - what GpuScene.set_media takes -, or None when no material of the
        file has the key and the file has no atmosphere."""
        n = self.desc.n_materials
        a, fog = np.zeros((n, 3)), np.zeros(4)
        present = C.c_int()
        _check_host(host_lib().rtch_scene_media(self._h, a.ctypes.data_as(_dp), fog.ctypes.data_as(_dp), C.byref(present), n))
        out = {"absorption": a, "fog_density": float(fog[0]), "fog_color": [float(x) for x in fog[1:]]}
        return out if present.value else None

    def environment(self):
        """The scene's "environment" (rtch_scene_environment): a dict of "rgb", "pattern" (a row of the description's pat_*
        tables, or ENV_NO_PATTERN), "projection", "sun_direction" and "sun_rgb" ((n, 3) each, as the file has them) - what
        GpuScene.set_environment takes -, or None when the file has no environment."""
        e = Environment()
        d, c = np.zeros((ENV_MAX_SUNS, 3)), np.zeros((ENV_MAX_SUNS, 3))
        present = C.c_int()
        _check_host(host_lib().rtch_scene_environment(self._h, C.byref(e), d.ctypes.data_as(_dp), c.ctypes.data_as(_dp), C.byref(present)))
        if not present.value:
            return None
        n = int(e.n_suns)
        return {"rgb": [float(x) for x in e.rgb], "pattern": int(e.pattern), "projection": int(e.projection),
                "sun_direction": d[:n].copy(), "sun_rgb": c[:n].copy()}

    def sky_light(self):
        """The environment's "light" (rtch_scene_sky_light): a dict of "gain", "samples" and "seed" - what
        GpuScene.set_sky_light takes -, or None when the file has none."""
        y = SkyLight()
        present = C.c_int()
        _check_host(host_lib().rtch_scene_sky_light(self._h, C.byref(y), C.byref(present)))
        if not present.value:
            return None
        return {"gain": float(y.gain), "samples": int(y.samples), "seed": int(y.seed)}

    def indirect(self):
        """The scene's "indirect" and the materials' "emission" rows, in mat_* order (rtch_scene_indirect): a dict of "gain",
        "bounces", "seed" and "emission" (n, 3) - what GpuScene.set_indirect takes -, or None when the file has neither key."""
        n = self.desc.n_materials
        d, e = Indirect(), np.zeros((n, 3))
        present = C.c_int()
        _check_host(host_lib().rtch_scene_indirect(self._h, C.byref(d), e.ctypes.data_as(_dp), C.byref(present), n))
        if not present.value:
            return None
        return {"gain": float(d.gain), "bounces": int(d.bounces), "seed": int(d.seed), "emission": e}

    def emitters(self):
        """The "emitters" key of the scene's "indirect" (rtch_scene_emitters): a dict of "samples" and "seed" - what
        GpuScene.set_emitters takes -, or None when the file has no such key."""
        e = Emitters()
        present = C.c_int()
        _check_host(host_lib().rtch_scene_emitters(self._h, C.byref(e), C.byref(present)))
        if not present.value:
            return None
        return {"samples": int(e.samples), "seed": int(e.seed)}

    def emitter_mis(self):
        """The "mis" key inside the scene's "emitters" (rtch_scene_emitter_mis): 1 where the file has it and it is true, else 0 -
        what GpuScene.set_emitter_mis takes."""
        mode = C.c_uint32()
        _check_host(host_lib().rtch_scene_emitter_mis(self._h, C.byref(mode)))
        return int(mode.value)

    def adaptive(self):
        """The camera's "sampling": {"adaptive": ...} of the scene file (rtch_scene_adaptive): an Adaptive whose max_passes
        is "passes", or None when the file has none."""
        on, a = C.c_int(), Adaptive()
        _check_host(host_lib().rtch_scene_adaptive(self._h, C.byref(on), C.byref(a)))
        return a if on.value else None

    def denoise(self):
        """The camera's "sampling": {"denoise": ...} of the scene file (rtch_scene_denoise): a DenoiseSetting, or None when
        the file has no such key (or has it false)."""
        on, d = C.c_int(), DenoiseSetting()
        _check_host(host_lib().rtch_scene_denoise(self._h, C.byref(on), C.byref(d)))
        return d if on.value else None

    def film(self):
        """The camera's "film" of the scene file (rtch_scene_film): a FilmSetting, or None when the file has no such key (or
        has it false)."""
        on, f = C.c_int(), FilmSetting()
        _check_host(host_lib().rtch_scene_film(self._h, C.byref(on), C.byref(f)))
        return f if on.value else None

    def robust(self):
        """The camera sampling's "robust" of the scene file (rtch_scene_robust): a RobustSetting, or None when the file has
        no such key (or has it false)."""
        on, r = C.c_int(), RobustSetting()
        _check_host(host_lib().rtch_scene_robust(self._h, C.byref(on), C.byref(r)))
        return r if on.value else None

    def rotate_camera(self, angle):
        """Renderer.rotateCamera (lib.zig:166-178): orbit the camera around its target, about `up`."""
        _check_host(host_lib().rtch_camera_rotate(self._h, C.c_double(angle)))

    def move_camera(self, distance):
        """Renderer.moveCamera (lib.zig:180-190): move the camera along its line of sight by distance * |to - from|."""
        _check_host(host_lib().rtch_camera_move(self._h, C.c_double(distance)))

    def array(self, field, count, width=1, dtype=None):
        """numpy view of one table of the flat description (writable: tests patch tables)."""
        ptr = getattr(self.desc, field)
        n = count * width
        if n == 0:
            return np.zeros((0,), dtype=dtype)
        arr = np.ctypeslib.as_array(ptr, shape=(n,))
        return arr.reshape(count, width) if width > 1 else arr

    def close(self):
        if self._h:
            host_lib().rtch_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_camera(hsize, vsize, fov, frm, to, up):
    """Camera.new + setTransform(viewTransform(from,to,up)) (camera.zig:33-61, matrix.zig:54-67)."""
    cam = Camera()
    arr = lambda v: (C.c_double * 3)(*v)
    _check_host(host_lib().rtch_camera_make(hsize, vsize, fov, arr(frm), arr(to), arr(up), C.byref(cam)))
    return cam


class GpuScene:
    """rtc_scene: the flat scene resident in HBM; many renders per upload."""

    def __init__(self, desc, lights=None, _clone_of=None):
        """lights: a LightDesc (HostScene.lights, LightDesc.make) that replaces desc's point lights
        (rtc_scene_create_with_lights); None: rtc_scene_create."""
        self._s = C.c_void_p()
        if _clone_of is not None:
            _check_hip(hip_lib().rtc_scene_clone(_clone_of._s, C.byref(self._s)))
        elif lights is not None:
            _check_hip(hip_lib().rtc_scene_create_with_lights(C.byref(desc), C.byref(lights), C.byref(self._s)))
        else:
            _check_hip(hip_lib().rtc_scene_create(C.byref(desc), C.byref(self._s)))

    def set_light_seed(self, seed):
        """rtc_scene_set_light_seed: the seed of the area lights' jitter on this handle."""
        _check_hip(hip_lib().rtc_scene_set_light_seed(self._s, seed))

    def set_sampling(self, grid=1, jitter=False, aperture=0.0, focal_distance=1.0, seed=0):
        """rtc_scene_set_sampling: grid x grid camera samples per pixel, optionally jittered, through a lens of radius
        `aperture` focused at `focal_distance` (0: a pinhole).  A Sampling as `grid` is passed as it is; None: the default."""
        if grid is None:
            _check_hip(hip_lib().rtc_scene_set_sampling(self._s, None))
            return
        s = grid if isinstance(grid, Sampling) else Sampling(grid, 1 if jitter else 0, aperture, focal_distance, seed)
        _check_hip(hip_lib().rtc_scene_set_sampling(self._s, C.byref(s)))

    def set_sample_pass(self, p):
        """rtc_scene_set_sample_pass: the sample pass every later render of this handle draws (0: the default)."""
        _check_hip(hip_lib().rtc_scene_set_sample_pass(self._s, p))

    def set_motion(self, displacements):
        """rtc_scene_set_motion: an (n_roots, 3) array of world-space displacements over the shutter, one per World.objects
        entry (HostScene.motion()); None: static."""
        if displacements is None:
            _check_hip(hip_lib().rtc_scene_set_motion(self._s, None))
            return
        d = np.ascontiguousarray(displacements, dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 3:
            raise ValueError(f"set_motion: displacements of shape {d.shape}, (n_roots, 3) expected")
        m = Motion(d.shape[0], d.ctypes.data_as(_dp))
        _check_hip(hip_lib().rtc_scene_set_motion(self._s, C.byref(m)))

    def set_spots(self, spots):
        """rtc_scene_set_spots: a dict of "cone" (n_lights,) 0 / 1, "axis" (n_lights, 3), "cos_inner" and "cos_outer"
        (n_lights,), one entry per World.lights entry (HostScene.spots()); None: no cones."""
        if spots is None:
            _check_hip(hip_lib().rtc_scene_set_spots(self._s, None))
            return
        sp, _keep = spot_struct(spots)
        _check_hip(hip_lib().rtc_scene_set_spots(self._s, C.byref(sp)))

    def set_bumps(self, bumps):
        """rtc_scene_set_bumps: a dict of "kind" (n_materials,) BUMP_*, "amplitude", "octaves", "persistence" (n_materials,)
        and "inverse" (n_materials, 12), one entry per material row (HostScene.bumps(), no_bumps()); None: no bumps."""
        if bumps is None:
            _check_hip(hip_lib().rtc_scene_set_bumps(self._s, None))
            return
        b, _keep = bump_struct(bumps)
        _check_hip(hip_lib().rtc_scene_set_bumps(self._s, C.byref(b)))

    def set_mesh_uvs(self, uvs):
        """rtc_scene_set_mesh_uvs: an (n_tris, 6) array of texture rows (a1, b1, a2, b2, a3, b3), one per triangle in tri_*
        order (HostScene.mesh_uvs()); None: the all-zero rows."""
        if uvs is None:
            _check_hip(hip_lib().rtc_scene_set_mesh_uvs(self._s, None))
            return
        u = np.ascontiguousarray(uvs, dtype=np.float64)
        if u.ndim != 2 or u.shape[1] != 6:
            raise ValueError(f"set_mesh_uvs: rows of shape {u.shape}, (n_tris, 6) expected")
        m = MeshUvs(u.shape[0], u.ctypes.data_as(_dp))
        _check_hip(hip_lib().rtc_scene_set_mesh_uvs(self._s, C.byref(m)))

    def set_gloss(self, gloss):
        """rtc_scene_set_gloss: a dict of "reflection" and "transmission" ((n_materials,) each; one may be missing: all zeros)
        and an optional "seed" (HostScene.gloss()); None: no gloss - as every row zero, the handle's previous kernels."""
        if gloss is None:
            _check_hip(hip_lib().rtc_scene_set_gloss(self._s, None))
            return
        g, _keep = gloss_struct(gloss)
        _check_hip(hip_lib().rtc_scene_set_gloss(self._s, C.byref(g)))

    def set_occlusion(self, occlusion):
        """rtc_scene_set_occlusion: a dict of "radius" ((n_materials,)) and optional "samples" (1) and "seed" (0)
        (HostScene.occlusion()); None: no occlusion - as every row zero, the handle's previous kernels."""
        if occlusion is None:
            _check_hip(hip_lib().rtc_scene_set_occlusion(self._s, None))
            return
        o, _keep = occlusion_struct(occlusion)
        _check_hip(hip_lib().rtc_scene_set_occlusion(self._s, C.byref(o)))

    def set_shadow_filters(self, filters):
        """rtc_scene_set_shadow_filters: a dict of "rgb" ((n_materials, 3)) (HostScene.shadow_filters()); None: no filter -
        as every row zero, the handle's previous kernels."""
        if filters is None:
            _check_hip(hip_lib().rtc_scene_set_shadow_filters(self._s, None))
            return
        f, _keep = shadow_filters_struct(filters)
        _check_hip(hip_lib().rtc_scene_set_shadow_filters(self._s, C.byref(f)))

    def set_media(self, media):
        """rtc_scene_set_media: a dict of "absorption" ((n_materials, 3)), "fog_density" and "fog_color" (HostScene.media());
        None: no media - as every row and the density zero, the handle's previous kernels."""
        if media is None:
            _check_hip(hip_lib().rtc_scene_set_media(self._s, None))
            return
        m, _keep = media_struct(media)
        _check_hip(hip_lib().rtc_scene_set_media(self._s, C.byref(m)))

    def set_environment(self, env):
        """rtc_scene_set_environment: a dict of "rgb", "pattern", "projection", "sun_direction" and "sun_rgb"
        (HostScene.environment()); None: no environment - as a sky of zero with no pattern and no suns, the handle's previous
        kernels."""
        if env is None:
            _check_hip(hip_lib().rtc_scene_set_environment(self._s, None))
            return
        e, _keep = environment_struct(env)
        _check_hip(hip_lib().rtc_scene_set_environment(self._s, C.byref(e)))

    def set_sky_light(self, light):
        """rtc_scene_set_sky_light: a dict of "gain", "samples" and "seed" (HostScene.sky_light()); None: no sky light - as a
        gain of zero, the handle's previous kernels."""
        if light is None:
            _check_hip(hip_lib().rtc_scene_set_sky_light(self._s, None))
            return
        y = sky_light_struct(light)
        _check_hip(hip_lib().rtc_scene_set_sky_light(self._s, C.byref(y)))

    def set_indirect(self, indirect):
        """rtc_scene_set_indirect: a dict of "gain", "bounces", "seed" and "emission" ((n_materials, 3) or None)
        (HostScene.indirect()); None: no table - as a table that forms no child and emits nothing, the handle's previous
        kernels."""
        if indirect is None:
            _check_hip(hip_lib().rtc_scene_set_indirect(self._s, None))
            return
        d, _keep = indirect_struct(indirect)
        _check_hip(hip_lib().rtc_scene_set_indirect(self._s, C.byref(d)))

    def set_emitters(self, emitters):
        """rtc_scene_set_emitters: a dict of "samples" and "seed" (HostScene.emitters()); None: no table - the handle's previous
        kernels.  The list of emitters is derived from the handle's indirect and shadow-filter tables, whenever either is set."""
        if emitters is None:
            _check_hip(hip_lib().rtc_scene_set_emitters(self._s, None))
            return
        e = emitters_struct(emitters)
        _check_hip(hip_lib().rtc_scene_set_emitters(self._s, C.byref(e)))

    def set_emitter_mis(self, mode):
        """rtc_scene_set_emitter_mis: False / 0 - emitter samples and diffuse children combined by a switch, the default -,
        True / 1 - weighted by the balance heuristic (HostScene.emitter_mis()).  It has an effect while the handle's derived
        emitter list is not empty, whatever the order of the setters."""
        _check_hip(hip_lib().rtc_scene_set_emitter_mis(self._s, int(mode)))

    def accumulate_device(self, accum, stream=None):
        """rtc_scene_accumulate_device: an Accum, enqueued on `stream` (None: the handle's own) after this handle's renders."""
        _check_hip(hip_lib().rtc_scene_accumulate_device(self._s, C.byref(accum), stream))

    def adaptive_begin(self, hsize, vsize, adaptive, state, stream=None):
        """rtc_scene_adaptive_begin_device: every tile active at 0 passes (state.round = 0)."""
        _check_hip(hip_lib().rtc_scene_adaptive_begin_device(self._s, hsize, vsize, C.byref(adaptive), C.byref(state), stream))

    def adaptive_accumulate_device(self, hsize, vsize, adaptive, state, d_frame_ptr, d_tiles_ptr, n_tiles, stream=None):
        """rtc_scene_adaptive_accumulate_device: a compact tile frame (region k: tile d_tiles[k]) into the run's sums, then
        the stopping rule over every tile."""
        _check_hip(hip_lib().rtc_scene_adaptive_accumulate_device(self._s, hsize, vsize, C.byref(adaptive), C.byref(state), d_frame_ptr,
                                                                  d_tiles_ptr, n_tiles, stream))

    def adaptive_step(self, cam, adaptive, state, max_depth=REFERENCE_DEPTH, stream=None):
        """rtc_scene_adaptive_step: one round; returns the tiles still active after it."""
        n = C.c_uint32()
        _check_hip(hip_lib().rtc_scene_adaptive_step(self._s, C.byref(cam), max_depth, C.byref(adaptive), C.byref(state), C.byref(n),
                                                     stream))
        return n.value

    def render_adaptive(self, cam, adaptive, max_depth=REFERENCE_DEPTH):
        """rtc_render_adaptive: a whole run; returns ([h][w][3] f64 mean, [T] u32 passes per tile), host arrays."""
        rgb = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        tx, ty = -(-cam.hsize // adaptive.tile_w), -(-cam.vsize // adaptive.tile_h)
        passes = np.empty(tx * ty, dtype=np.uint32)
        _check_hip(hip_lib().rtc_render_adaptive(self._s, C.byref(cam), max_depth, C.byref(adaptive), rgb.ctypes.data,
                                                 passes.ctypes.data))
        return rgb, passes

    def render_denoised(self, cam, passes, adaptive=None, setting=None, max_depth=REFERENCE_DEPTH):
        """rtc_render_denoised: `passes` sample passes (or, with an Adaptive, a whole adaptive run) accumulated on the device
        and filtered by the denoiser (setting: a DenoiseSetting; None: the defaults); returns (denoised, mean), both
        [h][w][3] f64 host arrays.  The handle's own sample pass is left as it was."""
        rgb = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        noisy = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        _check_hip(hip_lib().rtc_render_denoised(self._s, C.byref(cam), max_depth, passes, C.byref(adaptive) if adaptive is not None else None,
                                                 C.byref(setting) if setting is not None else None, rgb.ctypes.data, noisy.ctypes.data))
        return rgb, noisy

    def render_filmed(self, cam, passes, adaptive=None, denoise=None, film=None, max_depth=REFERENCE_DEPTH):
        """rtc_render_filmed: `passes` sample passes (or, with an Adaptive, a whole adaptive run) accumulated on the device,
        filtered by the denoiser where `denoise` is a DenoiseSetting, and taken to display values by the film stage (film: a
        FilmSetting; None: the defaults); returns (rgb [h][w][3] f64, rgba [h][w][4] u8, linear [h][w][3] f64: the image the
        film read), host arrays.  The handle's own sample pass is left as it was."""
        rgb = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        rgba = np.empty((cam.vsize, cam.hsize, 4), dtype=np.uint8)
        linear = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        _check_hip(hip_lib().rtc_render_filmed(self._s, C.byref(cam), max_depth, passes, C.byref(adaptive) if adaptive is not None else None,
                                               C.byref(denoise) if denoise is not None else None, C.byref(film) if film is not None else None,
                                               rgb.ctypes.data, rgba.ctypes.data, linear.ctypes.data))
        return rgb, rgba, linear

    def render_robust(self, cam, passes, robust=None, denoise=None, film=None, max_depth=REFERENCE_DEPTH):
        """rtc_render_robust: `passes` sample passes accumulated on the device, into the ordinary sums and round-robin into
        bucket sums; the Gini-weighted median of means of the buckets (robust: a RobustSetting; None: the defaults), filtered
        by the denoiser where `denoise` is a DenoiseSetting and taken to display values where `film` is a FilmSetting (None:
        no film stage); returns (rgb [h][w][3] f64: the last stage's image, rgba [h][w][4] u8: its clamp, robust [h][w][3]
        f64: the robust mean, plain [h][w][3] f64: the ordinary mean, rejected [h][w] u32: the buckets left out), host
        arrays.  The handle's own sample pass is left as it was."""
        shape = (cam.vsize, cam.hsize)
        rgb, robust_mean, plain = (np.empty(shape + (3,), dtype=np.float64) for _ in range(3))
        rgba = np.empty(shape + (4,), dtype=np.uint8)
        rejected = np.empty(shape, dtype=np.uint32)
        _check_hip(hip_lib().rtc_render_robust(self._s, C.byref(cam), max_depth, passes, C.byref(robust) if robust is not None else None,
                                               C.byref(denoise) if denoise is not None else None, C.byref(film) if film is not None else None,
                                               rgb.ctypes.data, rgba.ctypes.data, robust_mean.ctypes.data, plain.ctypes.data,
                                               rejected.ctypes.data))
        return rgb, rgba, robust_mean, plain, rejected

    def clone(self):
        """rtc_scene_clone: a handle of its own (stream, schedule, counters) on the same device copy of the scene - one
        per frame in flight."""
        return GpuScene(None, _clone_of=self)

    def render(self, cam, max_depth=REFERENCE_DEPTH, tile=None):
        """Camera.render for the whole image or tile=(x0,y0,w,h); returns [h][w][3] f64 (host)."""
        x0, y0, w, h = tile if tile else (0, 0, cam.hsize, cam.vsize)
        out = np.empty((h, w, 3), dtype=np.float64)
        _check_hip(hip_lib().rtc_render(self._s, C.byref(cam), max_depth, x0, y0, w, h, out.ctypes.data))
        return out

    def render_into(self, cam, out, max_depth=REFERENCE_DEPTH):
        """Camera.render into a caller-owned [h][w][3] f64 array (an interactive host reuses its canvas, and pins it
        once with canvas_register so that the copy runs at link speed)."""
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and out.shape == (cam.vsize, cam.hsize, 3)
        _check_hip(hip_lib().rtc_render(self._s, C.byref(cam), max_depth, 0, 0, cam.hsize, cam.vsize, out.ctypes.data))
        return out

    def render_rgba8(self, cam, max_depth=REFERENCE_DEPTH, tile=None, out=None):
        """The RGBA8 framebuffer of lib.zig:146-153, clamped on the device; returns [h][w][4] u8 (host)."""
        x0, y0, w, h = tile if tile else (0, 0, cam.hsize, cam.vsize)
        if out is None:
            out = np.empty((h, w, 4), dtype=np.uint8)
        _check_hip(hip_lib().rtc_render_rgba8(self._s, C.byref(cam), max_depth, x0, y0, w, h, out.ctypes.data))
        return out

    def render_device(self, cam, d_out_ptr, max_depth=REFERENCE_DEPTH, tile=None, stream=None):
        x0, y0, w, h = tile if tile else (0, 0, cam.hsize, cam.vsize)
        _check_hip(hip_lib().rtc_render_device(self._s, C.byref(cam), max_depth, x0, y0, w, h, d_out_ptr, stream))

    def render_tiles_device(self, cam, d_out_ptr, tile_w, tile_h, first_tile, tile_stride, n_my_tiles,
                            max_depth=REFERENCE_DEPTH, stream=None):
        _check_hip(hip_lib().rtc_render_tiles_device(self._s, C.byref(cam), max_depth, tile_w, tile_h, first_tile,
                                                     tile_stride, n_my_tiles, d_out_ptr, stream))

    def render_tile_list_device(self, cam, d_out_ptr, tile_w, tile_h, tiles, max_depth=REFERENCE_DEPTH, stream=None):
        """A rank's share of a cost-balanced split: region k of the buffer is tile tiles[k]."""
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
        _check_hip(hip_lib().rtc_render_tile_list_device(self._s, C.byref(cam), max_depth, tile_w, tile_h,
                                                         tiles.ctypes.data_as(_u32p), len(tiles), d_out_ptr, stream))

    def tile_costs(self, n_regions):
        """Measured cost of every region (tile) of the last measuring tile-mode render on this handle."""
        out = np.empty(n_regions, dtype=np.float64)
        _check_hip(hip_lib().rtc_get_tile_costs(self._s, out.ctypes.data_as(_dp), n_regions))
        return out

    def synchronize(self):
        _check_hip(hip_lib().rtc_scene_synchronize(self._s))

    def stats(self):
        st = Stats()
        _check_hip(hip_lib().rtc_get_stats(self._s, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def last_kernel_name(self):
        """The render kernel the last launch on this handle ran (the name rocprofv3 shows)."""
        return hip_lib().rtc_last_kernel_name(self._s).decode()

    def schedule(self):
        """Diagnostic: the packets the next launch of the current pixel map would run, [n][16] u32 (rtc_get_schedule)."""
        n = C.c_uint32()
        st = hip_lib().rtc_get_schedule(self._s, None, 0, C.byref(n))
        if n.value == 0:
            _check_hip(st)
            return np.zeros((0, 16), dtype=np.uint32)
        out = np.empty((n.value, 16), dtype=np.uint32)
        _check_hip(hip_lib().rtc_get_schedule(self._s, out.ctypes.data_as(_u32p), out.size, C.byref(n)))
        return out[:n.value]

    def chunk_times(self, cam):
        """Diagnostic: (estimated, measured) ticks per 8x8 chunk of the last scheduled launch's pixel map (rtc_get_chunk_times)."""
        n = C.c_uint32()
        _check_hip(hip_lib().rtc_get_chunk_times(self._s, C.byref(cam), None, None, 0, C.byref(n)))
        est, got = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _check_hip(hip_lib().rtc_get_chunk_times(self._s, C.byref(cam), est.ctypes.data_as(_u32p), got.ctypes.data_as(_u32p), n.value, C.byref(n)))
        return est, got

    def close(self):
        if self._s:
            hip_lib().rtc_scene_destroy(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Progressive:
    """Progressive rendering on the device: each step() renders the next sample pass of `gpu_scene` (rtc_scene_set_sample_pass)
    into a frame buffer and accumulates it (rtc_scene_accumulate_device) into running sums, the mean and its RGBA8 clamp,
    all torch tensors on the scene's device, on a torch stream of its own (`stream`).  The host decides when to stop, from
    what step() returns; mean() and rgba8() order the caller's current stream after the last step.  With robust=M (odd,
    3 .. 15) every step() also adds its pass to bucket `passes % M` of `buckets` ([M][h][w][3], a second
    rtc_scene_accumulate_device), and robust(), denoised(robust=...) and filmed(robust=...) resolve them (rtc_robust_device)."""

    def __init__(self, gpu_scene, cam, max_depth=REFERENCE_DEPTH, noise=True, robust=None):
        import torch
        self.gpu, self.cam, self.max_depth, self.noise_on = gpu_scene, cam, max_depth, noise
        if robust is not None and (robust % 2 == 0 or not 3 <= robust <= ROBUST_MAX_BUCKETS):
            raise ValueError(f"Progressive(robust={robust}): an odd bucket count from 3 to {ROBUST_MAX_BUCKETS}")
        self.robust_buckets = robust
        self.buckets = torch.empty((robust, cam.vsize, cam.hsize, 3), dtype=torch.float64, device="cuda") if robust is not None else None
        shape, dev = (cam.vsize, cam.hsize), "cuda"
        self.frame = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
        self.sum = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
        self.sumsq = torch.empty(shape, dtype=torch.float64, device=dev) if noise else None
        self._mean = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
        self._rgba = torch.empty(shape, dtype=torch.int32, device=dev)
        self._noise = torch.empty(1, dtype=torch.float64, device=dev) if noise else None
        self.stream = torch.cuda.Stream()   # (a stream of its own: the legacy default stream is no stream to the library)
        self.passes = 0

    def step(self):
        """Renders and accumulates pass `passes`; returns the noise estimate after it (a float; None after the first pass
        or without noise)."""
        stream = self.stream.cuda_stream
        self.gpu.set_sample_pass(self.passes)
        self.gpu.render_device(self.cam, self.frame.data_ptr(), self.max_depth, stream=stream)
        n = self.passes + 1
        want_noise = self.noise_on and n >= 2
        a = Accum(self.frame.data_ptr(), self.cam.hsize * self.cam.vsize, n, self.sum.data_ptr(),
                  self.sumsq.data_ptr() if self.sumsq is not None else None, self._mean.data_ptr(), self._rgba.data_ptr(),
                  self._noise.data_ptr() if want_noise else None)
        self.gpu.accumulate_device(a, stream)
        if self.buckets is not None:   # (pass p into bucket p % M, its passes // M + 1-th frame)
            m = self.robust_buckets
            self.gpu.accumulate_device(Accum(self.frame.data_ptr(), self.cam.hsize * self.cam.vsize, self.passes // m + 1,
                                             self.buckets[self.passes % m].data_ptr(), None, None, None, None), stream)
        self.passes = n
        if not want_noise:
            return None
        self.stream.synchronize()
        return float(self._noise.item())

    def mean(self):
        """[h][w][3] f64 on the device: the mean of the passes so far."""
        import torch
        torch.cuda.current_stream().wait_stream(self.stream)
        return self._mean

    def rgba8(self):
        """[h][w][4] u8 on the device: the clamp of mean(), the bits of rgba8_device(mean())."""
        import torch
        torch.cuda.current_stream().wait_stream(self.stream)
        return self._rgba.view(self.cam.vsize, self.cam.hsize, 1).view(torch.uint8)

    def robust(self, gain=1.0):
        """(mean [h][w][3] f64, sumsq [h][w] f64, rejected [h][w] i32) on the device: the Gini-weighted median of means of the
        buckets (rtc_robust_device) after the passes so far (M at least), the sum of squares the denoiser takes with it and
        the buckets left out of each pixel, on this object's stream after its last step.  ValueError on an object built
        without robust=."""
        import torch
        if self.buckets is None:
            raise ValueError("Progressive built without robust=M keeps no bucket sums")
        mean = torch.empty_like(self._mean)
        sumsq = torch.empty((self.cam.vsize, self.cam.hsize), dtype=torch.float64, device=mean.device)
        rejected = torch.empty((self.cam.vsize, self.cam.hsize), dtype=torch.int32, device=mean.device)
        self.stream.wait_stream(torch.cuda.current_stream())   # (the tensors were allocated on the current stream)
        robust_device(self.buckets.data_ptr(), self.cam.hsize * self.cam.vsize, self.passes, mean.data_ptr(), self.stream.cuda_stream,
                      setting=RobustSetting.make(self.robust_buckets, gain), sumsq_ptr=sumsq.data_ptr(), rejected_ptr=rejected.data_ptr())
        torch.cuda.current_stream().wait_stream(self.stream)
        return mean, sumsq, rejected

    def denoised(self, robust=None, **setting):
        """[h][w][3] f64 on the device: the denoiser (rtc_denoise_device) over the mean, the sums of squares and the passes
        so far (two at least), on this object's stream after its last step; `setting`: DenoiseSetting.make's keywords.
        Where `robust` is a dict of robust()'s keywords ({} for the defaults), over the robust mean and its sums of squares
        instead."""
        if robust is not None:
            mean, sumsq, _ = self.robust(**robust)
            return _denoised(self, self.passes, None, setting, mean, sumsq)
        if self.sumsq is None:
            raise ValueError("Progressive(noise=False) keeps no sums of squares: nothing to guide the denoiser")
        return _denoised(self, self.passes, None, setting)

    def filmed(self, denoise=None, robust=None, **film):
        """(out [h][w][3] f64, rgba [h][w][4] u8) on the device: the film stage (rtc_film_device) over the mean - or, where
        `denoise` is a dict of DenoiseSetting.make's keywords, over denoised(**denoise) - on this object's stream after its
        last step; `film`: FilmSetting.make's keywords.  Where `robust` is a dict of robust()'s keywords, the robust mean
        takes the mean's place (under the denoiser too)."""
        if denoise is not None:
            return _filmed(self, self.denoised(robust=robust, **denoise), film)
        return _filmed(self, self.robust(**robust)[0] if robust is not None else self._mean, film)


class AdaptiveProgressive:
    """Adaptive sampling on the device: each step() is one round of rtc_scene_adaptive_step - the tiles still noisy take
    the next sample pass - into torch tensors on the scene's device, on a torch stream of its own (`stream`).  run() steps
    until no tile is active; mean(), rgba8() and tile_passes() order the caller's current stream after the last round.
    The scene's own sample pass is not changed."""

    def __init__(self, gpu_scene, cam, max_depth=REFERENCE_DEPTH, adaptive=None):
        import torch
        if adaptive is None:
            raise ValueError("AdaptiveProgressive: an Adaptive setting is required")
        self.gpu, self.cam, self.max_depth, self.adaptive = gpu_scene, cam, max_depth, adaptive
        shape, dev = (cam.vsize, cam.hsize), "cuda"
        tx, ty = tile_grid(cam.hsize, cam.vsize, adaptive.tile_w, adaptive.tile_h)
        n_tiles = tx * ty
        self.sum = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
        self.sumsq = torch.empty(shape, dtype=torch.float64, device=dev)
        self._mean = torch.empty(shape + (3,), dtype=torch.float64, device=dev)
        self._rgba = torch.empty(shape, dtype=torch.int32, device=dev)
        self._tile_passes = torch.empty(n_tiles, dtype=torch.int32, device=dev)
        self.tile_noise = torch.empty(n_tiles, dtype=torch.float64, device=dev)
        self.active = torch.empty(n_tiles, dtype=torch.int32, device=dev)
        self.n_active = torch.empty(1, dtype=torch.int32, device=dev)
        self.max_noise = torch.empty(1, dtype=torch.float64, device=dev)
        self.state = AdaptiveState(self.sum.data_ptr(), self.sumsq.data_ptr(), self._mean.data_ptr(), self._rgba.data_ptr(),
                                   self._tile_passes.data_ptr(), self.tile_noise.data_ptr(), self.active.data_ptr(),
                                   self.n_active.data_ptr(), self.max_noise.data_ptr(), 0)
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())   # (the buffers were allocated on the current stream)
        self.gpu.adaptive_begin(cam.hsize, cam.vsize, adaptive, self.state, self.stream.cuda_stream)
        self.rounds = 0

    def step(self):
        """One round; returns the number of tiles still active after it (0: done, and nothing was rendered)."""
        n = self.gpu.adaptive_step(self.cam, self.adaptive, self.state, self.max_depth, self.stream.cuda_stream)
        self.rounds = self.state.round
        return n

    def run(self):
        """Rounds until no tile is active; returns the number of rounds."""
        while self.step():
            pass
        return self.rounds

    def _wait(self):
        import torch
        torch.cuda.current_stream().wait_stream(self.stream)

    def mean(self):
        """[h][w][3] f64 on the device: each tile's mean after its passes."""
        self._wait()
        return self._mean

    def rgba8(self):
        """[h][w][4] u8 on the device: the clamp of mean()."""
        import torch
        self._wait()
        return self._rgba.view(self.cam.vsize, self.cam.hsize, 1).view(torch.uint8)

    def tile_passes(self):
        """[T] int32 on the device: the passes each tile has taken."""
        self._wait()
        return self._tile_passes

    def denoised(self, **setting):
        """[h][w][3] f64 on the device: the denoiser (rtc_denoise_device) over the mean, the sums of squares and every
        tile's passes, on this object's stream after its last round; `setting`: DenoiseSetting.make's keywords."""
        return _denoised(self, 0, self._tile_passes, setting)

    def filmed(self, denoise=None, **film):
        """(out [h][w][3] f64, rgba [h][w][4] u8) on the device: the film stage (rtc_film_device) over the mean - or, where
        `denoise` is a dict of DenoiseSetting.make's keywords, over denoised(**denoise) - on this object's stream after its
        last round; `film`: FilmSetting.make's keywords."""
        return _filmed(self, self.denoised(**denoise) if denoise is not None else self._mean, film)


def denoise_device(mean_ptr, sumsq_ptr, hsize, vsize, out_ptr, stream, passes=0, tile_passes_ptr=None, tile=(0, 0), setting=None,
                   rgba_ptr=None):
    """rtc_denoise_device: the denoiser over a device image [vsize][hsize][3] and its sums of squares, enqueued on `stream`
    (a HIP stream, not None); `passes` behind every pixel, or tile_passes_ptr ([T] u32 on the device) with tile = (w, h);
    setting: a DenoiseSetting (None: the defaults); rgba_ptr: where the clamp of the result goes, or None."""
    d = Denoise(mean_ptr, sumsq_ptr, hsize, vsize, passes, tile_passes_ptr, tile[0], tile[1], setting if setting is not None else DenoiseSetting.make(),
                out_ptr, rgba_ptr)
    _check_hip(hip_lib().rtc_denoise_device(C.byref(d), stream))


def denoise_tile():
    """rtc_diag_denoise_tile: (w, h) of the tiled denoise kernels' output tile."""
    w, h = C.c_uint32(), C.c_uint32()
    _check_hip(hip_lib().rtc_diag_denoise_tile(C.byref(w), C.byref(h)))
    return w.value, h.value


def _denoised(prog, passes, tile_passes, setting, mean=None, sumsq=None):
    """Progressive.denoised / AdaptiveProgressive.denoised: a new tensor, filled on prog.stream; the caller's current stream
    is ordered after it.  mean, sumsq: the pair to filter in place of the object's own (the robust one)."""
    import torch
    mean, sumsq = mean if mean is not None else prog._mean, sumsq if sumsq is not None else prog.sumsq
    out = torch.empty_like(mean)
    prog.stream.wait_stream(torch.cuda.current_stream())   # (`out` was allocated on the current stream)
    tile = (prog.adaptive.tile_w, prog.adaptive.tile_h) if tile_passes is not None else (0, 0)
    denoise_device(mean.data_ptr(), sumsq.data_ptr(), prog.cam.hsize, prog.cam.vsize, out.data_ptr(), prog.stream.cuda_stream,
                   passes=passes, tile_passes_ptr=tile_passes.data_ptr() if tile_passes is not None else None, tile=tile,
                   setting=DenoiseSetting.make(**setting))
    torch.cuda.current_stream().wait_stream(prog.stream)
    return out


def robust_device(sums_ptr, n_pixels, passes, mean_ptr, stream, setting=None, sumsq_ptr=None, rejected_ptr=None, rgba_ptr=None):
    """rtc_robust_device: the Gini-weighted median of means over bucket sums [M][n][3] on the device after `passes` passes
    dealt round-robin, enqueued on `stream` (a HIP stream, not None); setting: a RobustSetting (None: the defaults);
    mean_ptr: [n][3] f64; sumsq_ptr: [n] f64 for the denoiser, rejected_ptr: [n] u32, rgba_ptr: the clamp of the mean, or None."""
    r = Robust(sums_ptr, n_pixels, passes, setting if setting is not None else RobustSetting.make(), mean_ptr, sumsq_ptr, rejected_ptr, rgba_ptr)
    _check_hip(hip_lib().rtc_robust_device(C.byref(r), stream))


def robust_grid():
    """rtc_diag_robust_grid: (max_blocks, block) - the cap of rtc_robust_device's grid and the threads of a block."""
    a, b = C.c_uint32(), C.c_uint32()
    _check_hip(hip_lib().rtc_diag_robust_grid(C.byref(a), C.byref(b)))
    return a.value, b.value


def film_scratch_bytes(hsize, vsize, setting=None):
    """rtc_film_scratch_bytes: the bytes of device memory rtc_film_device needs beside its images for a size and a
    FilmSetting (None: the defaults); 0 where it needs none.  A setting the contract refuses raises RtcError."""
    lib = hip_lib()
    n = lib.rtc_film_scratch_bytes(hsize, vsize, C.byref(setting if setting is not None else FilmSetting.make()))
    if n == 0 and lib.rtc_last_error():
        raise RtcError("InvalidArgument", lib.rtc_last_error().decode())
    return n


def film_device(in_ptr, hsize, vsize, out_ptr, stream, setting=None, scratch_ptr=None, rgba_ptr=None, scale_ptr=None):
    """rtc_film_device: the film stage over a device image [vsize][hsize][3], enqueued on `stream` (a HIP stream, not None);
    setting: a FilmSetting (None: the defaults); scratch_ptr: film_scratch_bytes() bytes on the device (None where that is
    0); rgba_ptr: where the clamp of the result goes, or None; scale_ptr: where the exposure E goes (one f64), or None."""
    f = Film(in_ptr, hsize, vsize, setting if setting is not None else FilmSetting.make(), scratch_ptr, out_ptr, rgba_ptr, scale_ptr)
    _check_hip(hip_lib().rtc_film_device(C.byref(f), stream))


def film_tile():
    """rtc_diag_film_tile: (row_w, col_w, col_h) - the width of the tiled row kernel's tile, the width and the height of the
    tiled resolve kernel's."""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check_hip(hip_lib().rtc_diag_film_tile(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def _filmed(prog, image, film):
    """Progressive.filmed / AdaptiveProgressive.filmed: new tensors, filled on prog.stream; the caller's current stream is
    ordered after it."""
    import torch
    setting = FilmSetting.make(**film)
    h, w = prog.cam.vsize, prog.cam.hsize
    out = torch.empty_like(image)
    rgba = torch.empty((h, w), dtype=torch.int32, device=image.device)
    n = film_scratch_bytes(w, h, setting)
    scratch = torch.empty((n + 7) // 8, dtype=torch.float64, device=image.device) if n else None
    prog.stream.wait_stream(torch.cuda.current_stream())   # (the tensors were allocated on the current stream)
    film_device(image.data_ptr(), w, h, out.data_ptr(), prog.stream.cuda_stream, setting=setting,
                scratch_ptr=scratch.data_ptr() if scratch is not None else None, rgba_ptr=rgba.data_ptr())
    torch.cuda.current_stream().wait_stream(prog.stream)
    return out, rgba.view(h, w, 1).view(torch.uint8)


def canvas_register(array):
    """rtc_canvas_register: pins a caller-owned numpy canvas for the HIP runtime (copies into it then run at link
    speed).  The caller keeps the array alive and calls canvas_unregister before dropping it."""
    _check_hip(hip_lib().rtc_canvas_register(array.ctypes.data, array.nbytes))


def canvas_unregister(array):
    _check_hip(hip_lib().rtc_canvas_unregister(array.ctypes.data))


def build_tables_digest(desc):
    """rtc_diag_build_tables: (digest, ms) of the host half of rtc_scene_create for a scene description - no device needed."""
    digest, ms = C.c_uint64(0), C.c_double(0.0)
    _check_hip(hip_lib().rtc_diag_build_tables(C.byref(desc), C.byref(digest), C.byref(ms)))
    return digest.value, ms.value


def root_boxes(desc):
    """rtc_diag_root_boxes: (boxes [n][7] f32: lo, hi, line_only; world_index [n] u32; (cull_bmax, cull_par)) of a scene
    description, as rtc_scene_create builds them - no device needed."""
    lib = hip_lib()
    n = C.c_uint32(0)
    f32p = C.POINTER(C.c_float)
    lib.rtc_diag_root_boxes.argtypes = [C.c_void_p, f32p, _u32p, C.c_uint32, _u32p, f32p]
    _check_hip(lib.rtc_diag_root_boxes(C.byref(desc), None, None, 0, C.byref(n), None))
    boxes = np.zeros((n.value, 7), dtype=np.float32)
    order = np.zeros(n.value, dtype=np.uint32)
    scales = np.zeros(2, dtype=np.float32)
    _check_hip(lib.rtc_diag_root_boxes(C.byref(desc), boxes.ctypes.data_as(f32p), order.ctypes.data_as(_u32p), n.value, C.byref(n),
                                       scales.ctypes.data_as(f32p)))
    return boxes, order, (float(scales[0]), float(scales[1]))


def root_spheres(desc):
    """rtc_diag_root_spheres: (spheres [n][4] f32: centre, radius squared - in root_boxes' table order; cull_cmax) of a scene
    description, as rtc_scene_create builds them - no device needed."""
    lib = hip_lib()
    n, cmax = C.c_uint32(0), C.c_float(0.0)
    f32p = C.POINTER(C.c_float)
    lib.rtc_diag_root_spheres.argtypes = [C.c_void_p, f32p, C.c_uint32, _u32p, f32p]
    _check_hip(lib.rtc_diag_root_spheres(C.byref(desc), None, 0, C.byref(n), None))
    spheres = np.zeros((n.value, 4), dtype=np.float32)
    _check_hip(lib.rtc_diag_root_spheres(C.byref(desc), spheres.ctypes.data_as(f32p), n.value, C.byref(n), C.byref(cmax)))
    return spheres, float(cmax.value)


ROOT_ALONE = 0x800  # RTC_ROOT_ALONE_FLAG (rtc_diag.h)


def root_flags(desc):
    """rtc_diag_root_flags: the kind_flags word [n] u32 of every root record - in root_boxes' table order - of a scene
    description, as rtc_scene_create builds them - no device needed.  Bit ROOT_ALONE: DESIGN.md section 5."""
    lib = hip_lib()
    n = C.c_uint32(0)
    lib.rtc_diag_root_flags.argtypes = [C.c_void_p, _u32p, C.c_uint32, _u32p]
    _check_hip(lib.rtc_diag_root_flags(C.byref(desc), None, 0, C.byref(n)))
    flags = np.zeros(n.value, dtype=np.uint32)
    _check_hip(lib.rtc_diag_root_flags(C.byref(desc), flags.ctypes.data_as(_u32p), n.value, C.byref(n)))
    return flags


def set_option(name, value):
    """rtc_set_option: a process-wide tuning / test option of the library (include/rtc_diag.h lists them)."""
    _check_hip(hip_lib().rtc_set_option(name.encode(), float(value)))


def set_loader_threads(threads):
    """rtch_set_loader_threads: threads HostScene's loader may build a scene's objects on (0: automatic, 1: one loop)."""
    host_lib().rtch_set_loader_threads(int(threads))


def canvas_ppm(rgb):
    """Canvas.ppm (canvas.zig:181-254) of an [h][w][3] f64 array."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    h, w, _ = rgb.shape
    n = host_lib().rtch_canvas_ppm(rgb.ctypes.data, w, h, None, 0)
    buf = C.create_string_buffer(n)
    host_lib().rtch_canvas_ppm(rgb.ctypes.data, w, h, buf, n)
    return buf.raw[:n].decode()


def canvas_rgba8(rgb):
    """RGBA8 framebuffer of lib.zig:146-153."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    h, w, _ = rgb.shape
    out = np.empty((h, w, 4), dtype=np.uint8)
    host_lib().rtch_canvas_rgba8(rgb.ctypes.data, w, h, out.ctypes.data)
    return out


# ---- multi-GPU tile partition: interleaved tiles, one gather, un-permute on rank 0
def tile_grid(hsize, vsize, tile_w, tile_h):
    return (hsize + tile_w - 1) // tile_w, (vsize + tile_h - 1) // tile_h


def tiles_of_rank(n_tiles, rank, world):
    """Tiles rank, rank+world, ... of the row-major tiling.  Returns (first_tile, stride, count, padded_count):
    `count` tiles are rendered, `padded_count` = ceil(n_tiles / world) is the size of every rank's buffer so that one
    equal-count gather suffices; slots count..padded_count-1 are never written (allocate the buffer zeroed)."""
    count = (n_tiles - rank + world - 1) // world if rank < n_tiles else 0
    padded = (n_tiles + world - 1) // world
    return rank, world, count, padded


def assign_tiles(tile_cost, world):
    """rtc_assign_tiles: (rank_of_tile, slot_of_tile) of a cost-balanced split; slot = rank * ceil(n / world) + k."""
    cost = np.ascontiguousarray(tile_cost, dtype=np.float64)
    rank_of = np.empty(len(cost), dtype=np.uint32)
    slot_of = np.empty(len(cost), dtype=np.uint32)
    _check_hip(hip_lib().rtc_assign_tiles(cost.ctypes.data_as(_dp), len(cost), world, rank_of.ctypes.data_as(_u32p),
                                          slot_of.ctypes.data_as(_u32p)))
    return rank_of, slot_of


def assemble_tile_list_device(d_gathered_ptr, d_slot_of_tile_ptr, tile_w, tile_h, hsize, vsize, d_canvas_ptr, stream):
    _check_hip(hip_lib().rtc_assemble_tile_list_device(d_gathered_ptr, d_slot_of_tile_ptr, tile_w, tile_h, hsize, vsize,
                                                       d_canvas_ptr, stream))


def assemble_tile_list_rgba8_device(d_gathered_rgba_ptr, d_slot_of_tile_ptr, tile_w, tile_h, hsize, vsize, d_rgba_ptr, stream):
    """Shares clamped to RGBA8 before the gather (rgba8_device on a rank's tile buffer) -> the [vsize][hsize] u32 framebuffer."""
    _check_hip(hip_lib().rtc_assemble_tile_list_rgba8_device(d_gathered_rgba_ptr, d_slot_of_tile_ptr, tile_w, tile_h, hsize, vsize,
                                                             d_rgba_ptr, stream))


def rgba8_device(d_canvas_ptr, n_pixels, d_rgba_ptr, stream):
    """rtc_rgba8_device: the clamp of color.zig:61-71 alone, device to device, asynchronous on `stream`."""
    _check_hip(hip_lib().rtc_rgba8_device(d_canvas_ptr, n_pixels, d_rgba_ptr, stream))


def assemble_tiles_device(d_gathered_ptr, world, padded, tile_w, tile_h, hsize, vsize, d_canvas_ptr, stream):
    """Device-side twin of assemble_tiles (rank 0, after the gather); asynchronous on `stream`."""
    _check_hip(hip_lib().rtc_assemble_tiles_device(d_gathered_ptr, world, padded, tile_w, tile_h, hsize, vsize,
                                                   d_canvas_ptr, stream))


def assemble_tiles(gathered, hsize, vsize, tile_w, tile_h, world):
    """gathered: [world][padded][tile_h][tile_w][3] -> [vsize][hsize][3] canvas (row-major, canvas.zig:132)."""
    tx, ty = tile_grid(hsize, vsize, tile_w, tile_h)
    n_tiles = tx * ty
    out = np.zeros((ty * tile_h, tx * tile_w, 3), dtype=gathered.dtype)
    for t in range(n_tiles):
        r, k = t % world, t // world
        y, x = divmod(t, tx)
        out[y * tile_h:(y + 1) * tile_h, x * tile_w:(x + 1) * tile_w] = gathered[r, k]
    return out[:vsize, :hsize]
