"""ctypes binding of the mesh-texture checker (tests/build/libmeshuv_oracle.so, tests/cpp/meshuv_oracle.cpp).  TEST
INFRASTRUCTURE.

The checker is the torus checker with the mesh mapping (RTC_TEX_MESH).  The oracle under it knows no
such mapping, so MeshUvScene hands it a copy of the flattened description in which every mesh map is a placeholder planar
map (and every torus a placeholder sphere, torus_binding's way), and a side table: which tex_* entries are mesh maps, and
the texture row of every triangle, keyed by its Shape.id (leaf_id).  Everything else - (desc, light table, camera, depth,
light seed, rtc_sampling, sample pass, displacements, spots, bumps) -> image and ray counts - is as torus_binding.TorusScene.
KAT entry: (tu, tv) of rows at barycentrics.
"""
import ctypes as C
import importlib
import os

import numpy as np

import bump_binding as bb
import torus_binding as tb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHUV_SO = os.path.join(REPO, "tests", "build", "libmeshuv_oracle.so")
MESHUV_DIR = os.path.join(REPO, "tests", "golden", "meshuv_scenes")
MESH_MIX = os.path.join(MESHUV_DIR, "mesh_mix.json")
RTC_TEX_PLANAR, RTC_TEX_MESH = 1, 4
RTC_TRIANGLE, RTC_SMOOTH_TRIANGLE = 4, 5

_lib = None


def lib():
    global _lib
    if _lib is None:
        rtc = importlib.import_module("ray-tracer-challenge_amd")
        l = C.CDLL(MESHUV_SO)
        l.area_last_error.restype = C.c_char_p
        l.area_scene_create.argtypes = [C.POINTER(rtc.SceneDesc), C.POINTER(rtc.LightDesc), C.POINTER(C.c_void_p)]
        l.area_scene_destroy.argtypes = [C.c_void_p]
        l.area_scene_destroy.restype = None
        l.bump_table_create.argtypes = [C.POINTER(rtc.SceneDesc), C.POINTER(rtc.Bump), C.POINTER(C.c_void_p)]
        l.bump_table_destroy.argtypes = [C.c_void_p]
        l.bump_table_destroy.restype = None
        l.torus_table_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        l.torus_table_destroy.argtypes = [C.c_void_p]
        l.torus_table_destroy.restype = None
        l.meshuv_table_create.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        l.meshuv_table_destroy.argtypes = [C.c_void_p]
        l.meshuv_table_destroy.restype = None
        render_args = ([C.POINTER(rtc.Camera), C.c_uint32, C.c_uint64, C.POINTER(rtc.Sampling), C.c_uint32, C.c_void_p, C.c_uint32]
                       + [C.c_void_p] * 4 + [C.c_uint32] * 6 + [C.c_void_p] * 2)
        l.torus_render.argtypes = [C.c_void_p] * 3 + render_args
        l.meshuv_render.argtypes = [C.c_void_p] * 4 + render_args
        l.meshuv_kat_texcoord_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        l.meshuv_kat_texcoord_many.restype = None
        _lib = l
    return _lib


def mix(rtc):
    """mesh_mix.json"""
    return rtc.HostScene.from_file(MESH_MIX, MESHUV_DIR)


def mesh_maps_of(desc):
    """the tex_* entries of mapping RTC_TEX_MESH"""
    return [i for i in range(desc.n_texmaps) if desc.tex_mapping[i] == RTC_TEX_MESH]


def triangles_of(desc):
    """[(leaf, Shape.id, tri_* index)] of the description's triangles"""
    return [(i, int(desc.leaf_id[i]), int(desc.leaf_geom[i])) for i in range(desc.n_leaves)
            if desc.leaf_kind[i] in (RTC_TRIANGLE, RTC_SMOOTH_TRIANGLE)]


def with_placeholders(desc, mapping=RTC_TEX_PLANAR):
    """-> (a copy of desc whose tori are spheres and whose mesh maps have `mapping`, the arrays it points into)"""
    d, kinds = tb.with_placeholders(desc)
    maps = np.array([desc.tex_mapping[i] for i in range(desc.n_texmaps)], dtype=np.uint8)
    maps[maps == RTC_TEX_MESH] = mapping
    d.tex_mapping = maps.ctypes.data_as(C.POINTER(C.c_uint8))
    return d, (kinds, maps)


class MeshUvScene:
    def __init__(self, desc, lights, bumps=None, uvs=None, side_table=True):
        """bumps: a dict as GpuScene.set_bumps takes (None: every kind none); uvs: (n_tris, 6) rows as GpuScene.set_mesh_uvs
        takes (None: no table - every row six zeros); side_table False: no map is a mesh map (the placeholders as they are)"""
        rtc = importlib.import_module("ray-tracer-challenge_amd")
        self._s, self._t, self._q, self._u = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        pdesc, arrays = with_placeholders(desc)
        self._keep = (desc, lights, pdesc, arrays)
        self.n_roots = desc.n_roots
        self.n_lights = lights.n_lights
        if lib().area_scene_create(C.byref(pdesc), C.byref(lights), C.byref(self._s)) != 0:
            raise RuntimeError("meshuv checker: " + lib().area_last_error().decode())
        bp = None
        if bumps is not None:
            b, _keep = rtc.bump_struct(bumps)
            bp = C.byref(b)
        if lib().bump_table_create(C.byref(pdesc), bp, C.byref(self._t)) != 0:
            raise RuntimeError("meshuv checker: " + lib().area_last_error().decode())
        tori = tb.tori_of(desc)
        ids = np.array([t[1] for t in tori], dtype=np.uint64)
        major = np.array([t[2] for t in tori], dtype=np.float64)
        minor = np.array([t[3] for t in tori], dtype=np.float64)
        if lib().torus_table_create(ids.ctypes.data, major.ctypes.data, minor.ctypes.data, len(ids), C.byref(self._q)) != 0:
            raise RuntimeError("meshuv checker: " + lib().area_last_error().decode())
        is_mesh = np.zeros(desc.n_texmaps if side_table else 0, dtype=np.uint8)
        if side_table:
            is_mesh[mesh_maps_of(desc)] = 1
        tris = triangles_of(desc) if (side_table and uvs is not None) else []
        tri_ids = np.array([t[1] for t in tris], dtype=np.uint64)
        rows = np.ascontiguousarray([np.asarray(uvs, dtype=np.float64)[t[2]] for t in tris], dtype=np.float64).reshape(len(tris), 6)
        if lib().meshuv_table_create(is_mesh.ctypes.data, len(is_mesh), tri_ids.ctypes.data, rows.ctypes.data, len(tris), C.byref(self._u)) != 0:
            raise RuntimeError("meshuv checker: " + lib().area_last_error().decode())

    _args = bb.BumpScene._args

    def _render(self, fn, head, cam, max_depth, smp, spots, disp, sample_pass, light_seed, tile, threads):
        (x0, y0, w, h), (d, cone, axis, ci, co), smp_p = self._args(cam, smp, spots, disp, tile)
        out = np.zeros((h, w, 3), dtype=np.float64)
        counters = np.zeros(3, dtype=np.uint64)
        if fn(*head, C.byref(cam), max_depth, light_seed, smp_p, sample_pass, d.ctypes.data, self.n_roots, cone.ctypes.data,
              axis.ctypes.data, ci.ctypes.data, co.ctypes.data, len(cone), x0, y0, w, h, threads, out.ctypes.data,
              counters.ctypes.data) != 0:
            raise RuntimeError("meshuv checker: " + lib().area_last_error().decode())
        return out, dict(zip(["primary", "secondary", "shadow_calls"], (int(c) for c in counters)))

    def render(self, cam, max_depth=5, smp=None, spots=None, disp=None, sample_pass=0, light_seed=0, tile=None, threads=0):
        """-> ([h][w][3] f64, {"primary", "secondary", "shadow_calls"})"""
        return self._render(lib().meshuv_render, (self._s, self._t, self._q, self._u), cam, max_depth, smp, spots, disp, sample_pass,
                            light_seed, tile, threads)

    def render_torus(self, cam, max_depth=5, smp=None, spots=None, disp=None, sample_pass=0, light_seed=0, threads=0):
        """the included torus checker's own render (torus_render) - the placeholder maps as planar maps -, for the identity
        of a scene without a mesh map"""
        return self._render(lib().torus_render, (self._s, self._t, self._q), cam, max_depth, smp, spots, disp, sample_pass, light_seed,
                            None, threads)

    def close(self):
        for name, free in (("_u", "meshuv_table_destroy"), ("_q", "torus_table_destroy"), ("_t", "bump_table_destroy"),
                           ("_s", "area_scene_destroy")):
            if getattr(self, name):
                getattr(lib(), free)(getattr(self, name))
                setattr(self, name, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def texcoords(rows, u, v):
    """(tu, tv) of rows [n][6] at the barycentrics u, v [n] -> [n][2]"""
    r = np.ascontiguousarray(rows, dtype=np.float64)
    a = np.ascontiguousarray(u, dtype=np.float64)
    b = np.ascontiguousarray(v, dtype=np.float64)
    out = np.zeros((len(a), 2))
    lib().meshuv_kat_texcoord_many(r.ctypes.data, a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data)
    return out
