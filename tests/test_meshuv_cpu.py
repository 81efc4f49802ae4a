"""UV-mapped mesh textures without a GPU (RTC_TEX_MESH): the loader ("texture-coordinates", `vt`, the
faces' t fields, "uv1".."uv3", the "mesh" mapping), the flattener (texture rows in tri_* order, the reference scenes'
tables unchanged), the checker against an independent statement of rtc.h's formula and against the torus checker, the C
ABI's refusals that need no device, the header, the documents and the recorded disassembly identity."""
import ctypes as C
import hashlib
import json
import math
import os

import numpy as np
import pytest

import meshuv_binding as mb
import torus_binding as tb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(REPO, "tests", "golden", "scenes")
CAMERA = {"width": 40, "height": 30, "field-of-view": 0.8, "from": [0, 1, -5], "to": [0, 0.5, 0], "up": [0, 1, 0]}
LIGHTS = [{"point-light": {"position": [-4, 8, -6], "intensity": [1, 1, 1]}}]
MESH_TEST = {"pattern": {"type": {"texture-map": {"mesh": {"uv-pattern": {"test": {}}}}}}}


def _scene(objects, **more):
    return json.dumps({"camera": CAMERA, "lights": LIGHTS, "objects": objects, **more})


def _obj_scene(rtc, tmp_path, text, key=True, material=None, **cfg):
    (tmp_path / "m.obj").write_text(text)
    o = {"file": "m.obj", "normalize": False, **cfg}
    if key is not None:
        o["texture-coordinates"] = key
    return rtc.HostScene(_scene([{"type": {"from-obj": o}, "material": material or MESH_TEST}]), str(tmp_path))


QUAD = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1 0.5\nvt 0 1\n"


# ---- the loader: OBJ
def test_vt_lines_are_one_indexed_and_a_fan_takes_first_last_current(rtc, tmp_path):
    hs = _obj_scene(rtc, tmp_path, QUAD + "v 0.5 1.5 0\nvt 0.5 2\nf 1/1 2/2 3/3 4/4 5/5\n")
    assert hs.desc.n_tris == 3
    rows = hs.mesh_uvs()
    assert rows.tolist() == [[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1], [0, 0, 0, 1, 0.5, 2]]
    # the t field and the v field are independent indices
    hs = _obj_scene(rtc, tmp_path, QUAD + "f 1/3 2/4 3/1\n")
    assert hs.mesh_uvs().tolist() == [[1, 1, 0, 1, 0, 0]]


def test_a_vertex_without_t_and_v_t_n_and_v_slash_slash_n(rtc, tmp_path):
    hs = _obj_scene(rtc, tmp_path, QUAD + "vn 0 0 -1\nf 1/2/1 2//1 3/4/1\nf 1/2 2 3/4\n")
    d = hs.desc
    assert [d.leaf_kind[i] for i in range(d.n_leaves)] == [5, 4]              # smooth, flat
    assert hs.mesh_uvs().tolist() == [[1, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1]]   # the corner without t: (0, 0)


def test_obj_refusals_by_name(rtc, tmp_path):
    with pytest.raises(rtc.RtcError) as e:
        _obj_scene(rtc, tmp_path, QUAD + "f 1/1 2/2 3/5\n")
    assert e.value.name == "IndexOutOfBounds" and "texture 5" in str(e.value)
    with pytest.raises(rtc.RtcError) as e:
        _obj_scene(rtc, tmp_path, QUAD + "f 1/0 2/2 3/3\n")
    assert e.value.name == "IndexOutOfBounds" and "texture 0" in str(e.value)
    # fewer than two numbers: the loader's IncompleteVertex - a line error, so the line is an ignored line (obj.zig:277)
    # and the list is one entry shorter
    with pytest.raises(rtc.RtcError) as e:
        _obj_scene(rtc, tmp_path, "v 0 0 0\nv 1 0 0\nv 1 1 0\nvt 0 0\nvt 1\nf 1/1 2/2 3/2\n")
    assert e.value.name == "IndexOutOfBounds" and "texture 2" in str(e.value)
    with pytest.raises(rtc.RtcError) as e:
        _obj_scene(rtc, tmp_path, QUAD, key="yes")
    assert "texture-coordinates" in str(e.value)
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene([{"type": {"sphere": {}}, "material": {"pattern": {"type": {"texture-map": {"meshes": {"uv-pattern": {"test": {}}}}}}}}]))
    assert e.value.name == "UnknownField" and "texture-map.meshes" in str(e.value)


def _tables(hs):
    d = hs.desc
    return {f: np.array(hs.array(f, n, w)).copy() for f, n, w in (("leaf_kind", d.n_leaves, 1), ("leaf_geom", d.n_leaves, 1),
            ("leaf_material", d.n_leaves, 1), ("tri_p1", d.n_tris, 3), ("tri_e1", d.n_tris, 3), ("tri_e2", d.n_tris, 3),
            ("tri_n1", d.n_tris, 3), ("mat_params", d.n_materials, 7), ("node_min", d.n_nodes, 3))}


def test_without_the_key_vt_lines_and_junk_t_fields_change_nothing(rtc, tmp_path):
    plain = "v 0 0 0\nv 1 0 0\nv 1 1 0\nvn 0 0 -1\nvn 0 0 -1\nvn 0 0 -1\nf 1 2 3\nf 1//3 2//1 3//2\n"
    junk = "v 0 0 0\nvt 0.5\nv 1 0 0\nvt 1 2 3\nv 1 1 0\nvn 0 0 -1\nvn 0 0 -1\nvn 0 0 -1\nvt x y\nf 1/0 2/102 3/14\nf 1/0/3 2/102/1 3/14/2\n"
    solid = {"pattern": {"type": {"solid": [1, 0, 0]}}}
    a = _obj_scene(rtc, tmp_path, plain, key=None, material=solid)
    for key in (None, False):
        b = _obj_scene(rtc, tmp_path, junk, key=key, material=solid)
        ta, tb_ = _tables(a), _tables(b)
        for f in ta:
            assert np.array_equal(ta[f], tb_[f]), f
        assert b.mesh_uvs() is None
    # (lines_ignored and the line errors' names: test_parser_level_kats below)  With the key the junk t fields are read,
    # and refused
    with pytest.raises(rtc.RtcError) as e:
        _obj_scene(rtc, tmp_path, junk, key=True, material=solid)
    assert e.value.name == "IndexOutOfBounds"


KAT = os.path.join(REPO, "tests", "build", "meshuv_kat")
KAT_CASES = ["key_absent_lines_ignored", "key_absent_every_vt_is_an_unknown_first_token", "key_absent_faces_load_without_rows",
             "vt_lines_change_no_triangle_without_the_key", "key_set_lines_ignored", "vt_with_one_number_is_IncompleteVertex",
             "vt_without_a_number_is_InvalidCharacter", "vt_not_finite_is_NonFiniteVertex", "comment_is_UnknownFirstToken",
             "key_set_rows", "vt_alone_is_IncompleteVertex", "t_out_of_range_is_IndexOutOfBounds"]


def test_parser_level_kats():
    """tests/cpp/meshuv_kat_main.cpp against librtc_host.so: ObjParser::lines_ignored with the key absent is 5 for its text
    - the comment and each of the four `vt` lines, the junk-t faces not: the count the parser of the commit before this
    feature gives for the same text -, with the key set 4, each under its line error's name (`vt 0.5`: IncompleteVertex)."""
    import subprocess
    if not os.path.exists(KAT):
        subprocess.run(["make", "-C", REPO, "tests/build/meshuv_kat"], check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([KAT], capture_output=True, text=True)
    lines = [l.split(" ", 4) for l in p.stdout.splitlines() if l.startswith("KAT meshuv ")]
    assert p.returncode == 0, p.stdout
    assert [l[2] for l in lines] == KAT_CASES and all(l[3] == "PASS" for l in lines), p.stdout
    assert lines[0][4] == "5" and lines[4][4] == "4"


def test_a_vt_that_is_not_finite_is_an_ignored_line(rtc, tmp_path):
    """`vt 1e999 0` never reaches rtc_scene_set_mesh_uvs: the line is ignored, so the list is one entry shorter."""
    hs = _obj_scene(rtc, tmp_path, "v 0 0 0\nv 1 0 0\nv 1 1 0\nvt 1e999 0\nvt 0.5 0.25\nvt inf 1\nf 1/1 2/1 3/1\n")
    assert hs.mesh_uvs().tolist() == [[0.5, 0.25, 0.5, 0.25, 0.5, 0.25]]


# ---- the loader: scene JSON
def _tri(**uv):
    return {"type": {"triangle": {"p1": [-1, 0, 0], "p2": [1, 0, 0], "p3": [0, 1.5, 0], **uv}}, "material": MESH_TEST}


def test_json_triangle_uvs_all_or_none(rtc):
    hs = rtc.HostScene(_scene([_tri(uv1=[0, 0.25], uv2=[1, 0], uv3=[0.5, -2])]))
    assert hs.mesh_uvs().tolist() == [[0, 0.25, 1, 0, 0.5, -2]]
    assert rtc.HostScene(_scene([_tri()])).mesh_uvs() is None
    for given, missing in ((("uv1",), "uv2"), (("uv1", "uv2"), "uv3"), (("uv2", "uv3"), "uv1")):
        with pytest.raises(rtc.RtcError) as e:
            rtc.HostScene(_scene([_tri(**{k: [0, 0] for k in given})]))
        assert "triangle." + missing in str(e.value)
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene([_tri(uv1=[0, 0, 0], uv2=[1, 0], uv3=[0, 1])]))
    assert "triangle.uv1" in str(e.value)


def test_mesh_mapping_in_every_position_of_a_pattern_tree(rtc):
    mesh = {"type": {"texture-map": {"mesh": {"uv-pattern": {"checkers": {"width": 2, "height": 2, "patterns": [
        {"type": {"solid": [1, 0, 0]}}, {"type": {"solid": [0, 0, 1]}}]}}}}}}
    solid = {"type": {"solid": [0, 1, 0]}}
    for wrap in (lambda m: m, lambda m: {"type": {"stripes": [m, solid]}}, lambda m: {"type": {"checkers": [solid, m]}},
                 lambda m: {"type": {"rings": [m, solid]}}, lambda m: {"type": {"perturb": m}}, lambda m: {"type": {"blend": [m, solid]}},
                 lambda m: {"type": {"gradient": [solid, m]}}, lambda m: {"type": {"blend": [{"type": {"gradient": [m, solid]}}, solid]}}):
        t = _tri(uv1=[0, 0], uv2=[1, 0], uv3=[0, 1])
        t["material"] = {"pattern": wrap(mesh)}
        hs = rtc.HostScene(_scene([t]))
        d = hs.desc
        assert [d.tex_mapping[i] for i in range(d.n_texmaps)] == [rtc.RTC_TEX_MESH]
        img, _ = mb.MeshUvScene(d, hs.lights, None, hs.mesh_uvs()).render(hs.camera(), 2)
        assert img.std() > 0


# ---- flattening
def test_rows_follow_tri_order_through_divide_definitions_and_groups(rtc):
    """Every triangle gets a row that names it: uv1 = (k, 0) for the k-th triangle as written.  The loader divides a group
    at 8 children (scene.zig:588): eighteen triangles written alternately into two far clusters are reordered into
    sub-groups.  After that, and after a definition was copied twice, row i still belongs to the triangle at tri_p1[i]."""
    def tri(k, x):
        return {"type": {"triangle": {"p1": [x, 0, 0], "p2": [x + 0.5, 0, 0], "p3": [x, 0.5, 0], "uv1": [k, 0], "uv2": [k, 1], "uv3": [k, 2]}}}
    xs = [(-30 - 0.7 * (k // 2)) if k % 2 == 0 else (30 + 0.7 * (k // 2)) for k in range(18)]
    defs = {"shape-definitions": [{"name": "marked", "value": tri(99, 60.0)}]}
    objects = [{"type": {"group": [tri(k, x) for k, x in enumerate(xs)]}},
               {"type": {"from-definition": "marked"}},
               {"type": {"from-definition": "marked"}, "transform": [{"translate": [0, 3, 0]}]}]
    hs = rtc.HostScene(_scene(objects, **defs))
    d = hs.desc
    rows, p1 = hs.mesh_uvs(), np.array(hs.array("tri_p1", d.n_tris, 3))
    assert d.n_tris == 20 and d.n_nodes > 1
    by_x = {x: k for k, x in enumerate(xs)}
    by_x[60.0] = 99
    for i in range(d.n_tris):
        k = by_x[p1[i, 0]]
        assert rows[i].tolist() == [k, 0, k, 1, k, 2]
    assert rows[:18, 0].tolist() != sorted(rows[:18, 0].tolist())     # divide reordered the group's triangles
    assert np.count_nonzero(rows[:, 0] == 99) == 2                    # the definition's row went with both copies


def _digest(hs):
    d = hs.desc
    h = hashlib.sha256()
    for field, count, width in (("leaf_kind", d.n_leaves, 1), ("leaf_xform", d.n_leaves, 1), ("leaf_material", d.n_leaves, 1),
                                ("leaf_shadow", d.n_leaves, 1), ("leaf_geom", d.n_leaves, 1), ("xf_inv", d.n_xforms, 16),
                                ("cyl_min", d.n_cyls, 1), ("cyl_max", d.n_cyls, 1), ("cyl_closed", d.n_cyls, 1),
                                ("mat_params", d.n_materials, 7), ("mat_pattern", d.n_materials, 1), ("node_min", d.n_nodes, 3),
                                ("node_max", d.n_nodes, 3), ("children", d.n_children, 1), ("roots", d.n_roots, 1),
                                ("tri_p1", d.n_tris, 3), ("tri_e1", d.n_tris, 3), ("tri_e2", d.n_tris, 3)):
        h.update(field.encode())
        h.update(np.ascontiguousarray(hs.array(field, count, width)).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(SCENES) if f.endswith(".json")))
def test_reference_scenes_flatten_to_the_tables_they_had(rtc, name):
    """tests/golden/torus_scenes/reference_tables.json (read, never written here): the digests of the scenes' tables -
    tests/test_torus_cpu.py's statement of them -; and no scene of the repository has a mesh map or a texture row."""
    want = json.load(open(os.path.join(tb.TORUS_DIR, "reference_tables.json")))
    hs = rtc.HostScene.from_file(name)
    assert _digest(hs) == want[name]
    assert not mb.mesh_maps_of(hs.desc) and hs.mesh_uvs() is None


def test_fixture_tables(rtc):
    hs = mb.mix(rtc)
    d = hs.desc
    assert d.n_tris == 262 and len(mb.mesh_maps_of(d)) == 9 and len(tb.tori_of(d)) == 1
    # a mesh is one material row, not one per triangle: the copies of its material share one mesh map
    assert d.n_materials <= 16 and d.n_texmaps == 10
    rows = hs.mesh_uvs()
    assert rows.shape == (262, 6) and rows.min() == -0.5 and rows.max() == 2.25
    assert np.count_nonzero(rows[:, 0::2] == 1.0) > 0                 # the globe's seam column at u = 1.0


# ---- the checker against an independent statement of rtc.h's formula
def _restated(row, u, v):
    a1, b1, a2, b2, a3, b3 = (float(x) for x in row)
    u, v = float(u), float(v)
    w = (1.0 - u) - v
    out = []
    for p1, p2, p3 in ((a1, a2, a3), (b1, b2, b3)):
        x = (p2 * u + p3 * v) + p1 * w
        if x < 0.0 or x > 1.0:
            x = x - math.floor(x)
        out.append(x)
    return out


def test_restatement_equals_the_checker_bit_for_bit():
    rng = np.random.default_rng(19)
    n = 4000
    rows = rng.uniform(-0.5, 2.25, size=(n, 6))
    rows[:500] = rng.uniform(0.0, 1.0, size=(500, 6))
    rows[500:600] = rng.integers(-2, 4, size=(100, 6))               # integer corners: tu, tv land on 0.0, 1.0 and the wrap
    u = rng.uniform(0, 1, n)
    v = rng.uniform(0, 1, n) * (1 - u)
    u[0:n:8] = 0.0                                                    # edges ...
    v[1:n:8] = 0.0
    k = slice(2, n, 8)
    v[k] = 1.0 - u[k]
    u[3:n:16], v[3:n:16] = 0.0, 0.0                                   # ... and vertices
    u[7:n:16], v[7:n:16] = 1.0, 0.0
    u[11:n:16], v[11:n:16] = 0.0, 1.0
    got = mb.texcoords(rows, u, v)
    want = np.array([_restated(rows[i], u[i], v[i]) for i in range(n)])
    assert np.array_equal(got, want)
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert np.count_nonzero(got == 1.0) > 0 and np.count_nonzero(got == 0.0) > 0     # 0.0 and 1.0 stay
    raw = (rows[:, 2] * u + rows[:, 4] * v) + rows[:, 0] * ((1.0 - u) - v)
    assert np.count_nonzero(raw != got[:, 0]) > 500                   # the texture tiled


def test_checker_renders_the_fixture_and_zero_rows_are_the_colour_of_0_0(rtc):
    hs = mb.mix(rtc)
    cam = hs.camera(80, 45)
    full, counters = mb.MeshUvScene(hs.desc, hs.lights, hs.bumps(), hs.mesh_uvs()).render(cam, 5, spots=hs.spots(), disp=hs.motion())
    assert counters["primary"] == 80 * 45 and np.isfinite(full).all() and full.std() > 0.05
    none, _ = mb.MeshUvScene(hs.desc, hs.lights, hs.bumps(), None).render(cam, 5, spots=hs.spots(), disp=hs.motion())
    zero, _ = mb.MeshUvScene(hs.desc, hs.lights, hs.bumps(), np.zeros((hs.desc.n_tris, 6))).render(cam, 5, spots=hs.spots(), disp=hs.motion())
    assert np.array_equal(none, zero) and not np.array_equal(none, full)
    # the quad alone, unlit: every pixel of it is the checkers' colour at (0, 0)
    cam1 = dict(CAMERA, **{"from": [-2.7, 0.5, -4], "to": [-2.7, 0.5, 0], "field-of-view": 0.6})
    obj = {"type": {"from-obj": {"file": "mesh_quads.obj", "normalize": False, "texture-coordinates": True}},
           "material": {"pattern": {"type": {"texture-map": {"mesh": {"uv-pattern": {"checkers": {"width": 4, "height": 4, "patterns": [
               {"type": {"solid": [1, 0.2, 0.2]}}, {"type": {"solid": [0.2, 0.2, 1]}}]}}}}}}, "ambient": 1, "diffuse": 0, "specular": 0}}
    q = rtc.HostScene(json.dumps({"camera": cam1, "lights": LIGHTS, "objects": [obj]}), mb.MESHUV_DIR)
    with_rows, _ = mb.MeshUvScene(q.desc, q.lights, None, q.mesh_uvs()).render(q.camera(), 5)
    without, _ = mb.MeshUvScene(q.desc, q.lights, None, None).render(q.camera(), 5)
    hit = without.sum(axis=2) > 0
    assert hit.sum() > 100 and np.all(without[hit] == np.array([1.0, 0.2, 0.2]))
    assert len(np.unique(with_rows[hit], axis=0)) == 2


def test_no_mesh_map_is_the_torus_checker_bit_for_bit(rtc):
    """The mesh maps swapped for the placeholder and no side table: the stack adds nothing where there is no mesh map."""
    hs = mb.mix(rtc)
    cam = hs.camera(80, 45)
    ck = mb.MeshUvScene(hs.desc, hs.lights, hs.bumps(), hs.mesh_uvs(), side_table=False)
    a, ca = ck.render(cam, 5, spots=hs.spots(), disp=hs.motion(), light_seed=3)
    b, cb_ = ck.render_torus(cam, 5, spots=hs.spots(), disp=hs.motion(), light_seed=3)
    assert np.array_equal(a, b) and ca == cb_
    hs = tb.mix(rtc)
    cam = hs.camera(64, 36)
    ck = mb.MeshUvScene(hs.desc, hs.lights, hs.bumps())
    a, _ = ck.render(cam, 5, spots=hs.spots(), disp=hs.motion())
    b, _ = tb.TorusScene(hs.desc, hs.lights, hs.bumps()).render(cam, 5, spots=hs.spots(), disp=hs.motion())
    assert np.array_equal(a, b)


# ---- the C ABI, without a device
def test_create_refuses_mapping_5_and_multi_refuses_the_fixture(rtc):
    hs = mb.mix(rtc)
    d, keep = mb.with_placeholders(hs.desc, mapping=5)
    out = C.c_void_p()
    assert rtc.hip_lib().rtc_scene_create(C.byref(d), C.byref(out)) == 4          # RTC_ERR_UNSUPPORTED
    assert b"mapping 5" in rtc.hip_lib().rtc_last_error()
    assert rtc.multi_lib().rtc_multi_create(C.byref(hs.desc), 1, 0, C.byref(out)) == 4   # before any device call
    assert b"RTC_TEX_MESH" in rtc.multi_lib().rtc_multi_last_error() and not out.value


def test_abi_names_header_and_option(rtc):
    assert rtc.RTC_TEX_MESH == 4 and "meshuv_kernels" in rtc.KERNEL_OPTIONS
    assert "rtc_scene_set_mesh_uvs" in rtc.RTC_SYMBOLS and "rtch_scene_mesh_uvs" in rtc.HOST_SYMBOLS
    lib = rtc.hip_lib()
    assert lib.rtc_scene_set_mesh_uvs and rtc.host_lib().rtch_scene_mesh_uvs
    assert lib.rtc_scene_set_mesh_uvs(None, None) == 1                            # RTC_ERR_INVALID_ARGUMENT: no handle
    assert lib.rtc_set_option(b"meshuv_kernels", 1.0) == 0 and lib.rtc_set_option(b"meshuv_kernels", 0.0) == 0
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    for line in ("#define RTC_TEX_MESH 4u", "typedef struct rtc_mesh_uvs {", "int rtc_scene_set_mesh_uvs(rtc_scene *scene, const rtc_mesh_uvs *uvs);",
                 "w  = (1.0 - u) - v", "tu = (a2 * u + a3 * v) + a1 * w", "tv = (b2 * u + b3 * v) + b1 * w", "x - floor(x)"):
        assert line in header, line
    assert "rtch_scene_mesh_uvs" in open(os.path.join(REPO, "include", "rtc_host.h")).read()
    assert "meshuv_kernels" in open(os.path.join(REPO, "include", "rtc_diag.h")).read()
    assert "RTC_TEX_MESH" in open(os.path.join(REPO, "include", "rtc_multi.h")).read()


def test_documents_speak_of_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "## 19." in design
    for word in ("RTC_TEX_MESH", "rtc_scene_set_mesh_uvs", "rtc_render_kernel_meshuv", "rtc_render_kernel_meshuv_bigworld", "meshuv_kernels",
                 "texture-coordinates", "tests/cpp/meshuv_oracle.cpp", "profiles/meshuv/disassembly_identity.txt"):
        assert word in design, word
    resources = json.load(open(os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json"))) \
        if os.path.exists(os.path.join(REPO, "ray-tracer-challenge_amd", "lib", "kernel_resources.json")) else None
    if resources is not None:   # (a built tree: DESIGN's resources row of the new kernels is the build's)
        k = resources.get("kernels", resources)["rtc_render_kernel_meshuv"]
        assert f"| `rtc_render_kernel_meshuv` | {k['vgprs']} | {k['vgprs_spilled']} | {k['sgprs_spilled']} | {k['scratch_bytes_per_lane']} |" in design
    for doc, word in (("README.md", "rtc_scene_set_mesh_uvs"), ("INTEGRATION.md", "rtc_scene_set_mesh_uvs"), (os.path.join("tools", "README.md"), "--meshuv")):
        assert word in open(os.path.join(REPO, doc)).read(), (doc, word)


def test_disassembly_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "meshuv", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_torus.o", "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_meshuv", "rtc_render_kernel_meshuv_bigworld", "rtc_render_kernel_torus", "rtc_render_kernel_simple3_b"):
        assert kernel in text
