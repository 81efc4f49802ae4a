"""A hit on a transparent top-level sphere or cube that is ALONE takes n1 and n2 from that root's own two entries instead of
the containers pass over every root (csrc/rtc_kernels.hip: render_body, kOwnRoot; csrc/rtc_capi.hip: markAloneRoots; DESIGN.md
section 5).  H is alone in a world of top-level spheres, planes and cubes when
  1. every other root's material has a refractive index of exactly 1.0,
  2. H's world box and every other bounded root's are apart on some axis by more than 1e-6 of the larger box's diagonal,
  3. H's world box, grown by H's margin, lies wholly on one side of every plane.  A sphere's margin is 1e-6 of its box's
     diagonal; a cube's is 0.05 x its largest half-extent (the lengths of its transform's columns), all of them <= 1e3.
Here, on the CPU: which roots rtc_scene_create marks (rtc_diag_root_flags) on the committed scenes and on worlds that miss one
condition each, and the reduction itself - in float64, on the reference's entries (tests/test_root_boxes_cpu.py:
_reference_entries, with the cube's parallel rule), the visitor's rule over all roots' entries against the same rule over H's
entries alone, for every ray whose closest hit is H."""
import json

import numpy as np
import pytest

from test_root_boxes_cpu import _object_rays, _reference_entries

INF = float("inf")
ALONE = 0x800


def _glass(ior=1.5):
    return {"transparency": 0.8, "refractive-index": ior, "reflective": 0.2, "diffuse": 0.2, "ambient": 0.1}


def _obj(kind, transform, material=None):
    return {"type": {kind: {}}, "transform": transform, "material": material if material is not None else {"diffuse": 0.7}}


def _scene(objs):
    camera = {"width": 16, "height": 12, "field-of-view": 1.0, "from": [0, 1, -8], "to": [0, 0, 0], "up": [0, 1, 0]}
    lights = [{"point-light": {"position": [-3, 6, -5], "intensity": [1, 1, 1]}}]
    return json.dumps({"camera": camera, "lights": lights, "objects": objs})


def _alone(rtc, desc):
    """{World.objects index: the root is marked alone}"""
    flags = rtc.root_flags(desc)
    _, order, _ = rtc.root_boxes(desc)
    return {int(order[pos]): bool(flags[pos] & ALONE) for pos in range(desc.n_roots)}


def _forward(desc, leaf):
    m = np.ctypeslib.as_array(desc.xf_inv, shape=(desc.n_xforms * 16,))[16 * desc.leaf_xform[leaf]:16 * desc.leaf_xform[leaf] + 16]
    return np.linalg.inv(m.reshape(4, 4)), m.reshape(4, 4).copy()


def _world_box(fwd):
    corners = np.array([[x, y, z, 1.0] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]) @ fwd.T
    return corners[:, :3].min(axis=0), corners[:, :3].max(axis=0)


def _ior(desc, leaf):
    return float(desc.mat_params[7 * desc.leaf_material[leaf] + 6])


def _conditions(desc):
    """The three conditions restated on the description: {World.objects index: alone}, None for a world that is not simple."""
    n = desc.n_roots
    leaves = [desc.roots[i] for i in range(n)]
    if desc.n_nodes != 0 or any(l & 0x80000000 or desc.leaf_kind[l] > 2 for l in leaves):
        return None
    if n > 128 or desc.n_materials > 64 or desc.n_patterns > 48 or desc.n_lights > 16:   # (RTC_LDS_*: what the simple kernels hold)
        return None
    kinds = [desc.leaf_kind[l] for l in leaves]
    fwd = [_forward(desc, l) for l in leaves]
    boxes = [_world_box(f[0]) if k != 1 else None for f, k in zip(fwd, kinds)]
    diag = [float(np.linalg.norm(b[1] - b[0])) if b is not None else 0.0 for b in boxes]
    out = {}
    for i in range(n):
        out[i] = False
        if kinds[i] == 1 or any(_ior(desc, leaves[j]) != 1.0 for j in range(n) if j != i):
            continue
        margin = 1e-6 * diag[i]
        if kinds[i] == 2:
            s = np.linalg.norm(fwd[i][0][:3, :3], axis=0)
            if s.max() > 1e3:
                continue
            margin = 0.05 * s.max()
        ok = True
        for j in range(n):
            if j == i:
                continue
            if kinds[j] != 1:
                gap = 1e-6 * max(diag[i], diag[j])
                ok = ok and bool(np.any(boxes[i][0] - boxes[j][1] > gap) or np.any(boxes[j][0] - boxes[i][1] > gap))
            else:
                lo, hi = boxes[i][0] - margin, boxes[i][1] + margin
                row = fwd[j][1][1]
                ys = [row[0] * x + row[1] * y + row[2] * z + row[3] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
                ok = ok and (all(v > 0 for v in ys) or all(v < 0 for v in ys))
        out[i] = ok
    return out


def test_exactly_the_glass_sphere_of_cover_is_alone(rtc):
    hs = rtc.HostScene.from_file("cover.json")
    desc = hs.desc
    alone = _alone(rtc, desc)
    marked = [i for i, a in alone.items() if a]
    assert len(marked) == 1, marked
    leaf = desc.roots[marked[0]]
    assert desc.leaf_kind[leaf] == 0 and _ior(desc, leaf) == 1.5
    assert float(desc.mat_params[7 * desc.leaf_material[leaf] + 5]) > 0.0   # (it is transparent: the pass is made for its hits)
    assert alone == _conditions(desc)


@pytest.mark.parametrize("name", ["cubes.json", "reflection_and_refraction.json", "fresnel.json", "skybox_demo.json"])
def test_flags_of_other_committed_scenes_are_what_the_conditions_say(rtc, name):
    desc = rtc.HostScene.from_file(name).desc
    alone = _alone(rtc, desc)
    want = _conditions(desc)
    print(name, "alone:", [i for i, a in alone.items() if a], "of", desc.n_roots, "roots;", "simple" if want is not None else "not a simple world")
    assert alone == (want if want is not None else {i: False for i in range(desc.n_roots)})


def _sphere_at(x, r=1.0, material=None):
    return _obj("sphere", [{"scale": [r, r, r]}, {"translate": [x, 0, 0]}], material)


def test_a_world_that_qualifies_and_worlds_that_miss_one_condition(rtc):
    floor = _obj("plane", [{"translate": [0, -3, 0]}])
    glass = _sphere_at(0.0, 1.0, _glass())
    diag = 2.0 * np.sqrt(3.0)   # of the unit sphere's box, the larger of the two below

    def marked(objs):
        return _alone(rtc, rtc.HostScene(_scene(objs)).desc)

    # the margin between two boxes is 1e-6 of the larger diagonal: just beyond it the sphere is alone, just under it not
    assert marked([glass, _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [1.5 + 1.5e-6 * diag, 0, 0]}]), floor])[0] is True
    cases = {
        "boxes touch (gap 0)": [glass, _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [1.5, 0, 0]}]), floor],
        "gap just under the margin": [glass, _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [1.5 + 0.9e-6 * diag, 0, 0]}]), floor],
        "across a plane": [glass, _obj("plane", [{"translate": [0, 0.3, 0]}]), floor],
        "another root with ior 1.0000001": [glass, _sphere_at(4.0, 1.0, {"diffuse": 0.7, "refractive-index": 1.0000001}), floor],
        "an opaque cube with ior 2.0": [glass, _obj("cube", [{"translate": [5, 0, 4]}], {"diffuse": 0.6, "refractive-index": 2.0}), floor],
    }
    for what, objs in cases.items():
        assert marked(objs)[0] is False, what
    # a glass cube: alone up to a half-extent of 1e3, not above it
    far_floor = _obj("plane", [{"translate": [0, -2000, 0]}])
    assert marked([_obj("cube", [{"scale": [900, 2, 2]}], _glass()), far_floor])[0] is True
    assert marked([_obj("cube", [{"scale": [1000.5, 2, 2]}], _glass()), far_floor])[0] is False, "a half-extent above 1e3"
    # a cube needs 0.05 x its largest half-extent towards a plane
    assert marked([_obj("cube", [{"scale": [10, 1, 1]}], _glass()), _obj("plane", [{"translate": [0, -1.51, 0]}])])[0] is True
    assert marked([_obj("cube", [{"scale": [10, 1, 1]}], _glass()), _obj("plane", [{"translate": [0, -1.49, 0]}])])[0] is False


# ---- the reduction ---------------------------------------------------------------------------------------------------------

def _entries(desc, o, d):
    """per World.objects entry: (leaf index, ior, [t of every entry, NaN where there is none]) for every ray"""
    out = []
    for i in range(desc.n_roots):
        leaf = desc.roots[i]
        kind = desc.leaf_kind[leaf]
        oo, dd = _object_rays(desc, leaf, o, d)
        with np.errstate(all="ignore"):
            if kind == 1:   # plane.zig:25-36
                has = np.abs(dd[:, 1]) > 1e-5
                ts = [np.where(has, -oo[:, 1] / np.where(has, dd[:, 1], 1.0), np.nan)]
            else:
                has, t1, t2 = _reference_entries(kind, oo, dd)
                ts = [np.where(has, t1, np.nan), np.where(has, t2, np.nan)]
        out.append((leaf, _ior(desc, leaf), ts))
    return out


def _n1_n2(entries, hit, t_hit, use):
    """The containers walk of PreComputations.new (world.zig:229-255) as the kernels' visitor states it, over the roots `use`:
    a leaf is open if an odd number of its entries lies at t < 0; n1 is the ior of the open leaf whose last negative entry is
    latest (ties: the larger leaf index), else 1; n2 is the hit leaf's ior if the hit leaf is not open, else the ior of the
    latest open leaf other than the hit leaf, else the hit leaf's again if two of its entries lie at t_hit, else 1."""
    n = len(t_hit)
    best_t, best_leaf, n1 = np.full(n, -INF), np.full(n, -1), np.ones(n)
    excl_t, excl_leaf, n2_excl = np.full(n, -INF), np.full(n, -1), np.ones(n)
    hit_leaf, hit_ior = entries[hit][0], entries[hit][1]
    hit_open, dups = np.zeros(n, bool), np.zeros(n, int)
    for r in use:
        leaf, ior, ts = entries[r]
        with np.errstate(invalid="ignore"):
            neg = [t < 0.0 for t in ts]
            count = sum(x.astype(int) for x in neg)
            last = np.full(n, -INF)
            for t, x in zip(ts, neg):
                last = np.where(x, np.fmax(last, t), last)
            if r == hit:
                dups = sum(((t == t_hit) & ~x).astype(int) for t, x in zip(ts, neg))
        is_open = count % 2 == 1
        later = is_open & ((last > best_t) | ((last == best_t) & ((best_leaf < 0) | (leaf > best_leaf))))
        best_t, best_leaf, n1 = np.where(later, last, best_t), np.where(later, leaf, best_leaf), np.where(later, ior, n1)
        if r == hit:
            hit_open = is_open
        else:
            later = is_open & ((last > excl_t) | ((last == excl_t) & ((excl_leaf < 0) | (leaf > excl_leaf))))
            excl_t, excl_leaf, n2_excl = np.where(later, last, excl_t), np.where(later, leaf, excl_leaf), np.where(later, ior, n2_excl)
    n2 = np.where(~hit_open, hit_ior, np.where(excl_leaf >= 0, n2_excl, np.where(dups >= 2, hit_ior, 1.0)))
    assert hit_leaf == entries[hit][0]
    return n1, n2, hit_open


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _reduction_world(rtc, rng, kind, stretch):
    """A simple world with one alone H at World.objects index 0 - a sphere, or a cube rotated, sheared and stretched to
    `stretch` - between neighbours of ior 1.0 whose boxes lie just beyond the margin and planes just beyond H's margin."""
    if kind == "sphere":
        h_xf = [{"scale": [float(s) for s in rng.uniform(0.5, 3.0, size=3)]}, {"rotate-x": float(rng.uniform(0, 3))}, {"rotate-z": float(rng.uniform(0, 3))},
                {"translate": [float(v) for v in rng.uniform(-2, 2, size=3)]}]
    else:
        h_xf = [{"scale": [float(stretch), float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))]},
                {"shear": {"xy": float(rng.uniform(-0.4, 0.4)), "xz": 0.0, "yx": float(rng.uniform(-0.4, 0.4)), "yz": 0.0, "zx": 0.0, "zy": float(rng.uniform(-0.4, 0.4))}},
                {"rotate-y": float(rng.uniform(0, 3))}, {"rotate-z": float(rng.uniform(0, 3))}, {"translate": [float(v) for v in rng.uniform(-2, 2, size=3)]}]
    h = _obj(kind, h_xf, _glass(1.5))
    probe = rtc.HostScene(_scene([h])).desc
    fwd, _ = _forward(probe, probe.roots[0])
    lo, hi = _world_box(fwd)
    diag = float(np.linalg.norm(hi - lo))
    s_max = float(np.linalg.norm(fwd[:3, :3], axis=0).max())
    margin = 1e-6 * diag if kind == "sphere" else 0.05 * s_max
    objs = [h]
    # neighbours of ior 1.0 (one of them transparent, one a mirror) whose boxes clear H's by 1.5 x the margin between boxes
    size = 0.25 * diag
    gap = 1.5e-6 * max(diag, 2.0 * np.sqrt(3.0) * size)
    mid = 0.5 * (lo + hi)
    for axis, side, material in ((0, 1, {"diffuse": 0.7}), (1, -1, {"transparency": 0.5, "refractive-index": 1.0, "diffuse": 0.3}), (2, 1, {"reflective": 0.8, "diffuse": 0.1})):
        c = mid.copy()
        c[axis] = (hi[axis] + gap + size) if side > 0 else (lo[axis] - gap - size)
        objs.append(_obj("cube" if axis != 1 else "sphere", [{"scale": [size, size, size]}, {"translate": [float(v) for v in c]}], material))
    # planes of ior 1.0 just beyond H's margin: axis-aligned below, and two tilted ones - their normals from the library's own
    # rotation (a plane rotated about the origin has its normal in row 1 of its inverse), then moved along the normal
    for angles in ({}, {"rotate-z": 0.7}, {"rotate-x": -0.9, "rotate-z": 2.0}):
        rot = [{k: v} for k, v in angles.items()]
        p = rtc.HostScene(_scene([_obj("plane", rot if rot else [{"translate": [0, 0, 0]}])])).desc
        normal = _forward(p, p.roots[0])[1][1][:3]
        corners = np.array([[x, y, z] for x in (lo[0] - margin, hi[0] + margin) for y in (lo[1] - margin, hi[1] + margin) for z in (lo[2] - margin, hi[2] + margin)])
        offset = float((corners @ normal).min()) * (1.0 + 1e-9) - 1e-9 * (1.0 + abs(float((corners @ normal).min())))   # every corner above it
        objs.append(_obj("plane", rot + [{"translate": [float(v) for v in normal * offset]}], {"diffuse": 0.8, "reflective": 0.3}))
    hs = rtc.HostScene(_scene(objs))
    return hs, fwd, (lo, hi), margin


def _reduction_rays(rng, desc, fwd, box, n):
    """Origins inside H, on the neighbours' and H's surfaces offset by +-1e-5, and far outside; directions random, aimed at H,
    and with one or two components below 1e-5 in H's space."""
    lo, hi = box
    o = np.empty((n, 3))
    third = n // 3
    inside = rng.uniform(-0.999, 0.999, size=(third, 3))
    if desc.leaf_kind[desc.roots[0]] == 0:
        inside *= (rng.random(third) ** (1 / 3) / np.maximum(np.linalg.norm(inside, axis=1), 1e-9))[:, None] * 0.999
    o[:third] = (np.c_[inside, np.ones(third)] @ fwd.T)[:, :3]
    # on a surface: a neighbour's (object-space point of a face or of the unit sphere) or H's own, offset by +-1e-5 along a random direction
    for k in range(third, 2 * third):
        r = int(rng.integers(0, 4))
        leaf = desc.roots[r]
        f, _ = _forward(desc, leaf)
        p = rng.uniform(-1, 1, size=3)
        if desc.leaf_kind[leaf] == 0:
            p /= np.linalg.norm(p)
        else:
            p[rng.integers(0, 3)] = rng.choice([-1.0, 1.0])
        w = (f @ np.r_[p, 1.0])[:3]
        nudge = rng.normal(size=3)
        o[k] = w + rng.choice([-1e-5, 1e-5]) * nudge / np.linalg.norm(nudge)
    far = rng.normal(size=(n - 2 * third, 3))
    o[2 * third:] = 0.5 * (lo + hi) + far / np.linalg.norm(far, axis=1, keepdims=True) * np.linalg.norm(hi - lo) * rng.uniform(0.8, 6.0, size=(n - 2 * third, 1))
    d = rng.normal(size=(n, 3))
    aim = rng.random(n) < 0.6   # towards a point of H
    target = (np.c_[rng.uniform(-0.9, 0.9, size=(n, 3)), np.ones(n)] @ fwd.T)[:, :3]
    d[aim] = (target - o)[aim]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # components below 1e-5 in H's space: the direction formed in object space, one or two axes tiny, and brought back
    tiny = rng.random(n) < 0.4
    inv3 = np.linalg.inv(fwd[:3, :3])
    dobj = d @ inv3.T
    for k in np.flatnonzero(tiny):
        axes = rng.choice(3, size=int(rng.integers(1, 3)), replace=False)
        dobj[k, axes] = 0.0
        length = np.linalg.norm(fwd[:3, :3] @ dobj[k])   # (the world direction is normalised below: the tiny components are what they are AFTER that)
        dobj[k, axes] = rng.choice([0.0, 1e-12, 1e-7, 3e-6, 9.9e-6], size=len(axes)) * rng.choice([-1.0, 1.0], size=len(axes)) * length
    d[tiny] = dobj[tiny] @ fwd[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


@pytest.mark.parametrize("kind,stretch", [("sphere", 1.0), ("cube", 1.5), ("cube", 50.0), ("cube", 900.0)])
def test_n1_n2_of_all_roots_are_those_of_the_hit_root_alone(rtc, kind, stretch):
    rng = np.random.default_rng(20261020 + int(stretch))
    for world in range(3):
        hs, fwd, box, margin = _reduction_world(rtc, rng, kind, stretch)
        desc = hs.desc
        assert _alone(rtc, desc)[0] is True, (kind, stretch, world)
        assert all(_ior(desc, desc.roots[i]) == 1.0 for i in range(1, desc.n_roots))
        o, d = _reduction_rays(rng, desc, fwd, box, 60000)
        entries = _entries(desc, o, d)
        with np.errstate(invalid="ignore"):
            first = [np.fmin.reduce([np.where(t >= 0.0, t, INF) for t in ts]) for _, _, ts in entries]   # the first entry at t >= 0 of every root
        t_hit = first[0]
        hits_h = np.isfinite(t_hit) & np.all([first[r] > t_hit for r in range(1, desc.n_roots)], axis=0)
        n1_all, n2_all, is_open = _n1_n2(entries, 0, t_hit, range(desc.n_roots))
        n1_own, n2_own, open_own = _n1_n2(entries, 0, t_hit, [0])
        n_open, n_closed = int((hits_h & is_open).sum()), int((hits_h & ~is_open).sum())
        print(f"{kind} stretched to {stretch}, world {world}: {n_open} rays with H open, {n_closed} with H not open, margin {margin:.3g}")
        assert n_open >= 1000 and n_closed >= 1000, (kind, stretch, world, n_open, n_closed)
        bad = np.flatnonzero(hits_h & ((n1_all != n1_own) | (n2_all != n2_own) | (is_open != open_own)))
        assert len(bad) == 0, (kind, stretch, world, len(bad), o[bad[0]].tolist(), d[bad[0]].tolist(), float(n1_all[bad[0]]), float(n2_all[bad[0]]),
                               float(n1_own[bad[0]]), float(n2_own[bad[0]]))
        # with H open the pair is (H's ior, 1); with H not open it is (1, H's ior)
        assert np.all(n1_own[hits_h & is_open] == 1.5) and np.all(n2_own[hits_h & is_open] == 1.0)
        assert np.all(n1_own[hits_h & ~is_open] == 1.0) and np.all(n2_own[hits_h & ~is_open] == 1.5)
