"""The containers pass (n1 / n2 of a refracted ray) uses a root only if an ODD number of its entries lies behind the origin.  In
a world of planes, spheres and cubes (the simple kernels; csrc/rtc_kernels.hip, trace(), RTC_CONTAINERS_SOLIDS; DESIGN.md
section 5) its phase 1 drops a bounded root whose bound lies entirely behind the origin, which is right only if such a root's
count is even.  Here - on the CPU, no GPU - phase 1 is replayed in float32 on the tables rtc_scene_create builds, world boxes
(rtc_diag_root_boxes, the replay of tests/test_root_boxes_cpu.py) and bounding spheres (rtc_diag_root_spheres, `roots_kept`
restated below), against the float64 restatement of Sphere / Cube.localIntersect, for rays that start inside, on and within
1e-5 of the solids - where a count is odd, or only just is not -, cubes stretched until the "parallel" rule applies included.

  (a) every root with an odd count of negative entries is kept by the closest visitor's limits, box and sphere tables (the
      closest-hit trace of the same ray tests every root the pass can use: what a record of such roots would rest on);
  (b) every bounded root the tightened containers limits reject has an even count.

The pass's plane test makes no division where o.y and d.y differ in sign: restated in float64 and held against the quotient."""
import json

import numpy as np

from test_root_boxes_cpu import F, INF, _kernel_keeps, _object_rays, _rays, _reference_entries

RAYS_PER_SCENE = 260000

CLOSEST = (-1.0002e-4, INF)          # ClosestVisitor::box_limits with t = inf
BEHIND_BEFORE = (-INF, 1.0002e-4)    # BehindVisitor::box_limits
BEHIND = (-1.0002e-4, 1.0002e-4)     # ... as trace() tightens it in a simple world


def _sphere_keeps(sphere, cmax, o, d, front_only, behind_only, solids):
    """ray_f32 + roots_kept of csrc/rtc_kernels.hip for one root of a world without groups, in float32 (an FMA: the product and
    the sum in float64, rounded once)."""
    o32, d32 = o.astype(F), d.astype(F)
    c, r2 = sphere[0:3].astype(F), F(sphere[3])
    f64 = np.float64
    with np.errstate(all="ignore"):
        a = ((d32[:, 0] * d32[:, 0] + d32[:, 1] * d32[:, 1]).astype(F) + d32[:, 2] * d32[:, 2]).astype(F)
        s = (np.sqrt(((o32[:, 0] * o32[:, 0] + o32[:, 1] * o32[:, 1]).astype(F) + o32[:, 2] * o32[:, 2]).astype(F)).astype(F) + F(cmax)).astype(F)
        s2 = (s * s).astype(F)
        t_scale = (F(8e-6) * a).astype(F)
        oc = (c[None, :] - o32).astype(F)
        fma = lambda x, y, z: (x.astype(f64) * y.astype(f64) + z.astype(f64)).astype(F)
        b = fma(oc[:, 0], d32[:, 0], fma(oc[:, 1], d32[:, 1], (oc[:, 2] * d32[:, 2]).astype(F)))
        oc2 = fma(oc[:, 0], oc[:, 0], fma(oc[:, 1], oc[:, 1], (oc[:, 2] * oc[:, 2]).astype(F)))
        T = ((oc2 + s2).astype(F) * t_scale).astype(F)
        ac = ((oc2 - r2).astype(F) * a).astype(F)
        bb = (b * b).astype(F)
        disc = (bb - ac).astype(F)
        miss = disc < -T
        sided = (ac > T) & (bb > T)
        behind, front = sided & (b < 0), sided & (b > 0)
        culled = miss | (behind & (front_only or solids)) | (front & behind_only)
    return ~culled


def _solid(kind, transform):
    return {"type": {kind: {}}, "transform": transform, "material": {"transparency": 0.7, "refractive-index": 1.4}}


def _scene(objs):
    return json.dumps({"camera": {"width": 8, "height": 8, "field-of-view": 1.0, "from": [0, 2, -9], "to": [0, 1, 0], "up": [0, 1, 0]},
                       "lights": [{"point-light": {"position": [-4, 8, -5], "intensity": [1, 1, 1]}}],
                       "objects": objs + [{"type": {"plane": {}}, "transform": [{"translate": [0, -2, 0]}]}]})


def _nested_solids():
    return _scene([
        _solid("sphere", []), _solid("sphere", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [0.3, 0.2, -0.1]}]),
        _solid("sphere", [{"scale": [3, 0.3, 1]}, {"rotate-z": 0.4}, {"translate": [2, 1, 0]}]),
        _solid("sphere", [{"scale": [8, 8, 8]}]), _solid("sphere", [{"scale": [0.05, 0.05, 0.05]}, {"translate": [-3, 0.5, 2]}]),
        _solid("cube", [{"translate": [0.5, 0, 0.5]}]), _solid("cube", [{"scale": [1.5, 1.5, 1.5]}]),
        _solid("cube", [{"rotate-y": 0.6}, {"shear": {"xy": 0.4, "zy": -0.3}}, {"rotate-z": 0.2}, {"translate": [-3.5, 1.3, 1]}]),
        _solid("cube", [{"scale": [0.3, 1.7, 0.9]}, {"rotate-y": -0.4}, {"translate": [4.6, 1.7, 2]}]),
        _solid("cube", [{"translate": [2.5, 0, 0.5]}]),           # shares the face x = 1.5 with the first cube
    ])


def _stretched_cubes(stretch):
    """cubes so long that an ordinary ray's direction has a component below 1e-5 in their object space (cube.zig:28-35)"""
    return _scene([
        _solid("cube", [{"scale": [stretch, 0.02, 1]}, {"translate": [0, 0.5, 0]}]),
        _solid("cube", [{"scale": [0.3, stretch, 0.3]}, {"rotate-z": 0.3}, {"translate": [1, 0, 2]}]),
        _solid("cube", [{"scale": [1, 1, stretch]}, {"rotate-y": 0.7}, {"translate": [-2, 1, 0]}]),
        _solid("sphere", [{"scale": [stretch, 0.5, 0.5]}, {"translate": [0, 2, 1]}]),
        _solid("sphere", [{"translate": [0.2, 0.4, 0.1]}]),
    ])


def _scenes(rtc):
    for name in ("cover.json", "cubes.json", "reflection_and_refraction.json", "fresnel.json"):
        yield name, rtc.HostScene.from_file(name)
    yield "nested solids", rtc.HostScene(_nested_solids())
    yield "stretched cubes 50", rtc.HostScene(_stretched_cubes(50.0))
    yield "stretched cubes 1000", rtc.HostScene(_stretched_cubes(1000.0))
    yield "stretched cubes 1e5", rtc.HostScene(_stretched_cubes(1.0e5))


def _solids(desc, order):
    """[(table position, leaf, kind)] of the top-level spheres and cubes"""
    out = []
    for pos in range(desc.n_roots):
        root = desc.roots[int(order[pos])]
        if not (root & 0x80000000) and desc.leaf_kind[root] in (0, 2):
            out.append((pos, root, int(desc.leaf_kind[root])))
    return out


def _rays_about_the_solids(rng, desc, solids, boxes, n):
    """A quarter: the random and box-aimed rays of tests/test_root_boxes_cpu.py.  The rest start in a solid's object space -
    inside it, on its surface, within 1e-5 either side of the surface - and go anywhere, along the surface, or nearly parallel
    to an axis of the solid."""
    o, d = _rays(rng, desc, boxes, n)
    k = n - n // 4
    which = rng.integers(0, len(solids), size=k)
    p = rng.uniform(-1.0, 1.0, size=(k, 3))
    dl = rng.normal(size=(k, 3))
    place = rng.integers(0, 3, size=k)          # 0 inside, 1 on the surface, 2 within 1e-5 of it
    off = np.where(place == 2, rng.choice([1e-5, -1e-5, 3e-6, -3e-6, 1e-7, -1e-7, 1e-9, -1e-9, 1e-12, -1e-12], size=k), 0.0)
    for i, (_, leaf, kind) in enumerate(solids):
        m = which == i
        if not m.any():
            continue
        q = p[m]
        if kind == 0:
            r = np.linalg.norm(q, axis=1, keepdims=True)
            unit = q / np.where(r > 0, r, 1.0)
            q = np.where((place[m] == 0)[:, None], unit * rng.uniform(0.0, 1.0, size=(int(m.sum()), 1)), unit * (1.0 + off[m])[:, None])
        else:
            axis = rng.integers(0, 3, size=int(m.sum()))
            face = rng.choice([-1.0, 1.0], size=int(m.sum())) * (1.0 + off[m])
            on = place[m] != 0
            q[on, axis[on]] = face[on]
            edge = on & (rng.random(int(m.sum())) < 0.2)                 # a fifth of those on an edge as well
            q[edge, (axis[edge] + 1) % 3] = rng.choice([-1.0, 1.0], size=int(edge.sum()))
        dq = dl[m]
        tiny = rng.random(int(m.sum())) < 0.4                            # along the surface / nearly parallel to an axis
        comp = rng.integers(0, 3, size=int(m.sum()))
        dq[tiny, comp[tiny]] = (rng.choice([0.0, 1e-12, 1e-7, 3e-6, 9.9e-6, 1.1e-5, 1e-4], size=int(tiny.sum())) *
                                rng.choice([-1.0, 1.0], size=int(tiny.sum())))
        inv = np.ctypeslib.as_array(desc.xf_inv, shape=(desc.n_xforms * 16,))[16 * desc.leaf_xform[leaf]:16 * desc.leaf_xform[leaf] + 16]
        fwd = np.linalg.inv(np.array(inv, dtype=np.float64).reshape(4, 4))
        o[n // 4:][m] = q @ fwd[:3, :3].T + fwd[:3, 3]
        dw = dq @ fwd[:3, :3].T
        d[n // 4:][m] = dw / np.linalg.norm(dw, axis=1, keepdims=True)
    return o, d


def test_open_roots_are_tested_by_the_closest_hit_trace_and_kept_by_the_tightened_pass(rtc):
    rng = np.random.default_rng(20261018)
    rays = odd_pairs = dropped_even = 0
    for name, hs in _scenes(rtc):
        desc = hs.desc
        boxes, order, scales = rtc.root_boxes(desc)
        spheres, cmax = rtc.root_spheres(desc)
        solids = _solids(desc, order)
        assert solids, name
        o, d = _rays_about_the_solids(rng, desc, solids, boxes, RAYS_PER_SCENE)
        rays += len(o)
        for pos, leaf, kind in solids:
            has, t1, t2 = _reference_entries(kind, *_object_rays(desc, leaf, o, d))
            with np.errstate(invalid="ignore"):
                odd = has & ((t1 < 0) != (t2 < 0))
            tables = {
                "closest, boxes": _kernel_keeps(boxes[pos], scales, o, d, *CLOSEST),
                "closest, spheres": _sphere_keeps(spheres[pos], cmax, o, d, True, False, False),
                "containers, boxes": _kernel_keeps(boxes[pos], scales, o, d, *BEHIND),
                "containers, spheres": _sphere_keeps(spheres[pos], cmax, o, d, False, True, True),
            }
            for what, keeps in tables.items():   # (a): odd => the closest limits keep; (b): the containers limits reject => even
                bad = np.flatnonzero(odd & ~keeps)
                assert len(bad) == 0, (name, "table position", pos, what, "ray", o[bad[0]].tolist(), d[bad[0]].tolist(),
                                       "entries", float(t1[bad[0]]), float(t2[bad[0]]))
            odd_pairs += int(odd.sum())
            before = _kernel_keeps(boxes[pos], scales, o, d, *BEHIND_BEFORE) & _sphere_keeps(spheres[pos], cmax, o, d, False, True, False)
            dropped_even += int((before & ~tables["containers, boxes"] & ~tables["containers, spheres"]).sum())
    print(f"{rays} rays, {odd_pairs} (ray, root) pairs with an odd count, {dropped_even} pairs only the tightened limits drop")
    assert rays >= 2000000 and odd_pairs > 1000000 and dropped_even > 100000   # (the test did look at something)


def test_a_plane_without_a_division_has_no_negative_entry():
    """leaf_of_kind's plane branch of the containers pass in a simple world (|d.y| > 1e-5 given): the division is made only where
    `o.y > 0` equals `d.y > 0`.  Everywhere else the quotient -o.y / d.y must not be < 0 - zeros of either sign, NaNs and
    infinities included."""
    rng = np.random.default_rng(5)
    n = 400000
    mag = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, size=n) * rng.choice([-1.0, 1.0], size=n)
    oy = np.where(rng.random(n) < 0.5, mag(-6, 3), mag(-320, 300))
    oy[rng.random(n) < 0.05] = 0.0
    oy[rng.random(n) < 0.02] = -0.0
    oy[rng.random(n) < 0.01] = np.nan
    oy[rng.random(n) < 0.01] = np.inf
    oy[rng.random(n) < 0.01] = -np.inf
    dy = np.where(rng.random(n) < 0.7, mag(-5, 0), mag(-5, 300))
    dy[rng.random(n) < 0.01] = np.inf
    dy[rng.random(n) < 0.01] = -np.inf
    assert (np.abs(dy) > 1e-5).all()
    with np.errstate(all="ignore"):
        divides = (oy > 0.0) == (dy > 0.0)
        q = -oy / dy
        negative = q < 0.0
    assert not (negative & ~divides).any(), (oy[negative & ~divides][:3], dy[negative & ~divides][:3])
    assert (~divides).sum() > 100000 and (negative & divides).sum() > 100000 and (~negative & divides).sum() > 1000
