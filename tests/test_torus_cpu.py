"""Torus primitives without a GPU (RTC_TORUS): the checker's solver by hand, against mpmath at 60
digits and against a pure-Python restatement of rtc.h's steps bit for bit; the checker against the bump checker it stacks
on; the loader, the flattened tables and rtc_scene_create's refusals; the product's conservative bounds against the
checker's entries; the disassembly-identity record.

Solver accuracy, measured with the checker on the 3000-ray family below: 2066 rays hit, root counts equal on all 3000, no
ray left out, worst |t - t_exact| / max(1, |t_exact|) = 1.832e-15 - the bound of the test is 16 times that, 2.9e-14."""
import ctypes as C
import hashlib
import json
import math
import os
import random

import numpy as np
import pytest

import bump_binding as bb
import torus_binding as tb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(REPO, "tests", "golden", "scenes")
TORUS = 7
# worst relative error of the checker on the family, times 16 (four bits of slack for a sample), and below 1e-9 in any case
WORST_MEASURED = 1.84e-15
ACCURACY_BOUND = 16 * WORST_MEASURED
assert ACCURACY_BOUND < 1e-9


# ---- hand-derivable KATs, R = 2, r = 0.5
def test_roots_by_hand():
    assert np.array_equal(tb.roots([-5, 0, 0], [1, 0, 0], 2, 0.5), [2.5, 3.5, 6.5, 7.5])
    assert len(tb.roots([0, 5, 0], [0, -1, 0], 2, 0.5)) == 0            # through the hole
    assert np.array_equal(tb.roots([2, 5, 0], [0, -1, 0], 2, 0.5), [4.5, 5.5])
    assert len(tb.roots([0, 0.5 + 1e-3, -5], [0, 0, 1], 2, 0.5)) == 0   # above the tube
    t = tb.roots([0, 0.25, -5], [0, 0, 1], 2, 0.5)
    assert len(t) == 4 and np.all(np.diff(t) > 0)
    assert np.allclose(t + t[::-1], 10.0, rtol=0, atol=1e-14)           # symmetric about t = 5
    h = math.sqrt(0.5 ** 2 - 0.25 ** 2)
    assert np.allclose(t, [5 - 2 - h, 5 - 2 + h, 5 + 2 - h, 5 + 2 + h], rtol=0, atol=1e-14)


def test_normals_by_hand():
    assert np.array_equal(tb.normal([2.5, 0, 0], 2), [0.5, 0, 0])
    assert np.array_equal(tb.normal([2, 0.5, 0], 2), [0, 0.5, 0])
    assert np.array_equal(tb.normal([1.5, 0, 0], 2), [-0.5, 0, 0])
    assert np.array_equal(tb.normal([0, 0.3, 0], 2), [0, 0.3, 0])     # rho == 0: no NaN


def test_coefficients_by_hand():
    # from (-5, 0, 0) along +x: t0 = 5, p = 0: q(s) = s^4 + 2 (R^2 - r^2 - 2 R^2) s^2 + (R^2 - r^2)^2
    k = tb.coefficients([-5, 0, 0], [1, 0, 0], 2, 0.5)
    assert np.array_equal(k, [5.0, 1.0, 0.0, 2 * 3.75 - 16.0, 0.0, 3.75 * 3.75])


def test_a_scaled_direction_gives_scaled_parameters():
    t1 = tb.roots([-5, 0.1, 0.2], [1, 0, 0], 2, 0.5)
    t2 = tb.roots([-5, 0.1, 0.2], [4, 0, 0], 2, 0.5)
    assert len(t1) == len(t2) == 4 and np.allclose(t1, 4 * t2, rtol=1e-15, atol=0)


# ---- the seeded ray family (the issue's: R in [0.5, 3], r / R in [0.05, 0.95], origins at 3, 10, 100 and 1000 R, aimed
# into a box 5 % larger than the torus's)
def _family(n=3000, seed=1):
    random.seed(seed)
    rays = []
    for _ in range(n):
        R = random.uniform(0.5, 3)
        r = random.uniform(0.05, 0.95) * R
        dist = random.choice([3, 10, 100, 1000])
        o = [random.gauss(0, 1) for _ in range(3)]
        m = math.sqrt(sum(x * x for x in o))
        o = [x / m * dist * R for x in o]
        tgt = [random.uniform(-1, 1) * (R + r) * 1.05, random.uniform(-1, 1) * r * 1.2, random.uniform(-1, 1) * (R + r) * 1.05]
        d = [t - x for t, x in zip(tgt, o)]
        m = math.sqrt(sum(x * x for x in d))
        rays.append((o, [x / m for x in d], R, r))
    return rays


def _checker_roots(rays):
    n, t = tb.roots_many([q[0] for q in rays], [q[1] for q in rays], [q[2] for q in rays], [q[3] for q in rays])
    return [list(t[i, :n[i]]) for i in range(len(rays))]


def test_solver_against_mpmath_at_60_digits():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    rays = _family()
    got = _checker_roots(rays)
    worst, left_out, hits = 0.0, 0, 0
    for (o, d, R, r), g in zip(rays, got):
        o = [mp.mpf(x) for x in o]
        d = [mp.mpf(x) for x in d]
        R, r = mp.mpf(R), mp.mpf(r)
        al = sum(x * x for x in d)
        be = 2 * sum(a * b for a, b in zip(o, d))
        ga = sum(x * x for x in o) + R * R - r * r
        f4 = 4 * R * R
        c = [al * al, 2 * al * be, be * be + 2 * al * ga - f4 * (d[0] ** 2 + d[2] ** 2), 2 * be * ga - 2 * f4 * (o[0] * d[0] + o[2] * d[2]),
             ga * ga - f4 * (o[0] ** 2 + o[2] ** 2)]
        rs = mp.polyroots(c, maxsteps=200, extraprec=200)
        if any(abs(rs[a] - rs[b]) < 1e-4 * R for a in range(4) for b in range(a)):   # a tangent ray
            left_out += 1
            continue
        exact = sorted(mp.re(z) for z in rs if abs(mp.im(z)) < mp.mpf(10) ** -40)
        assert len(g) == len(exact), (o, d, R, r, g, exact)
        hits += bool(g)
        for a, e in zip(g, exact):
            worst = max(worst, float(abs(mp.mpf(a) - e)) / max(1.0, abs(float(e))))
    print(f"{len(rays)} rays, {hits} hit, {left_out} left out, worst relative error {worst:.3e} (bound {ACCURACY_BOUND:.3e})")
    assert left_out <= len(rays) // 100
    assert hits > len(rays) // 2
    assert worst <= ACCURACY_BOUND


# ---- rtc.h's steps 1 to 5 in plain Python floats: the stated operation order is the implemented one
INF = float("inf")


def _check_axis(origin, direction, mn, mx):
    a, b = mn - origin, mx - origin
    if abs(direction) >= 1e-5:
        lo, hi = a / direction, b / direction
    else:
        with np.errstate(invalid="ignore"):
            lo, hi = float(np.float64(a) * INF), float(np.float64(b) * INF)
    if lo > hi:
        lo, hi = hi, lo
    return lo, hi


def _fmax(a, b):
    return b if (a != a or b > a) else a


def _fmin(a, b):
    return b if (a != a or b < a) else a


def _restated(o, d, R, r):
    alpha = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    t0 = -((o[0] * d[0] + o[1] * d[1]) + o[2] * d[2]) / alpha
    bxz, by = (R + r) * (1.0 + 1e-9), r * (1.0 + 1e-9)
    ax = [_check_axis(o[k], d[k], -e, e) for k, e in enumerate((bxz, by, bxz))]
    tmin = _fmax(ax[0][0], _fmax(ax[1][0], ax[2][0]))
    tmax = _fmin(ax[0][1], _fmin(ax[1][1], ax[2][1]))
    if tmin > tmax:
        return []
    lo, hi = tmin - t0, tmax - t0
    if not (lo < hi) or not (hi - lo < INF):
        return []
    px, py, pz = o[0] + t0 * d[0], o[1] + t0 * d[1], o[2] + t0 * d[2]
    beta = 2.0 * ((px * d[0] + py * d[1]) + pz * d[2])
    gamma = (((px * px + py * py) + pz * pz) + R * R) - r * r
    f = 4.0 * (R * R)
    c4 = alpha * alpha
    c3 = (2.0 * alpha) * beta
    c2 = (beta * beta + (2.0 * alpha) * gamma) - f * (d[0] * d[0] + d[2] * d[2])
    c1 = (2.0 * beta) * gamma - (2.0 * f) * (px * d[0] + pz * d[2])
    c0 = gamma * gamma - f * (px * px + pz * pz)

    def scan(a4, a3, a2, a1, a0, points, cap):
        b3, b2, b1, b0 = 4.0 * a4, 3.0 * a3, 2.0 * a2, a1
        P = lambda x: (((a4 * x + a3) * x + a2) * x + a1) * x + a0
        D = lambda x: ((b3 * x + b2) * x + b1) * x + b0
        out = []

        def emit(x):
            if len(out) >= cap or (out and not (x > out[-1])):
                return
            out.append(x)

        def refine(l, h, fa):
            x = 0.5 * (l + h)
            for _ in range(80):
                fx = P(x)
                if fx == 0.0:
                    break
                if (fx < 0.0) == (fa < 0.0):
                    l = x
                else:
                    h = x
                dv = D(x)
                xn = x - fx / dv if dv != 0.0 else l
                if not (xn > l and xn < h):
                    xn = 0.5 * (l + h)
                m = 0.5 * (l + h)
                stop = xn == x or not (l < h) or m == l or m == h
                x = xn
                if stop:
                    break
            return x

        a, fa = lo, P(lo)
        for i, b in enumerate(list(points) + [hi]):
            if i < len(points) and not (b > a and b < hi):
                continue
            fb = P(b)
            if fa == 0.0:
                emit(a)
            elif (fa < 0.0) != (fb < 0.0) and fb != 0.0:
                emit(refine(a, b, fa))
            a, fa = b, fb
        if fa == 0.0:
            emit(a)
        return out

    a3, a2, a1, a0 = 4.0 * c4, 3.0 * c3, 2.0 * c2, c1
    q0, q1, q2 = 3.0 * a3, 2.0 * a2, a1
    disc = q1 * q1 - (4.0 * q0) * q2
    crit = []
    if disc >= 0.0:
        sq = math.sqrt(disc)
        k0, k1 = (-q1 - sq) / (2.0 * q0), (-q1 + sq) / (2.0 * q0)
        crit = [k1, k0] if k1 < k0 else [k0, k1]
    turning = scan(0.0, a3, a2, a1, a0, crit, 3)
    return [t0 + s for s in scan(c4, c3, c2, c1, c0, turning, 4)]


def test_restatement_equals_the_checker_bit_for_bit():
    rays = _family()
    # (and rays that start inside the box, run along an axis, or miss)
    rays += [([0.3, 0.1, -0.2], [0.0, 1.0, 0.0], 1.0, 0.25), ([1.0, 0.0, 0.0], [0.0, 0.0, 1.0], 1.0, 0.25),
             ([1.0, 0.0, 0.0], [1e-6, 0.0, 1.0], 1.0, 0.25), ([9.0, 9.0, 9.0], [1.0, 0.0, 0.0], 1.0, 0.25),
             ([-5.0, 0.0, 0.0], [1.0, 0.0, 0.0], 2.0, 0.5), ([-5.0, 0.5, 0.0], [1.0, 0.0, 0.0], 2.0, 0.5)]
    got = _checker_roots(rays)
    hits = 0
    for q, g in zip(rays, got):
        want = _restated(*q)
        assert len(g) == len(want), (q, g, want)
        assert all(a == b for a, b in zip(g, want)), (q, g, want)
        hits += bool(g)
    assert hits > 1500


# ---- the checker against the bump checker it stacks on
@pytest.mark.parametrize("which", ["bump_mix", "spot_mix"])
def test_no_torus_is_the_bump_checker_bit_for_bit(rtc, which):
    hs = bb.mix(rtc) if which == "bump_mix" else rtc.HostScene.from_file(bb.SPOT_MIX)
    assert not tb.tori_of(hs.desc)
    cam = hs.camera(48, 27)
    want, wc = bb.BumpScene(hs.desc, hs.lights, hs.bumps()).render(cam, 5, spots=hs.spots(), light_seed=3)
    ck = tb.TorusScene(hs.desc, hs.lights, hs.bumps())
    got, gc = ck.render(cam, 5, spots=hs.spots(), light_seed=3)
    assert np.array_equal(got, want) and gc == wc
    own, oc = ck.render_bump(cam, 5, spots=hs.spots(), light_seed=3)
    assert np.array_equal(own, want) and oc == wc


def test_tori_change_the_image_of_their_placeholders(rtc):
    hs = tb.mix(rtc)
    cam = hs.camera(48, 27)
    ck = tb.TorusScene(hs.desc, hs.lights, hs.bumps())
    tori, tc = ck.render(cam, 5, spots=hs.spots())
    spheres, sc = ck.render_bump(cam, 5, spots=hs.spots())
    assert tc["primary"] == sc["primary"] == 48 * 27
    assert (np.abs(tori - spheres).max(axis=2) > 1e-3).mean() > 0.1


def test_a_glass_torus_is_crossed_through_four_surfaces(rtc):
    hs = tb.mix(rtc)
    ck = tb.TorusScene(hs.desc, hs.lights, hs.bumps())
    leaf, sid, R, r = ck.tori[1]       # the upright glass torus at (0.1, 1.05, -1.4), rotated about y by 0.3
    c, s = math.cos(0.3), math.sin(0.3)
    xs = [x for x in ck.intersect([0.1 - 5 * c, 1.05, -1.4 + 5 * s], [c, 0, -s]) if x[1] == sid]
    assert len(xs) == 4
    assert np.allclose([x[0] for x in xs], [5 - R - r, 5 - R + r, 5 + R - r, 5 + R + r], rtol=0, atol=1e-12)


# ---- the loader and the flattened tables
def _scene(objects, extra=None):
    cam = {"width": 40, "height": 20, "field-of-view": 1.0, "from": [0, 1.5, -5], "to": [0, 1, 0], "up": [0, 1, 0]}
    scene = {"camera": cam, "lights": [{"point-light": {"position": [0, 4, 0], "intensity": [1, 1, 1]}}], "objects": objects}
    scene.update(extra or {})
    return json.dumps(scene)


def _kinds(d):
    return [d.leaf_kind[i] for i in range(d.n_leaves)]


def test_loader_reads_the_fixture(rtc):
    hs = tb.mix(rtc)
    d = hs.desc
    assert _kinds(d) == [1, 7, 7, 7, 7, 7, 0, 7, 2, 7, 7, 7, 7, 0]
    tori = tb.tori_of(d)
    assert [(t[2], t[3]) for t in tori] == [(1.0, 0.3), (0.8, 0.25), (0.9, 0.35), (1.0, 0.25), (0.6, 0.2), (0.7, 0.3), (0.7, 0.3),
                                            (0.7, 0.3), (0.7, 0.28), (0.5, 0.18)]
    assert sorted(d.leaf_geom[t[0]] for t in tori) == list(range(10)) and d.n_cyls == 10
    assert d.n_roots == 11 and d.n_nodes == 3
    assert [d.node_op[n] for n in range(3)] == [0, 3, 2]      # the group, the difference, the intersection
    assert np.array_equal(hs.motion()[9], [0.5, 0.1, 0.0]) and np.count_nonzero(hs.motion()) == 2
    assert hs.bumps() is not None and hs.spots() is not None


def test_loader_defaults_and_fields(rtc):
    d = rtc.HostScene(_scene([{"type": {"torus": {}}}, {"type": {"torus": {"major-radius": 3}}},
                              {"type": {"torus": {"minor-radius": 0.5}}, "casts-shadow": False,
                               "transform": [{"translate": [1, 2, 3]}], "material": {"diffuse": 0.25}}])).desc
    assert _kinds(d) == [7, 7, 7]
    assert [(d.cyl_min[i], d.cyl_max[i]) for i in range(3)] == [(1.0, 0.25), (3.0, 0.25), (1.0, 0.5)]
    assert [d.leaf_shadow[i] for i in range(3)] == [1, 1, 0]
    assert d.leaf_xform[2] != d.leaf_xform[0] and d.leaf_material[2] != d.leaf_material[0]
    assert [d.xf_inv[16 * d.leaf_xform[2] + k] for k in (3, 7, 11)] == [-1.0, -2.0, -3.0]


@pytest.mark.parametrize("cfg, key", [
    ({"major-radius": "big"}, "torus.major-radius"),
    ({"minor-radius": [1]}, "torus.minor-radius"),
    ({"major-radius": 31415.9265}, "torus.major-radius"),      # (written 1e999 below: json.dumps has no finite spelling of it)
    ({"major-radius": 2, "minor-radius": 0}, "torus.minor-radius"),
    ({"minor-radius": -0.25}, "torus.minor-radius"),
    ({"major-radius": 1, "minor-radius": 1}, "torus.minor-radius"),
    ({"major-radius": 0.2}, "torus.minor-radius"),
    ({"major-radius": -1}, "torus.minor-radius"),
    ({"radius": 1}, "torus"),
], ids=["major-string", "minor-list", "major-infinite", "minor-zero", "minor-negative", "minor-equals-major", "minor-above-major",
        "major-negative", "unknown-field"])
def test_loader_refuses_a_malformed_torus(rtc, cfg, key):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene([{"type": {"torus": cfg}}]).replace("31415.9265", "1e999"))
    assert key in str(e.value)


def test_loader_refuses_a_torus_that_is_no_object(rtc):
    with pytest.raises(rtc.RtcError) as e:
        rtc.HostScene(_scene([{"type": {"torus": 2}}]))
    assert "torus" in str(e.value)


def test_a_torus_in_a_group_a_csg_and_an_extended_definition(rtc):
    group = {"type": {"group": [{"type": {"torus": {"major-radius": 2, "minor-radius": 0.5}}, "transform": [{"rotate-x": math.pi / 2}]},
                                {"type": {"sphere": {}}}]}, "transform": [{"translate": [10, 0, 0]}]}
    csg = {"type": {"csg": {"operation": "union", "left": {"type": {"torus": {}}}, "right": {"type": {"cube": {}}}}}}
    defs = {"shape-definitions": [{"name": "ring", "value": {"type": {"torus": {"major-radius": 1.5, "minor-radius": 0.5}},
                                                            "material": {"diffuse": 0.3}}}]}
    ext = {"type": {"from-definition": "ring"}, "transform": [{"scale": [2, 2, 2]}]}
    hs = rtc.HostScene(_scene([group, csg, ext], defs))
    d = hs.desc
    assert _kinds(d) == [7, 0, 7, 2, 7]
    assert [(d.cyl_min[d.leaf_geom[i]], d.cyl_max[d.leaf_geom[i]]) for i in (0, 2, 4)] == [(2.0, 0.5), (1.0, 0.25), (1.5, 0.5)]
    assert d.xf_inv[16 * d.leaf_xform[4]] == 0.5
    # the group's box: the torus's padded box, stood upright (x: R + r, y: R + r, z: r), and moved 10 along x
    e, t = 2.5 * (1.0 + 1e-9), 0.5 * (1.0 + 1e-9)
    lo = [d.node_min[k] for k in range(3)]
    hi = [d.node_max[k] for k in range(3)]
    assert np.allclose(lo, [10 - e, -e, -1.0], rtol=0, atol=1e-12) and np.allclose(hi, [10 + e, e, 1.0], rtol=0, atol=1e-12)
    assert lo[0] < 10 - 2.5 and hi[1] > 2.5          # grown, not the bare torus
    # the checker, which takes its group boxes from these tables, finds the torus through the group
    ck = tb.TorusScene(d, hs.lights)
    ts = [x[0] for x in ck.intersect([10, 0, -5], [0, 0, 1]) if x[1] == d.leaf_id[0]]
    assert ts == []                                   # through the hole, along the upright torus's axis
    ts = [x[0] for x in ck.intersect([10 - 5, 0, 0], [1, 0, 0]) if x[1] == d.leaf_id[0]]
    assert np.allclose(ts, [2.5, 3.5, 6.5, 7.5], rtol=0, atol=1e-14)


def test_divide_takes_the_torus_box(rtc):
    """The loader divides every object at 8 children (scene.zig:588): sixteen small tori in two far clusters end up in
    sub-groups, split by their boxes; the top box is the union of the padded torus boxes."""
    ring = [{"type": {"torus": {"major-radius": 0.4, "minor-radius": 0.1}}, "transform": [{"translate": [x + 0.01 * k, 0, 1.2 * k]}]}
            for x in (-30, 30) for k in range(8)]
    d = rtc.HostScene(_scene([{"type": {"group": ring}}])).desc
    assert _kinds(d) == [7] * 16
    assert d.n_nodes >= 3                                       # the group and at least a sub-group per cluster
    e, t = 0.5 * (1.0 + 1e-9), 0.1 * (1.0 + 1e-9)
    assert np.allclose([d.node_min[k] for k in range(3)], [-30 - e, -t, -e], rtol=0, atol=1e-12)
    assert np.allclose([d.node_max[k] for k in range(3)], [30.07 + e, t, 8.4 + e], rtol=0, atol=1e-12)
    boxes = sorted((d.node_min[3 * n], d.node_max[3 * n]) for n in range(1, d.n_nodes))
    assert boxes[0][1] < 0 < boxes[-1][0]                       # no sub-group spans both clusters


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
    """tests/golden/torus_scenes/reference_tables.json: the digests of the 17 scenes' tables, taken with the host library of
    the commit before the torus."""
    want = json.load(open(os.path.join(tb.TORUS_DIR, "reference_tables.json")))
    hs = rtc.HostScene.from_file(name)
    assert TORUS not in _kinds(hs.desc)
    assert _digest(hs) == want[name]


# ---- rtc_scene_create's refusals, on the host before any HIP call
def test_create_refuses_bad_tori_without_a_gpu(rtc):
    hs = rtc.HostScene(_scene([{"type": {"sphere": {}}}, {"type": {"torus": {"major-radius": 2, "minor-radius": 0.5}}}]))
    d = hs.desc
    lib = rtc.hip_lib()
    out = C.c_void_p()
    kinds = hs.array("leaf_kind", d.n_leaves)
    geom = hs.array("leaf_geom", d.n_leaves)
    major, minor = hs.array("cyl_min", d.n_cyls), hs.array("cyl_max", d.n_cyls)
    assert kinds[1] == TORUS and (major[0], minor[0]) == (2.0, 0.5)
    geom[1] = 5
    assert lib.rtc_scene_create(C.byref(d), C.byref(out)) == 5          # RTC_ERR_BAD_INDEX
    assert b"leaf 1" in lib.rtc_last_error() and b"torus" in lib.rtc_last_error()
    geom[1] = 0
    for R, r in ((2.0, 0.0), (2.0, -0.5), (2.0, 2.0), (0.4, 0.5), (np.inf, 0.5), (2.0, np.nan), (np.nan, 0.5), (-2.0, -3.0)):
        major[0], minor[0] = R, r
        assert lib.rtc_scene_create(C.byref(d), C.byref(out)) == 1      # RTC_ERR_INVALID_ARGUMENT
        assert b"leaf 1" in lib.rtc_last_error() and b"torus" in lib.rtc_last_error()
    major[0], minor[0] = 2.0, 0.5
    kinds[1] = 8
    assert lib.rtc_scene_create(C.byref(d), C.byref(out)) == 4          # RTC_ERR_UNSUPPORTED: above RTC_TORUS
    assert b"kind 8" in lib.rtc_last_error()
    kinds[1] = TORUS


def test_multi_refuses_a_scene_with_a_torus(rtc):
    hs = tb.mix(rtc)
    lib = rtc.multi_lib()
    out = C.c_void_p()
    assert lib.rtc_multi_create(C.byref(hs.desc), 1, 0, C.byref(out)) == 4   # RTC_ERR_UNSUPPORTED, before any device call
    assert not out.value


def test_torus_constant_and_option(rtc):
    assert rtc.RTC_TORUS == 7 and "torus_kernels" in rtc.KERNEL_OPTIONS
    lib = rtc.hip_lib()
    assert lib.rtc_set_option(b"torus_kernels", 1.0) == 0
    assert lib.rtc_set_option(b"torus_kernels", 0.0) == 0
    header = open(os.path.join(REPO, "include", "rtc.h")).read()
    assert "RTC_TORUS = 7" in header


# ---- the product's conservative bounds never cull an entry the checker finds
def test_every_entry_lies_on_a_ray_that_passes_the_leafs_sphere_and_box(rtc):
    hs = tb.mix(rtc)
    d = hs.desc
    rng = np.random.default_rng(18)
    total = 0
    for leaf, sid, R, r in tb.tori_of(d):
        sphere, box = tb.leaf_bounds(d, leaf)
        assert sphere[3] > 0 and np.all(np.isfinite(box)) and np.all(box[:3] < box[3:])       # a bounded leaf
        inv = np.array([d.xf_inv[16 * d.leaf_xform[leaf] + k] for k in range(16)]).reshape(4, 4)
        centre, ext = 0.5 * (box[:3] + box[3:]), 0.5 * (box[3:] - box[:3])
        n = 10000
        o = rng.normal(size=(n, 3))
        o = centre + o / np.linalg.norm(o, axis=1)[:, None] * np.linalg.norm(ext) * rng.choice([1.5, 4.0, 50.0], size=(n, 1))
        tgt = centre + rng.uniform(-1.1, 1.1, size=(n, 3)) * ext        # some rays miss the box
        dr = tgt - o
        dr /= np.linalg.norm(dr, axis=1)[:, None]
        lo = o @ inv[:3, :3].T + inv[:3, 3]
        ld = dr @ inv[:3, :3].T
        counts, _ = tb.roots_many(lo, ld, np.full(n, R), np.full(n, r))
        hit = counts > 0
        assert hit.sum() > 1000
        total += int(hit.sum())
        # the line against the sphere
        oc = sphere[:3] - o[hit]
        along = np.einsum("ij,ij->i", oc, dr[hit])
        dist2 = np.einsum("ij,ij->i", oc, oc) - along * along
        assert np.all(dist2 <= sphere[3] ** 2), leaf
        # the line against the box
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (box[:3] - o[hit]) / dr[hit], (box[3:] - o[hit]) / dr[hit]
        tmin, tmax = np.nanmax(np.minimum(t1, t2), axis=1), np.nanmin(np.maximum(t1, t2), axis=1)
        assert np.all(tmin <= tmax), leaf
    print(f"{total} rays with entries, none outside its leaf's bounds")


# ---- the record that no existing kernel changed
def test_disassembly_identity_is_recorded():
    text = open(os.path.join(REPO, "profiles", "torus", "disassembly_identity.txt")).read()
    for obj in ("rtc_kernels.o", "rtc_motion.o", "rtc_spot.o", "rtc_bump.o", "rtc_accum.o", "rtc_adaptive.o"):
        assert obj in text and "identical" in text
    for kernel in ("rtc_render_kernel_torus", "rtc_render_kernel_torus_bigworld", "rtc_render_kernel_bump", "rtc_render_kernel_simple3_b"):
        assert kernel in text
