"""A closest-hit or shadow trace does not test a cube that lies behind the ray's origin on one of the cube's own axes
(`cube_entirely_behind`, csrc/rtc_kernels.hip: on some axis the origin is beyond a face and the direction does not
point back - or, beyond the +1 face, is "parallel" by the reference's 1e-5 rule, which multiplies by +inf).  The argument next to the code says that the reference's own
arithmetic (cube.zig:24-79) then yields no entry with t >= 0.  Here, as tests/test_early_outs_cpu.py does for the plane's
and the room's early-outs, the same conditions are evaluated in numpy float64 - whose -, x, / are the hardware's - on
millions of operand sets placed where the argument is thinnest: origins one ulp either side of +-1, directions either
side of 0 and of +-1e-5, up to the 1e10 guard and beyond it, quotients that underflow, NaNs and infinities; every case
the kernel would skip is held to what the reference's arithmetic yields.  tests/cpp/cube_behind_check.cpp runs the same
loops against the oracle's own checkAxis under the address and undefined-behaviour sanitizers; the second test builds
and runs it where a host compiler is at hand.  CPU only."""
import os
import shutil
import subprocess

import numpy as np

from test_early_outs_cpu import _reference_cube, _ulps

INF = float("inf")
NAN = float("nan")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _predicate(o, d, guard=True):
    """cube_entirely_behind, vectorised over (n, 3) origins and directions in the cube's object space."""
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        above = (o > 1.0) & ((d >= 0.0) | (ad < 1e-5))
        below = (o < -1.0) & (d <= -1e-5)
        axis = above | below
        if guard:
            axis &= ad <= 1e10
    return axis.any(axis=1)


def _cases(rng, n):
    def pick(p):
        return rng.random((n, 3)) < p

    def signs(k):
        return rng.choice([-1.0, 1.0], k)

    o = rng.uniform(-3.0, 3.0, (n, 3))
    m = pick(0.35)                                   # a few ulps either side of a face's coordinate, +-1
    o[m] = _ulps(signs(int(m.sum())), rng.integers(-3, 4, int(m.sum())))
    m = pick(0.05)                                   # far away, up to where 1 - o rounds to -o and beyond 2^200
    o[m] = signs(int(m.sum())) * 10.0 ** rng.uniform(0, 300, int(m.sum()))
    m = pick(0.01)
    o[m] = rng.choice([INF, -INF, NAN], int(m.sum()))

    d = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 1, (n, 1))
    m = pick(0.15)                                   # either side of the reference's parallel rule, to the ulp
    d[m] = _ulps(signs(int(m.sum())) * 1e-5, rng.integers(-3, 4, int(m.sum())))
    m = pick(0.1)                                    # either side of zero: +-0, denormals, tiny
    d[m] = signs(int(m.sum())) * rng.choice([0.0, 5e-324, 1e-310, 1e-300, 1e-30], int(m.sum()))
    m = pick(0.1)                                    # up to the 1e10 guard, to the ulp, and beyond it
    d[m] = _ulps(signs(int(m.sum())) * 1e10, rng.integers(-3, 4, int(m.sum())))
    m = pick(0.1)                                    # beyond the guard as far as doubles go: quotients that underflow
    d[m] = signs(int(m.sum())) * 10.0 ** rng.uniform(10, 308.25, int(m.sum()))
    m = pick(0.03)
    d[m] = rng.choice([INF, -INF, NAN, 1.7976931348623157e308, -1.7976931348623157e308], int(m.sum()))
    return o, d


def _matters(o, d):
    """Does the reference's cube test report an entry a front-only visitor looks at?  ClosestVisitor::entry and
    ShadowVisitor::entry both begin with `et >= 0`; entries are reported unless tmin > tmax."""
    tmin, tmax = _reference_cube(o, d)
    return ~(tmin > tmax) & ((tmin >= 0.0) | (tmax >= 0.0))


def test_a_cube_is_skipped_only_where_it_has_no_entry_at_or_after_the_origin():
    rng = np.random.default_rng(20261018)
    skipped = unguarded = 0
    for _ in range(8):
        o, d = _cases(rng, 500_000)
        skip = _predicate(o, d)
        matters = _matters(o, d)
        wrong = skip & matters
        assert not wrong.any(), (o[wrong][:3], d[wrong][:3])
        skipped += int(skip.sum())
        # (the guard is not vacuous: (1 - o) / d with o one ulp past the face and d near the largest double, or infinite,
        # is -0, which `t >= 0` lets through; only `|d| <= 1e10` keeps the predicate off such a ray)
        unguarded += int((_predicate(o, d, guard=False) & matters).sum())
    assert skipped > 1_000_000 and unguarded > 0


def test_the_cases_the_argument_names():
    """One operand set per clause of the comment at cube_entirely_behind."""
    inside = [0.25, -0.5]   # the other two axes: the origin between their faces, travelling along them

    def one(ox, dx):
        o = np.array([[ox, inside[0], inside[1]]])
        d = np.array([[dx, 0.3, -0.2]])
        return bool(_predicate(o, d)[0]), bool(_matters(o, d)[0])

    up = float(np.nextafter(1.0, 2.0))
    assert one(up, 1.0) == (True, False)                # one ulp beyond the face, travelling away
    assert one(1.0, 1.0) == (False, True)               # ON the face (a neighbour's coplanar face): tmax is +-0, the test runs
    assert one(-up, -1e10) == (True, False)             # at the guard
    assert one(up, float(np.nextafter(1e10, INF)))[0] is False   # past it
    assert one(up, -9e-6) == (True, False)              # pointing back, but "parallel" by the reference's rule: -inf
    assert one(up, -1e-5)[0] is False                   # pointing back for real: the ray enters the cube
    assert one(-up, -1e-5) == (True, False)             # below the cube, travelling away: positive numerators, a negative divisor
    assert one(-up, -9e-6)[0] is False and one(-up, 0.0)[0] is False   # ... "parallel": numerator x +inf = +inf, not behind
    assert one(up, INF) == (False, True)                # -2^-52 / inf = -0: an entry at "t >= 0" - the guard's case
    assert one(INF, 1.0) == (True, False)               # -inf / d
    assert one(NAN, 1.0)[0] is False and one(up, NAN)[0] is False
    assert one(0.999, 1.0)[0] is False                  # inside (a refracted ray from under_point)


def test_the_stand_alone_check_under_sanitizers():
    """tests/cpp/cube_behind_check.cpp: the same loops in C++ against the oracle's checkAxis, a program of its own built
    with -fsanitize=address,undefined (host code only; nothing is loaded into this interpreter)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    out = os.path.join(REPO, "tests", "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "cube_behind_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(REPO, "tests", "cpp", "cube_behind_check.cpp")], check=True)
    run = subprocess.run([exe, "2000000"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "wrong 0" in run.stdout and "unguarded 0" not in run.stdout, run.stdout
