"""A lane of the simple kernels does not run the specular power when its material has no specular term
(`ks_is_specular`, csrc/rtc_kernels.hip, render_body's point-light branch): with `specular` a zero of either sign, an integer
shininess in 2 .. 2^20 (DevMaterial::shininess_int != 0, the pow_small_int path) and 0 < reflect_dot_eye <= 1 the lane keeps
ks = specular.  The argument next to the code says that the reference's own arithmetic (material.zig:69,
`specular * std.math.pow(f64, reflect_dot_eye, shininess)`) yields that very zero, to the bit: the squaring loop returns a
finite value >= +0 there, and (+-0) * that is +-0 with specular's sign.  Here, as tests/test_cube_behind_cpu.py does for the
cube's early-out, pow_small_int and zig_pow are restated in float64 - whose x and + are the hardware's - and run on
operand sets placed where the argument is thinnest: denormal bases, bases whose power underflows, 1.0 and a few ulps either
side of it, bases above 1 up to overflow; shininess 2, 3, 5, 200, 2^20 and random integers, and the non-integer, negative and
huge ones that take zig_pow's general path; specular +0, -0, 1e-320 and 0.9; light intensities that are negative, zeros of
both signs, infinite and NaN.  tests/cpp/specular_skip_check.cpp runs the same loops against the oracle's own zig_pow under the
address and undefined-behaviour sanitizers; the last test builds and runs it where a host compiler is at hand.  CPU only."""
import math
import os
import shutil
import subprocess

import numpy as np

INF = float("inf")
NAN = float("nan")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _shininess_int(shininess):
    """rtc_scene_create's classification (csrc/rtc_capi.hip): the shininess as an integer if it is one in 2 .. 2^20, else 0."""
    s = np.asarray(shininess, dtype=np.float64)
    with np.errstate(all="ignore"):
        small = (s >= 2.0) & (s <= 1048576.0) & (s == np.floor(s))
    return np.where(small, s, 0.0).astype(np.uint32)


def _predicate(specular, shininess, x, guard=True, int_only=True):
    """ks_is_specular.  guard=False drops `reflect_dot_eye <= 1.0`, int_only=False drops `shininess_int != 0`: the two clauses
    the tests below show to be needed."""
    skip = np.asarray(specular) == 0.0
    if int_only:
        skip = skip & (_shininess_int(shininess) != 0)
    if guard:
        skip = skip & (np.asarray(x) <= 1.0)
    return skip


def _pow_small_int(x, n):
    """pow_small_int (csrc/rtc_kernels.hip), vectorised: finite x > 0, integer n."""
    x1, xe = np.frexp(np.asarray(x, dtype=np.float64))
    xe = xe.astype(np.int64)
    a1 = np.ones_like(x1)
    ae = np.zeros(x1.shape, dtype=np.int64)
    i = np.asarray(n).astype(np.int64) + np.zeros(x1.shape, dtype=np.int64)
    live = i != 0
    with np.errstate(all="ignore"):
        while live.any():
            out = live & ((xe < -(1 << 12)) | ((1 << 12) < xe))
            ae = np.where(out, ae + xe, ae)
            live = live & ~out
            odd = live & ((i & 1) == 1)
            a1 = np.where(odd, a1 * x1, a1)
            ae = np.where(odd, ae + xe, ae)
            x1 = np.where(live, x1 * x1, x1)
            xe = np.where(live, xe << 1, xe)
            low = live & (x1 < 0.5)
            x1 = np.where(low, x1 + x1, x1)
            xe = np.where(low, xe - 1, xe)
            i = np.where(live, i >> 1, i)
            live = live & (i != 0)
        return np.ldexp(a1, ae.astype(np.int32))


def _is_odd_integer(v):
    if abs(v) >= 9007199254740992.0:
        return False
    ip = float(math.trunc(v))
    return v == ip and (int(ip) & 1) == 1


def _zig_pow(x, y):
    """zig_pow (csrc/rtc_kernels.hip; Zig's std.math.pow), one operand pair."""
    x, y = float(x), float(y)
    with np.errstate(all="ignore"):
        if y == 0.0 or x == 1.0:
            return 1.0
        if x != x or y != y:
            return NAN
        if y == 1.0:
            return x
        if x == 0.0:
            if y < 0.0:
                return math.copysign(INF, x) if _is_odd_integer(y) else INF
            return x if _is_odd_integer(y) else 0.0
        if math.isinf(y):
            if x == -1.0:
                return 1.0
            return 0.0 if (abs(x) < 1.0) == (y > 0.0) else INF
        if math.isinf(x):
            if x < 0.0:
                if y < 0.0:
                    return -0.0 if _is_odd_integer(y) else 0.0
                return -INF if _is_odd_integer(y) else INF
            return 0.0 if y < 0.0 else INF
        if y == 0.5:
            return math.sqrt(x)
        if y == -0.5:
            return 1.0 / math.sqrt(x)
        ay = abs(y)
        yi = float(math.trunc(ay))
        yf = ay - yi
        if yf != 0.0 and x < 0.0:
            return NAN
        if yi >= 9223372036854775808.0:
            return float(np.exp(np.float64(y) * np.log(np.float64(x))))
        a1, ae = 1.0, 0
        if yf != 0.0:
            if yf > 0.5:
                yf -= 1.0
                yi += 1.0
            a1 = float(np.exp(np.float64(yf) * np.log(np.float64(x))))
        x1, xe = math.frexp(x)
        i = int(yi)
        while i != 0:
            if xe < -(1 << 12) or (1 << 12) < xe:
                ae += xe
                break
            if i & 1:
                a1 *= x1
                ae += xe
            x1 *= x1
            xe <<= 1
            if x1 < 0.5:
                x1 += x1
                xe -= 1
            i >>= 1
        if y < 0.0:
            a1 = float(np.float64(1.0) / np.float64(a1))
            ae = -ae
        return float(np.ldexp(np.float64(a1), np.int32(max(-(1 << 30), min(1 << 30, ae)))))


def _power(x, shininess):
    """What the lighting code multiplies `specular` by: pow_small_int where shininess_int says so and x is finite, else zig_pow."""
    x = np.asarray(x, dtype=np.float64)
    shininess = np.asarray(shininess, dtype=np.float64) + np.zeros_like(x)
    n = _shininess_int(shininess)
    fast = (n != 0) & (x < INF)
    out = np.empty_like(x)
    out[fast] = _pow_small_int(x[fast], n[fast])
    slow = np.flatnonzero(~fast)
    out[slow] = [_zig_pow(x[k], shininess[k]) for k in slow]
    return out


def _ulps(x, k):
    return (_bits(x) + np.asarray(k, dtype=np.int64)).view(np.float64)


SPECULARS = np.array([0.0, -0.0, 1e-320, 0.9])
LIGHTS = np.array([1.0, 0.3, -0.7, 0.0, -0.0, INF, -INF, NAN, 5e-324, -1e308])
INT_SHININESS = np.array([2.0, 3.0, 5.0, 200.0, 1048576.0])
OTHER_SHININESS = np.array([0.0, 1.0, 0.5, -0.5, 1.5, 199.5, 200.0000000001, -1.0, -2.0, -200.0, -1048576.0, 1048577.0, 2097152.0,
                            1e30, -1e30, 9223372036854775808.0, 1e300, INF, -INF, NAN])


def _bases_to_one(rng, n):
    """(0, 1]: denormals, the smallest double, bases whose power underflows, 1.0, a few ulps below it, the rest spread in exponent"""
    x = 2.0 ** rng.uniform(-1074.0, 0.0, n)
    x = np.minimum(np.maximum(x, 5e-324), 1.0)
    m = rng.random(n) < 0.2
    x[m] = _ulps(np.ones(int(m.sum())), -rng.integers(0, 6, int(m.sum())))
    m = rng.random(n) < 0.1
    x[m] = rng.choice([5e-324, 1e-323, 2.2250738585072014e-308, 2.225073858507201e-308, 1e-310, 1e-162, 1e-155, 0.5, 1.0], int(m.sum()))
    m = rng.random(n) < 0.1
    x[m] = rng.uniform(0.9, 1.0, int(m.sum()))
    return x


def _bases_above_one(rng, n):
    """(1, max]: a few ulps above 1.0, bases whose power overflows, the largest double"""
    x = 2.0 ** rng.uniform(0.0, 1024.0, n)
    x = np.minimum(np.maximum(x, np.nextafter(1.0, 2.0)), 1.7976931348623157e308)
    m = rng.random(n) < 0.3
    x[m] = _ulps(np.ones(int(m.sum())), rng.integers(1, 6, int(m.sum())))
    m = rng.random(n) < 0.1
    x[m] = rng.uniform(1.0, 1.1, int(m.sum()))
    x[x <= 1.0] = np.nextafter(1.0, 2.0)
    return x


def _check(specular, shininess, x, light, **clauses):
    """-> (lanes the predicate skips, lanes among them whose skipped product is NOT the kept one to the bit)"""
    skip = _predicate(specular, shininess, x, **clauses)
    with np.errstate(all="ignore"):
        ks = specular * _power(x, shininess)       # the parent's ks
        wrong = skip & (_bits(ks) != _bits(specular))
        # pr / pg / pb = L * ks, formed either way: the same bits, the sign of a zero and a NaN or infinite intensity included
        wrong |= skip & (_bits(light * ks) != _bits(light * np.where(skip, specular, ks)))
    return skip, wrong


def test_a_skipped_lane_keeps_the_reference_bits():
    rng = np.random.default_rng(20261018)
    skipped = 0
    for _ in range(4):
        n = 400_000
        x = np.where(rng.random(n) < 0.7, _bases_to_one(rng, n), _bases_above_one(rng, n))
        shininess = np.where(rng.random(n) < 0.5, rng.choice(INT_SHININESS, n), np.floor(rng.uniform(2.0, 1048577.0, n)))
        specular, light = rng.choice(SPECULARS, n), rng.choice(LIGHTS, n)
        skip, wrong = _check(specular, shininess, x, light)
        assert not wrong.any(), (x[wrong][:3], shininess[wrong][:3], specular[wrong][:3])
        assert not skip[x > 1.0].any() and not skip[specular != 0.0].any()
        assert skip[(x <= 1.0) & (specular == 0.0)].all()   # (every shininess here is an integer in range)
        skipped += int(skip.sum())
    assert skipped > 500_000


def test_the_base_guard_is_needed():
    """Above 1.0 the power overflows - 0 * inf is a NaN in the reference -: the predicate leaves every such lane on the
    parent's path, and without `<= 1.0` it would not."""
    rng = np.random.default_rng(7)
    n = 200_000
    x = _bases_above_one(rng, n)
    shininess = np.where(rng.random(n) < 0.5, rng.choice(INT_SHININESS, n), np.floor(rng.uniform(2.0, 1048577.0, n)))
    specular, light = rng.choice(SPECULARS[:2], n), rng.choice(LIGHTS, n)
    skip, wrong = _check(specular, shininess, x, light)
    assert not skip.any() and not wrong.any()
    skip, wrong = _check(specular, shininess, x, light, guard=False)
    assert skip.all() and wrong.sum() > 1000      # (NaN where the power is infinite)
    # one ulp above 1.0 the power is still finite for every exponent of the table: the guard is at the first base for which
    # the argument's "the mantissa loop cannot overflow" stops being a one-line statement, not at the first that fails
    up = np.full(5, np.nextafter(1.0, 2.0))
    assert not _predicate(np.zeros(5), INT_SHININESS, up).any()
    assert _predicate(np.zeros(5), INT_SHININESS, np.ones(5)).all()


def test_the_integer_clause_is_needed():
    """A shininess that is no integer in 2 .. 2^20 takes zig_pow's general path, which overflows for a negative exponent
    (0 * inf: NaN) and returns NaN for a NaN one: the predicate leaves those lanes alone, and without `shininess_int != 0`
    it would not."""
    rng = np.random.default_rng(11)
    n = 30_000
    x = _bases_to_one(rng, n)
    shininess = rng.choice(OTHER_SHININESS, n)
    assert (_shininess_int(OTHER_SHININESS) == 0).all() and (_shininess_int(INT_SHININESS) == INT_SHININESS).all()
    specular, light = rng.choice(SPECULARS[:2], n), rng.choice(LIGHTS, n)
    skip, wrong = _check(specular, shininess, x, light)
    assert not skip.any() and not wrong.any()
    skip, wrong = _check(specular, shininess, x, light, int_only=False)
    assert skip.all() and wrong.sum() > 100


def test_a_specular_term_is_never_skipped():
    rng = np.random.default_rng(13)
    n = 100_000
    x = _bases_to_one(rng, n)
    for specular in (1e-320, 5e-324, -5e-324, 0.9, -0.9, INF, NAN):
        assert not _predicate(np.full(n, specular), rng.choice(INT_SHININESS, n), x).any()


def test_the_cases_the_argument_names():
    def one(specular, shininess, x):
        skip, wrong = _check(np.array([specular]), np.array([shininess]), np.array([x]), np.array([-0.7]))
        assert not wrong[0]
        with np.errstate(all="ignore"):
            ks = np.array([specular]) * _power(np.array([x]), np.array([shininess]))
        return bool(skip[0]), float(ks[0])

    def same(a, b):
        return _bits(a) == _bits(b)

    s, ks = one(0.0, 200.0, 0.5)
    assert s and same(ks, 0.0)
    s, ks = one(-0.0, 200.0, 0.5)
    assert s and same(ks, -0.0)                                  # the sign of the zero is specular's
    s, ks = one(-0.0, 1048576.0, 5e-324)
    assert s and same(ks, -0.0)                                  # the power underflows to +0: (-0) * (+0) = -0
    s, ks = one(0.0, 2.0, 1.0)
    assert s and same(ks, 0.0)                                   # ON the guard
    assert one(0.0, 200.0, float(np.nextafter(1.0, 2.0)))[0] is False
    s, ks = one(0.0, 200.0, 1e300)
    assert not s and ks != ks                                    # what the guard is for: 0 * inf
    s, ks = one(0.0, -200.0, 1e-300)
    assert not s and ks != ks                                    # zig_pow's path: 0 * inf
    assert one(0.0, 199.5, 0.5)[0] is False and one(0.0, 1.0, 0.5)[0] is False and one(0.0, 1048577.0, 0.5)[0] is False
    assert one(1e-320, 200.0, 0.5)[0] is False                   # a denormal specular is a specular term
    # pow_small_int is zig_pow on its domain
    for x in (5e-324, 1e-310, 0.3, 1.0 - 2.0 ** -53, 1.0, 1.5, 1e300):
        for n in (2, 3, 5, 200, 1048576, 77777):
            assert same(_pow_small_int(np.array([x]), np.array([n]))[0], _zig_pow(x, float(n))), (x, n)


def test_the_stand_alone_check_under_sanitizers():
    """tests/cpp/specular_skip_check.cpp: the same loops in C++ against the oracle's zig_pow, a program of its own built with
    -fsanitize=address,undefined (host code only; nothing is loaded into this interpreter).  As C++20: the oracle's zig_pow
    doubles the base's exponent with `xe <<= 1`, negative for a base below 1, which C++20 defines (as every compiler did
    before it) and the undefined-behaviour sanitizer reports under C++17."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    out = os.path.join(REPO, "tests", "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "specular_skip_check")
    subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(REPO, "tests", "cpp", "specular_skip_check.cpp")], check=True)
    run = subprocess.run([exe, "1000000"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "wrong 0" in run.stdout and "unguarded 0" not in run.stdout and "general 0" not in run.stdout, run.stdout
