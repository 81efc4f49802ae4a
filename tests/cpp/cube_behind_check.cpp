// cube_behind_check - a host-only program: cube_entirely_behind's conditions (csrc/rtc_kernels.hip) against the oracle's
// own cube arithmetic (orc::checkAxis, oracle/rtc_oracle.hpp), on operand sets placed where the argument written next to
// the predicate is thinnest - the loops of tests/test_cube_behind_cpu.py.  Built with -fsanitize=address,undefined and
// run on the CPU (tests/test_cube_behind_cpu.py does both); nothing of it is loaded into another process.
//
//   cube_behind_check [operand sets, default 4000000]   ->  "sets N skipped S wrong W unguarded U", exit 1 if W != 0 or U == 0
#include "../../oracle/rtc_oracle.hpp"

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// splitmix64: a generator of this file's own, so that a run is the same everywhere
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double unit() { return static_cast<double>(next() >> 11) * 0x1p-53; }  // [0, 1)
  double uniform(double a, double b) { return a + (b - a) * unit(); }
  double sign() { return (next() & 1u) ? 1.0 : -1.0; }
  int ulps() { return static_cast<int>(next() % 7u) - 3; }
};

double move_ulps(double x, int k) {
  int64_t b;
  std::memcpy(&b, &x, sizeof b);
  b += k;
  std::memcpy(&x, &b, sizeof x);
  return x;
}

const double kInf = orc::INF;
const double kNan = std::numeric_limits<double>::quiet_NaN();
const double kMax = std::numeric_limits<double>::max();

double origin(Rng& r) {
  const double p = r.unit();
  if (p < 0.35) return move_ulps(r.sign(), r.ulps());                 // a few ulps either side of a face
  if (p < 0.40) return r.sign() * std::pow(10.0, r.uniform(0.0, 300.0));
  if (p < 0.41) { const double v[3] = {kInf, -kInf, kNan}; return v[r.next() % 3u]; }
  return r.uniform(-3.0, 3.0);
}

double direction(Rng& r) {
  const double p = r.unit();
  if (p < 0.15) return move_ulps(r.sign() * 1e-5, r.ulps());          // either side of the reference's parallel rule
  if (p < 0.25) { const double v[5] = {0.0, 5e-324, 1e-310, 1e-300, 1e-30}; return r.sign() * v[r.next() % 5u]; }
  if (p < 0.35) return move_ulps(r.sign() * 1e10, r.ulps());          // at the guard
  if (p < 0.45) return r.sign() * std::pow(10.0, r.uniform(10.0, 308.25));  // beyond it: quotients that underflow
  if (p < 0.48) { const double v[5] = {kInf, -kInf, kNan, kMax, -kMax}; return v[r.next() % 5u]; }
  return r.uniform(-1.0, 1.0) * std::pow(10.0, r.uniform(-3.0, 1.0));
}

// cube_entirely_behind, one axis
bool behind(double o, double d, bool guard) {
  const double ad = std::fabs(d);
  const bool above = (o > 1.0) & ((d >= 0.0) | (ad < 1e-5)), below = (o < -1.0) & (d <= -1e-5);
  return (above | below) & (!guard | (ad <= 1e10));
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4000000ull;
  Rng rng{20261018ull};
  std::vector<double> o(3), d(3);  // (on the heap: what the address sanitizer watches)
  uint64_t skipped = 0, wrong = 0, unguarded = 0;
  for (uint64_t i = 0; i < n; ++i) {
    for (int a = 0; a < 3; ++a) {
      o[a] = origin(rng);
      d[a] = direction(rng);
    }
    // cube.zig:49-79 as the oracle has it (slabIntersect) for the unit cube
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) orc::checkAxis(o[a], d[a], -1.0, 1.0, lo[a], hi[a]);
    const double tmin = std::fmax(lo[0], std::fmax(lo[1], lo[2]));
    const double tmax = std::fmin(hi[0], std::fmin(hi[1], hi[2]));
    const bool matters = !(tmin > tmax) && (tmin >= 0.0 || tmax >= 0.0);  // an entry a front-only visitor looks at
    const bool skip = behind(o[0], d[0], true) | behind(o[1], d[1], true) | behind(o[2], d[2], true);
    const bool loose = behind(o[0], d[0], false) | behind(o[1], d[1], false) | behind(o[2], d[2], false);
    skipped += skip;
    if (skip && matters) {
      if (wrong++ < 5) std::printf("WRONG o %a %a %a d %a %a %a tmin %a tmax %a\n", o[0], o[1], o[2], d[0], d[1], d[2], tmin, tmax);
    }
    unguarded += loose && matters;  // what the |d| <= 1e10 guard is there for
  }
  std::printf("sets %" PRIu64 " skipped %" PRIu64 " wrong %" PRIu64 " unguarded %" PRIu64 "\n", n, skipped, wrong, unguarded);
  return wrong != 0 || unguarded == 0 || skipped < n / 8;
}
