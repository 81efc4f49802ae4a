// specular_skip_check - a host-only program: the specular skip's condition (ks_is_specular, csrc/rtc_kernels.hip) against the
// oracle's own power (orc::zig_pow, oracle/rtc_oracle.hpp), on operand sets placed where the argument written next to the
// condition is thinnest - the loops of tests/test_specular_skip_cpu.py.  Built with -fsanitize=address,undefined and run on
// the CPU (tests/test_specular_skip_cpu.py does both, as C++20: the oracle's zig_pow shifts a negative exponent left, which
// C++17 leaves undefined); nothing of it is loaded into another process.
//
//   specular_skip_check [operand sets, default 2000000]
//     ->  "sets N skipped S wrong W unguarded U general G short-cut mismatches M", exit 1 if W or M != 0, U or G == 0
//   wrong       skipped lanes whose specular * zig_pow(x, shininess), or a light component times it, is not specular's bits
//   unguarded   lanes the condition would skip without `x <= 1.0` that are wrong
//   general     lanes it would skip without `shininess_int != 0` that are wrong
//   mismatches  pow_small_int(x, n) != zig_pow(x, n) on finite x > 0 (the kernels' short form of the loop)
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
};

uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

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

double base(Rng& r) {
  const double p = r.unit();
  if (p < 0.15) return move_ulps(1.0, -static_cast<int>(r.next() % 6u));      // 1.0 and a few ulps below it
  if (p < 0.25) return move_ulps(1.0, 1 + static_cast<int>(r.next() % 5u));   // a few ulps above it
  if (p < 0.35) { const double v[8] = {5e-324, 1e-323, 2.2250738585072014e-308, 1e-310, 1e-162, 1e-155, 0.5, 1.0}; return v[r.next() % 8u]; }
  if (p < 0.65) return std::fmax(5e-324, std::fmin(1.0, std::exp2(r.uniform(-1074.0, 0.0))));   // denormals up to 1
  if (p < 0.75) return r.uniform(0.9, 1.0);
  if (p < 0.95) return std::fmin(kMax, std::fmax(move_ulps(1.0, 1), std::exp2(r.uniform(0.0, 1024.0))));   // above 1 up to overflow
  return std::fmax(move_ulps(1.0, 1), r.uniform(1.0, 1.1));
}

double shininess(Rng& r) {
  const double p = r.unit();
  if (p < 0.35) { const double v[5] = {2.0, 3.0, 5.0, 200.0, 1048576.0}; return v[r.next() % 5u]; }
  if (p < 0.70) return std::floor(r.uniform(2.0, 1048577.0));
  const double v[20] = {0.0, 1.0, 0.5, -0.5, 1.5, 199.5, 200.0000000001, -1.0, -2.0, -200.0, -1048576.0, 1048577.0, 2097152.0,
                        1e30, -1e30, 9223372036854775808.0, 1e300, kInf, -kInf, kNan};
  return v[r.next() % 20u];
}

// rtc_scene_create's classification (csrc/rtc_capi.hip)
uint32_t shininess_int(double s) {
  const bool small_int = s >= 2.0 && s <= 1048576.0 && s == std::floor(s);
  return small_int ? static_cast<uint32_t>(s) : 0u;
}

// pow_small_int (csrc/rtc_kernels.hip); the exponent doubled by an addition: the same value, and defined for a negative one
double pow_small_int(double x, uint32_t n) {
  double a1 = 1.0;
  int ae = 0;
  int xe;
  double x1 = std::frexp(x, &xe);
  for (uint32_t i = n; i != 0u; i >>= 1) {
    if (xe < -(1 << 12) || (1 << 12) < xe) {
      ae += xe;
      break;
    }
    if (i & 1u) {
      a1 *= x1;
      ae += xe;
    }
    x1 *= x1;
    xe += xe;
    if (x1 < 0.5) {
      x1 += x1;
      xe -= 1;
    }
  }
  return std::ldexp(a1, ae);
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 2000000ull;
  Rng rng{20261018ull};
  const double speculars[4] = {0.0, -0.0, 1e-320, 0.9};
  const double lights[10] = {1.0, 0.3, -0.7, 0.0, -0.0, kInf, -kInf, kNan, 5e-324, -1e308};
  std::vector<double> op(4);  // (on the heap: what the address sanitizer watches)
  uint64_t skipped = 0, wrong = 0, unguarded = 0, general = 0, mismatches = 0;
  for (uint64_t i = 0; i < n; ++i) {
    op[0] = base(rng);
    op[1] = shininess(rng);
    op[2] = speculars[rng.next() % 4u];
    op[3] = lights[rng.next() % 10u];
    const double x = op[0], s = op[1], specular = op[2], light = op[3];
    const uint32_t ni = shininess_int(s);
    const double ks = specular * orc::zig_pow(x, s);  // material.zig:69 as the oracle has it
    const bool zero = specular == 0.0;
    const bool skip = zero && ni != 0u && x <= 1.0;
    // a skipped lane keeps ks = specular and forms light * ks as before
    const bool differs = bits(ks) != bits(specular) || bits(light * ks) != bits(light * specular);
    skipped += skip;
    if (skip && differs) {
      if (wrong++ < 5) std::printf("WRONG x %a shininess %a specular %a light %a ks %a\n", x, s, specular, light, ks);
    }
    unguarded += zero && ni != 0u && differs;   // what `x <= 1.0` is there for
    general += zero && x <= 1.0 && differs;     // what `shininess_int != 0` is there for
    if (ni != 0u && bits(pow_small_int(x, ni)) != bits(orc::zig_pow(x, s))) {
      if (mismatches++ < 5) std::printf("SHORT-CUT x %a n %u\n", x, ni);
    }
  }
  std::printf("sets %" PRIu64 " skipped %" PRIu64 " wrong %" PRIu64 " unguarded %" PRIu64 " general %" PRIu64 " short-cut mismatches %" PRIu64 "\n",
              n, skipped, wrong, unguarded, general, mismatches);
  return wrong != 0 || mismatches != 0 || unguarded == 0 || general == 0 || skipped < n / 16;
}
