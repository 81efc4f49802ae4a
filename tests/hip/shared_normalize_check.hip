// GPU check of the shared-reciprocal normalisation of csrc/rtc_kernels.hip (shared_normalize_ok / shared_normalize)
// against the plain divisions x / m, y / m, z / m, bit for bit, the sign of a zero included, over vectors inside and
// outside the guard's range.  Built and run by tests/test_shared_normalize_gpu.py.  TEST INFRASTRUCTURE.
// refined_rcp, quotient, shared_normalize_ok and shared_normalize below are COPIES of the kernel file's: a change to one
// is a change to both.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>

__device__ __forceinline__ double refined_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(r, e, r);
}
__device__ __forceinline__ double quotient(double x, double d, double r) {
  const double q = x * r;
  return __builtin_fma(__builtin_fma(-d, q, x), r, q);
}
__device__ __forceinline__ bool shared_normalize_ok(double x, double y, double z, double m) {
  const int lowest = min(min(__builtin_amdgcn_frexp_exp(x), __builtin_amdgcn_frexp_exp(y)), __builtin_amdgcn_frexp_exp(z));
  const uint32_t m_exponent = static_cast<uint32_t>(__builtin_bit_cast(uint64_t, m) >> 52);  // (a sign bit set: out of the band)
  return (lowest >= -800) & (m_exponent - (1023u - 200u) <= 400u);
}
__device__ __forceinline__ void shared_normalize(double& x, double& y, double& z, double m) {
  const double rcp = refined_rcp(m);
  x = __builtin_copysign(quotient(x, m, rcp), x);
  y = __builtin_copysign(quotient(y, m, rcp), y);
  z = __builtin_copysign(quotient(z, m, rcp), z);
}
// (the same without the sign copy: what the test must see fail on a -0 numerator)
__device__ __forceinline__ void shared_normalize_unsigned(double& x, double& y, double& z, double m) {
  const double rcp = refined_rcp(m);
  x = quotient(x, m, rcp);
  y = quotient(y, m, rcp);
  z = quotient(z, m, rcp);
}

__device__ uint64_t mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// a number of random sign and mantissa with its exponent uniform in [emin, emax] (below -1022: a denormal)
__device__ double number(uint64_t h, int emin, int emax) {
  const uint64_t g = mix(h);
  const double v = ldexp(1.0 + static_cast<double>(h >> 12) * 0x1p-52, emin + static_cast<int>(g % static_cast<uint64_t>(emax - emin + 1)));
  return (g >> 40) & 1 ? -v : v;
}
// ... or, one time in eight, a zero of random sign: vectors with one and two zero components (and a few with three)
__device__ double component(uint64_t h, int emin, int emax) {
  const uint64_t g = mix(h ^ 0x5555555555555555ull);
  if ((g & 7) == 0) return (g >> 3) & 1 ? -0.0 : 0.0;
  return number(h, emin, emax);
}

enum { ORDINARY = 0, EXTREME = 1, NEAR_MAGNITUDE = 2, BAND_EDGES = 3, CLASSES = 4 };
enum { DIVIDED = 0, ACCEPTED = 1, BAD_GUARDED = 2, BAD_UNGUARDED = 3, BAD_UNSIGNED_GUARDED = 4, COUNTS = 5 };

__device__ bool same(double a, double b) { return __builtin_bit_cast(uint64_t, a) == __builtin_bit_cast(uint64_t, b); }

// ORDINARY: every component zero or of an exponent within +-100: the guard must accept every vector.
// EXTREME: component exponents from -1070 (denormals) to +500, zeros of both signs.
// NEAR_MAGNITUDE: one component within a few ulps of the magnitude - the others 2^-24 .. 2^-30 of it, or zero -, and
//   vectors of three equal components.
// BAND_EDGES: magnitudes of exponents -204 .. -196 and 196 .. 204, on either side of the guard's band; and magnitudes
//   inside it with one component of an exponent -806 .. -796, on either side of the numerators' limit.
__global__ void check(uint64_t seed, int cls, unsigned long long* counts, double* first) {
  const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
  const uint64_t a = mix(seed + 4 * i), b = mix(seed + 4 * i + 1), c = mix(seed + 4 * i + 2), s = mix(seed + 4 * i + 3);
  double x, y, z;
  if (cls == ORDINARY) {
    x = component(a, -100, 99);
    y = component(b, -100, 99);
    z = component(c, -100, 99);
  } else if (cls == EXTREME) {
    x = component(a, -1070, 500);
    y = component(b, -1070, 500);
    z = component(c, -1070, 500);
  } else if (cls == NEAR_MAGNITUDE) {
    const double big = number(a, -150, 150);
    double u = ldexp(big, -24 - static_cast<int>(b % 7u)), v = ldexp(big, -24 - static_cast<int>(c % 7u));
    if ((b >> 8) & 1) u = (b >> 9) & 1 ? -0.0 : 0.0;
    if ((c >> 8) & 1) v = -v;
    if ((s & 15) == 0) u = v = big;
    const uint32_t turn = static_cast<uint32_t>((s >> 4) % 3u);
    x = turn == 0 ? big : (turn == 1 ? u : v);
    y = turn == 1 ? big : (turn == 2 ? u : v);
    z = turn == 2 ? big : (turn == 0 ? u : v);
  } else {
    const int side = (s & 1) ? 196 : -204;
    const int scale = side + static_cast<int>((s >> 1) % 9u);
    x = component(a, -3, 0);
    y = component(b, -3, 0);
    z = component(c, -3, 0);
    if ((s >> 8) & 1) {  // the magnitude inside the band, one numerator at its own limit
      x = number(a, 100, 199);
      y = number(b, -806, -796);
      if ((s >> 9) & 1) z = y, y = x, x = z, z = 0.0;
    } else {
      x = ldexp(x, scale);
      y = ldexp(y, scale);
      z = ldexp(z, scale);
    }
  }
  const double m = __builtin_sqrt((x * x + y * y) + z * z);  // as the kernel forms it
  const bool divided = m != 0.0;
  bool accepted = false, bad = false, bad_unsigned = false;
  double px = x, py = y, pz = z, qx = x, qy = y, qz = z, ux = x, uy = y, uz = z;
  if (divided) {
    px = x / m;
    py = y / m;
    pz = z / m;
    accepted = shared_normalize_ok(x, y, z, m);
    shared_normalize(qx, qy, qz, m);
    shared_normalize_unsigned(ux, uy, uz, m);
    bad = !(same(px, qx) && same(py, qy) && same(pz, qz));
    bad_unsigned = !(same(px, ux) && same(py, uy) && same(pz, uz));
  }
  const bool flags[COUNTS] = {divided, accepted, bad && accepted, bad, bad_unsigned && accepted};
  for (int k = 0; k < COUNTS; ++k) {
    const unsigned long long n = static_cast<unsigned long long>(__builtin_popcountll(__ballot(flags[k])));
    if ((threadIdx.x & 63u) == 0u && n != 0ull) atomicAdd(counts + COUNTS * cls + k, n);
  }
  if (bad && accepted && atomicAdd(counts + COUNTS * CLASSES, 1ull) == 0ull) {
    first[0] = x; first[1] = y; first[2] = z; first[3] = m;
    first[4] = px; first[5] = py; first[6] = pz;
    first[7] = qx; first[8] = qy; first[9] = qz;
  }
}

int main() {
  static const char* names[CLASSES] = {"ordinary", "extreme", "near_magnitude", "band_edges"};
  unsigned long long* d_counts;
  double* d_first;
  const size_t n_counts = COUNTS * CLASSES + 1;
  if (hipMalloc(&d_counts, n_counts * sizeof *d_counts) != hipSuccess || hipMalloc(&d_first, 10 * sizeof(double)) != hipSuccess ||
      hipMemset(d_counts, 0, n_counts * sizeof *d_counts) != hipSuccess || hipMemset(d_first, 0, 10 * sizeof(double)) != hipSuccess) {
    std::printf("shared_normalize_check: HIP error\n");
    return 2;
  }
  unsigned long long per_class = 0;
  // (a launch draws mix(seed .. seed + 2^26): the repetitions' seeds lie 2^28 apart, the classes' 2^36, so no two launches share an input)
  for (int rep = 0; rep < 4; ++rep) {
    for (int cls = 0; cls < CLASSES; ++cls)
      hipLaunchKernelGGL(check, dim3(1 << 16), dim3(256), 0, 0, 0x2468ACEull + (static_cast<uint64_t>(rep) << 28) + 0x1000000000ull * cls, cls, d_counts, d_first);
    per_class += 1ull << 24;
  }
  if (hipDeviceSynchronize() != hipSuccess) {
    std::printf("shared_normalize_check: HIP error\n");
    return 2;
  }
  unsigned long long counts[COUNTS * CLASSES + 1];
  double first[10];
  (void)hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost);
  (void)hipMemcpy(first, d_first, sizeof first, hipMemcpyDeviceToHost);
  std::printf("shared_normalize_check: %llu vectors\n", per_class * CLASSES);
  for (int cls = 0; cls < CLASSES; ++cls) {
    const unsigned long long* c = counts + COUNTS * cls;
    std::printf("class %s: vectors %llu divided %llu accepted %llu bad_guarded %llu bad_unguarded %llu bad_unsigned_guarded %llu\n",
                names[cls], per_class, c[DIVIDED], c[ACCEPTED], c[BAD_GUARDED], c[BAD_UNGUARDED], c[BAD_UNSIGNED_GUARDED]);
  }
  if (counts[COUNTS * CLASSES])
    std::printf("first: v=(%a %a %a) m=%a  plain (%a %a %a) shared (%a %a %a)\n", first[0], first[1], first[2], first[3], first[4],
                first[5], first[6], first[7], first[8], first[9]);
  return 0;
}
