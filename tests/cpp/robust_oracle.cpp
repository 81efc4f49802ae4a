// robust_oracle.cpp — robust accumulation's checker.  TEST INFRASTRUCTURE: include/rtc.h's contract of rtc_robust_device
//  restated as plain loops in doubles, built with -ffp-contract=off; it includes and links nothing of
// the product.  Every operation is the contract's, in its order, so the results are held to the kernels' bit for bit.
#include <cmath>
#include <cstdint>
#include <limits>

namespace {

constexpr uint32_t kMaxBuckets = 15u;  // RTC_ROBUST_MAX_BUCKETS

uint32_t clamp8(double channel) {  // (rtc_rgba8_device's clamp)
  const double t = std::round(channel * 255);
  if (!(t >= 0)) return 0u;
  if (t > 255) return 255u;
  return static_cast<uint32_t>(t);
}

}  // namespace

extern "C" {

// sums [M][n][3]; mean [n][3]; sumsq, rejected, gini (G0), variance (v), each [n] or NULL.  0, or 1 for what the contract refuses.
int robust_oracle(const double* sums, uint64_t n, uint32_t passes, uint32_t M, double gain, double* mean, double* sumsq,
                  uint32_t* rejected, double* gini, double* variance) {
  if (!sums || !mean || n == 0u || n > (1ull << 40) || M % 2u == 0u || M < 3u || M > kMaxBuckets || passes < M ||
      !std::isfinite(gain) || gain < 0.0)
    return 1;
  const uint32_t h = (M - 1u) / 2u;
  const double inf = std::numeric_limits<double>::infinity();
  for (uint64_t p = 0; p < n; ++p) {
    double m[kMaxBuckets][3], k[kMaxBuckets];
    uint32_t rank[kMaxBuckets];
    // 1. bucket means and keys
    for (uint32_t j = 0; j < M; ++j) {
      const uint32_t n_j = passes / M + (j < passes % M ? 1u : 0u);
      for (int c = 0; c < 3; ++c) m[j][c] = sums[(static_cast<uint64_t>(j) * n + p) * 3u + c] / static_cast<double>(n_j);
      const double y = (0.2126 * m[j][0] + 0.7152 * m[j][1]) + 0.0722 * m[j][2];
      k[j] = (y - y == 0) ? (y > 0 ? y : 0.0) : inf;
    }
    // 2. rank
    for (uint32_t j = 0; j < M; ++j) {
      rank[j] = 0u;
      for (uint32_t i = 0; i < M; ++i)
        if (i != j && (k[i] < k[j] || (k[i] == k[j] && i < j))) ++rank[j];
    }
    // 3. the Gini coefficient
    double T = 0.0, A = 0.0;
    for (uint32_t j = 0; j < M; ++j) T = T + k[j];
    for (uint32_t j = 0; j < M; ++j) A = A + static_cast<double>(rank[j] + 1u) * k[j];
    const double G0 = (T > 0 && T < inf) ? (2.0 * A) / (static_cast<double>(M) * T) - static_cast<double>(M + 1u) / static_cast<double>(M)
                                         : (T > 0 ? 1.0 : 0.0);
    const double g = gain * G0;
    const double G = g > 0 ? (g < 1 ? g : 1.0) : 0.0;
    // 4. the kept half-width
    uint32_t c = static_cast<uint32_t>(std::floor((1.0 - G) * static_cast<double>(h) + 0.5));
    if (c > h) c = h;
    const uint32_t kept = 2u * c + 1u;
    // 5. the outputs
    double u[3];
    for (int ch = 0; ch < 3; ++ch) {
      double s = 0.0;
      for (uint32_t j = 0; j < M; ++j)
        if (h - c <= rank[j] && rank[j] <= h + c) s = s + m[j][ch];
      u[ch] = s / static_cast<double>(kept);
      mean[p * 3u + ch] = u[ch];
    }
    if (rejected) rejected[p] = M - kept;
    if (gini) gini[p] = G0;
    // 6. the variance of that mean
    const uint32_t cv = c > 1u ? c : 1u, kv = 2u * cv + 1u;
    double D = 0.0;
    for (uint32_t j = 0; j < M; ++j)
      if (h - cv <= rank[j] && rank[j] <= h + cv) {
        const double d[3] = {m[j][0] - u[0], m[j][1] - u[1], m[j][2] - u[2]};
        D = D + ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      }
    const double v = D / (3.0 * (static_cast<double>(kv - 1u) * static_cast<double>(kv)));
    const double P = static_cast<double>(passes);
    if (variance) variance[p] = v;
    if (sumsq) sumsq[p] = P * ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + (3.0 * ((P - 1.0) * P)) * v;
  }
  return 0;
}

// 7. the clamp
void robust_oracle_rgba(const double* image, uint64_t n, uint32_t* rgba) {
  for (uint64_t p = 0; p < n; ++p)
    rgba[p] = clamp8(image[3 * p]) | (clamp8(image[3 * p + 1]) << 8) | (clamp8(image[3 * p + 2]) << 16) | 0xFF000000u;
}

}  // extern "C"
