// denoise_oracle.cpp — the denoiser's checker.  TEST INFRASTRUCTURE: include/rtc.h's contract of rtc_denoise_device
//  restated as plain loops in doubles, built with -ffp-contract=off; it includes and links nothing of
// the product.  Rows are shared among threads; a pixel's value does not depend on that.
//
// `flags` selects a variant for the tests that show a mistake missing its bound: NO_CANCEL leaves the c3 term out of a
// distance.
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace {

constexpr double kEps = 1e-10;  // RTC_DENOISE_EPS
constexpr uint32_t NO_CANCEL = 1u;

struct Job {
  const double* u;
  const double* s;
  int64_t w, h;
  uint32_t passes;
  const uint32_t* tile_passes;
  uint32_t tile_w, tile_h;
  int radius, patch;
  double k2, c3;
  uint32_t flags;
  double* out;
  std::vector<double> v;
};

uint32_t passesAt(const Job& j, int64_t x, int64_t y) {
  if (!j.tile_passes) return j.passes;
  const int64_t tiles_x = (j.w + j.tile_w - 1) / j.tile_w;
  return j.tile_passes[(y / j.tile_h) * tiles_x + x / j.tile_w];
}

double varianceAt(const Job& j, int64_t x, int64_t y) {
  const uint32_t p = passesAt(j, x, y);
  if (p < 2u) return 0.0;
  const double P = static_cast<double>(p);
  const double* u = j.u + 3 * (y * j.w + x);
  const double d = j.s[y * j.w + x] - P * ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  const double m = d > 0.0 ? d : 0.0;
  return m / (3.0 * ((P - 1.0) * P));
}

void pixel(const Job& j, int64_t px, int64_t py) {
  double W = 0.0, A[3] = {0.0, 0.0, 0.0};
  for (int dy = -j.radius; dy <= j.radius; ++dy)
    for (int dx = -j.radius; dx <= j.radius; ++dx) {
      const int64_t qx = px + dx, qy = py + dy;
      if (qx < 0 || qx >= j.w || qy < 0 || qy >= j.h) continue;
      double S = 0.0;
      int n = 0;
      for (int oy = -j.patch; oy <= j.patch; ++oy)
        for (int ox = -j.patch; ox <= j.patch; ++ox) {
          const int64_t ax = px + ox, ay = py + oy, bx = qx + ox, by = qy + oy;
          if (ax < 0 || ax >= j.w || ay < 0 || ay >= j.h || bx < 0 || bx >= j.w || by < 0 || by >= j.h) continue;
          const double* ua = j.u + 3 * (ay * j.w + ax);
          const double* ub = j.u + 3 * (by * j.w + bx);
          const double va = j.v[ay * j.w + ax], vb = j.v[by * j.w + bx];
          const double dr = ua[0] - ub[0], dg = ua[1] - ub[1], db = ua[2] - ub[2];
          const double vmin = vb < va ? vb : va;
          double t = (dr * dr + dg * dg) + db * db;
          if (!(j.flags & NO_CANCEL)) t = t - j.c3 * (va + vmin);
          S = S + t / (kEps + j.k2 * (va + vb));
          n = n + 1;
        }
      const double q = S / (3.0 * static_cast<double>(n));
      const double w = std::exp(-(q > 0.0 ? q : 0.0));
      const double* uq = j.u + 3 * (qy * j.w + qx);
      W = W + w;
      for (int c = 0; c < 3; ++c) A[c] = A[c] + w * uq[c];
    }
  for (int c = 0; c < 3; ++c) j.out[3 * (py * j.w + px) + c] = A[c] / W;
}

}  // namespace

extern "C" {

// mean [h][w][3], sumsq [h][w], tile_passes [T] or NULL, out [h][w][3]; threads 0: as many as the machine has, at most 16.
// Returns 0, or 1 for an argument the contract refuses.
int denoise_oracle(const double* mean, const double* sumsq, uint32_t w, uint32_t h, uint32_t passes, const uint32_t* tile_passes,
                   uint32_t tile_w, uint32_t tile_h, uint32_t radius, uint32_t patch, double strength, double cancel, uint32_t flags,
                   uint32_t threads, double* out) {
  if (!mean || !sumsq || !out || w == 0u || h == 0u || radius > 10u || patch > 3u) return 1;
  if (!std::isfinite(strength) || strength <= 0.0 || !std::isfinite(cancel) || cancel < 0.0) return 1;
  if (tile_passes ? (tile_w == 0u || tile_h == 0u) : passes < 2u) return 1;
  Job j{mean, sumsq, w, h, passes, tile_passes, tile_w, tile_h, static_cast<int>(radius), static_cast<int>(patch),
        strength * strength, 3.0 * cancel, flags, out, {}};
  j.v.resize(static_cast<size_t>(w) * h);
  for (int64_t y = 0; y < j.h; ++y)
    for (int64_t x = 0; x < j.w; ++x) j.v[y * j.w + x] = varianceAt(j, x, y);
  uint32_t n = threads ? threads : std::thread::hardware_concurrency();
  n = n < 1u ? 1u : (n > 16u ? 16u : n);
  if (n > h) n = h;
  std::vector<std::thread> pool;
  for (uint32_t t = 0; t < n; ++t)
    pool.emplace_back([&j, t, n] {
      for (int64_t y = t; y < j.h; y += n)
        for (int64_t x = 0; x < j.w; ++x) pixel(j, x, y);
    });
  for (std::thread& t : pool) t.join();
  return 0;
}

uint32_t denoise_oracle_flags(void) { return NO_CANCEL; }
}
