// adaptive_oracle.cpp — CPU checker of adaptive sampling (libadaptive_oracle.so).  TEST INFRASTRUCTURE.
//
// Adaptive sampling (include/rtc.h rtc_scene_adaptive_*) restated on the host: one round's
// accumulation of a compact tile frame into whole-image sums, each tile's noise in the order the kernel documents (items of
// two horizontally adjacent pixels, item i to lane i mod B, each lane's terms in item order, an xor butterfly in each wave
// of 64 lanes, the waves' totals in order), the stopping rule and the ascending active list.  The sample-pass checker is
// included, read-only, so that one library renders the passes (pass_render) and accumulates them; tests/adaptive_binding.py
// runs the rounds.  Nothing of the product is included or linked.
#include "progressive_oracle.cpp"

#include <cmath>
#include <limits>

namespace adapt {

// Lanes of the kernel's work-group for a tile shape: its items rounded up to whole waves, at most 1024
uint32_t block(uint32_t tile_w, uint32_t tile_h) {
  const uint64_t items = static_cast<uint64_t>(tile_h) * ((tile_w + 1u) / 2u);
  const uint64_t b = (items + 63u) / 64u * 64u;
  return static_cast<uint32_t>(std::min<uint64_t>(b, 1024u));
}

// color.zig:61-71's clamp
uint32_t clamp8(double channel) {
  const double t = std::round(channel * 255);
  if (!(t >= 0)) return 0u;
  if (t > 255) return 255u;
  return static_cast<uint32_t>(t);
}

// One pixel: sums, mean, rgba; returns its noise term (0 at one pass)
double pixel(uint32_t p, const double* c, double* sum, double* sumsq, double* mean, uint32_t* rgba) {
  const double passes = static_cast<double>(p);
  const double sq = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  for (int k = 0; k < 3; ++k) sum[k] = p == 1u ? c[k] : sum[k] + c[k];
  *sumsq = p == 1u ? sq : *sumsq + sq;
  double m[3];
  for (int k = 0; k < 3; ++k) m[k] = sum[k] / passes;
  if (mean)
    for (int k = 0; k < 3; ++k) mean[k] = m[k];
  if (rgba) *rgba = clamp8(m[0]) | (clamp8(m[1]) << 8) | (clamp8(m[2]) << 16) | 0xFF000000u;
  if (p == 1u) return 0.0;
  const double d = *sumsq - passes * ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  return d > 0.0 ? d : 0.0;
}

// The lanes' values summed as the kernel does: xor butterfly in each wave (every lane ends with the same value; lane 0's
// is a + b level by level), then the waves in order
double groupSum(std::vector<double> v) {
  double total = 0.0;
  for (size_t w = 0; w < v.size() / 64; ++w) {
    double* x = v.data() + 64 * w;
    for (int off = 32; off >= 1; off >>= 1) {
      double next[64];
      for (int l = 0; l < 64; ++l) next[l] = x[l] + x[l ^ off];
      std::copy(next, next + 64, x);
    }
    total = w == 0 ? x[0] : total + x[0];
  }
  return total;
}

}  // namespace adapt

extern "C" {

uint32_t adapt_block(uint32_t tile_w, uint32_t tile_h) { return adapt::block(tile_w, tile_h); }

// rtc_scene_adaptive_accumulate_device on host arrays (the same meaning, every array of the state required but mean,
// rgba and max_noise); the list's tiles are distinct and inside the tiling
void adapt_accumulate(uint32_t hsize, uint32_t vsize, uint32_t tile_w, uint32_t tile_h, uint32_t min_passes, uint32_t max_passes,
                      double threshold, const double* frame, const uint32_t* list, uint32_t n_list, double* sum, double* sumsq,
                      double* mean, uint32_t* rgba, uint32_t* tile_passes, double* tile_noise, uint32_t* active, uint32_t* n_active,
                      double* max_noise) {
  const uint32_t tiles_x = (hsize + tile_w - 1u) / tile_w;
  const uint32_t n_tiles = tiles_x * ((vsize + tile_h - 1u) / tile_h);
  const uint32_t half = (tile_w + 1u) / 2u, items = tile_h * half, B = adapt::block(tile_w, tile_h);
  for (uint32_t k = 0; k < n_list; ++k) {
    const uint32_t t = list[k];
    const uint32_t x0 = (t % tiles_x) * tile_w, y0 = (t / tiles_x) * tile_h;
    const uint32_t w_in = std::min(tile_w, hsize - x0), h_in = std::min(tile_h, vsize - y0);
    const uint32_t p = tile_passes[t] + 1u;
    std::vector<double> lane(B, 0.0);
    for (uint32_t it = 0; it < items; ++it) {
      const uint32_t r = it / half, x = 2u * (it % half);
      if (r >= h_in || x >= w_in) continue;
      double d = 0.0;
      for (uint32_t e = 0; e < 2u; ++e) {
        if (x + e >= w_in) {
          d = d + 0.0;
          continue;
        }
        const size_t f = (static_cast<size_t>(k) * tile_h + r) * tile_w + x + e;
        const size_t i = static_cast<size_t>(y0 + r) * hsize + x0 + x + e;
        const double term = adapt::pixel(p, frame + 3 * f, sum + 3 * i, sumsq + i, mean ? mean + 3 * i : nullptr, rgba ? rgba + i : nullptr);
        d = e == 0u ? term : d + term;
      }
      lane[it % B] += d;
    }
    const double total = adapt::groupSum(lane);
    const double passes = static_cast<double>(p);
    const double n_t = static_cast<double>(w_in) * static_cast<double>(h_in);
    tile_noise[t] = p >= 2u ? std::sqrt(total / n_t / (3.0 * (passes - 1.0) * passes)) : std::numeric_limits<double>::infinity();
    tile_passes[t] = p;
  }
  uint32_t n = 0;
  double most = 0.0;
  for (uint32_t t = 0; t < n_tiles; ++t) {
    if (tile_passes[t] < min_passes || (tile_passes[t] < max_passes && tile_noise[t] > threshold)) active[n++] = t;
    most = tile_noise[t] > most ? tile_noise[t] : most;
  }
  *n_active = n;
  if (max_noise) *max_noise = most;
}

}  // extern "C"
