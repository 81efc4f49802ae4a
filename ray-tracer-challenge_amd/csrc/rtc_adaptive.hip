// rtc_adaptive.hip — adaptive sampling's per-tile accumulation and stopping rule (rtc_scene_adaptive_*).
//
// A translation unit of its own, so that the render kernels' and the progressive accumulation's code objects do not change
// with it.  Three kernels:
//
//   rtc_adaptive_begin_kernel     every tile: passes 0, noise +inf, active; n_active = T (and max_noise = +inf).
//   rtc_adaptive_accum_kernel     one work-group per listed tile (WIDE / narrow): region k of the compact frame
//     [n][tile_h][tile_w][3] (as rtc_render_tile_list_device leaves it) into the image's sums at tile list[k]; pixels
//     outside the image are skipped.  P = tile_passes[t] + 1 (P == 1: overwrite, nothing read but the frame); sum, sumsq,
//     and optionally mean = sum / P and rgba = the clamp of mean, per pixel as rtc_accum.hip's accum_pixel.  The tile's
//     noise is reduced in a fixed order: the tile is cut into items of two horizontally adjacent pixels, item
//     i = row * ceil(tile_w / 2) + column pair; lane l of the B-lane work-group (B = adaptiveBlock(), a function of the
//     tile's shape alone) adds the terms of items l, l + B, l + 2B, ... in that order, an item's term being
//     d(left) + d(right) (0 for a pixel outside the image); then an xor butterfly in each wave (offsets 32, 16, ..., 1)
//     and the waves' totals in order.  noise_t = sqrt(total / n_t / (3 (P - 1) P)) for P >= 2, +inf for P == 1.
//     WIDE (tile_w and hsize even, every pointer 16-byte aligned, rgba 8): an item is one pair, three 16-byte accesses
//     per [n][3] array; otherwise one pixel at a time, 8-byte accesses, same items, same order, same bits.
//   rtc_adaptive_compact_kernel   one work-group of 1024 over all T tiles in strips of 1024: tile t stays active iff
//     P_t < min_passes, or P_t < max_passes and noise_t > threshold.  A ballot and the waves' counts in order give each
//     active tile its place: `active` holds them in ascending order, n_active their number; max_noise the largest
//     noise_t (a maximum: order-independent).
//
// Plain adds and one correctly rounded divide (-ffp-contract=off).  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtc_device.h"

#define RTC_ADAPTIVE_MAX_BLOCK 1024u
#define RTC_ADAPTIVE_COMPACT_BLOCK 1024u

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

struct AdaptArgs {
  const double* frame;  // [n_list][tile_h][tile_w][3]
  const uint32_t* list;  // [n_list]
  double* sum;
  double* sumsq;
  double* mean;
  uint32_t* rgba;
  uint32_t* tile_passes;
  double* tile_noise;
  uint32_t hsize, vsize, tile_w, tile_h, tiles_x, n_tiles;
};

// clamp() of color.zig:61-71, as rtc_accum.hip has it
__device__ __forceinline__ uint32_t clamp8(double channel) {
  const double t = round(channel * 255);
  if (!(t >= 0)) return 0u;
  if (t > 255) return 255u;
  return static_cast<uint32_t>(t);
}

__device__ __forceinline__ uint32_t rgba_of(const double m[3]) {
  return clamp8(m[0]) | (clamp8(m[1]) << 8) | (clamp8(m[2]) << 16) | 0xFF000000u;
}

// One pixel: rtc_accum.hip's accum_pixel to the operation
template <bool FIRST>
__device__ __forceinline__ double accum_pixel(double passes, const double c[3], const double sum_old[3], double sq_old, double sum_new[3],
                                              double& sq_new, double m[3]) {
  const double sq = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  for (int i = 0; i < 3; ++i) sum_new[i] = FIRST ? c[i] : sum_old[i] + c[i];
  sq_new = FIRST ? sq : sq_old + sq;
  for (int i = 0; i < 3; ++i) m[i] = sum_new[i] / passes;
  if (FIRST) return 0.0;
  const double d = sq_new - passes * ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  return d > 0.0 ? d : 0.0;
}

// One pixel at 8-byte accesses: frame pixel f, image pixel i
template <bool FIRST>
__device__ __forceinline__ double accum_one(const AdaptArgs& a, double passes, size_t f, size_t i) {
  double c[3], so[3] = {0.0, 0.0, 0.0}, sn[3], m[3], sq_old = 0.0, sq_new;
  for (int k = 0; k < 3; ++k) c[k] = __builtin_nontemporal_load(a.frame + 3 * f + k);  // (read once)
  if (!FIRST) {
    for (int k = 0; k < 3; ++k) so[k] = a.sum[3 * i + k];
    sq_old = a.sumsq[i];
  }
  const double d = accum_pixel<FIRST>(passes, c, so, sq_old, sn, sq_new, m);
  for (int k = 0; k < 3; ++k) a.sum[3 * i + k] = sn[k];
  a.sumsq[i] = sq_new;
  if (a.mean)
    for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(m[k], a.mean + 3 * i + k);  // (not read back)
  if (a.rgba) __builtin_nontemporal_store(rgba_of(m), a.rgba + i);
  return d;
}

// Two pixels at 16-byte accesses: frame pixels f, f + 1 and image pixels i, i + 1 (f and i even)
template <bool FIRST>
__device__ __forceinline__ double accum_pair(const AdaptArgs& a, double passes, size_t f, size_t i) {
  const d2* f2 = reinterpret_cast<const d2*>(a.frame) + 3 * (f / 2);
  const d2 fr[3] = {__builtin_nontemporal_load(f2), __builtin_nontemporal_load(f2 + 1), __builtin_nontemporal_load(f2 + 2)};
  const size_t q = i / 2;
  d2* s2 = reinterpret_cast<d2*>(a.sum) + 3 * q;
  d2 so2[3] = {d2{0.0, 0.0}, d2{0.0, 0.0}, d2{0.0, 0.0}};
  d2 sq2 = d2{0.0, 0.0};
  if (!FIRST) {
    so2[0] = s2[0], so2[1] = s2[1], so2[2] = s2[2];
    sq2 = reinterpret_cast<const d2*>(a.sumsq)[q];
  }
  // [r0 g0] [b0 r1] [g1 b1]
  const double c0[3] = {fr[0].x, fr[0].y, fr[1].x}, c1[3] = {fr[1].y, fr[2].x, fr[2].y};
  const double o0[3] = {so2[0].x, so2[0].y, so2[1].x}, o1[3] = {so2[1].y, so2[2].x, so2[2].y};
  double n0[3], n1[3], m0[3], m1[3], q0, q1;
  const double d0 = accum_pixel<FIRST>(passes, c0, o0, sq2.x, n0, q0, m0);
  const double d1 = accum_pixel<FIRST>(passes, c1, o1, sq2.y, n1, q1, m1);
  s2[0] = d2{n0[0], n0[1]};
  s2[1] = d2{n0[2], n1[0]};
  s2[2] = d2{n1[1], n1[2]};
  reinterpret_cast<d2*>(a.sumsq)[q] = d2{q0, q1};
  if (a.mean) {
    d2* m2 = reinterpret_cast<d2*>(a.mean) + 3 * q;
    __builtin_nontemporal_store(d2{m0[0], m0[1]}, m2);
    __builtin_nontemporal_store(d2{m0[2], m1[0]}, m2 + 1);
    __builtin_nontemporal_store(d2{m1[1], m1[2]}, m2 + 2);
  }
  if (a.rgba) __builtin_nontemporal_store(u2{rgba_of(m0), rgba_of(m1)}, reinterpret_cast<u2*>(a.rgba) + q);
  return d0 + d1;
}

// The work-group's sum of its lanes' values: xor butterfly in each wave, then the waves' totals in order.  Thread 0.
__device__ __forceinline__ double group_sum(double v) {
  __shared__ double wave_total[RTC_ADAPTIVE_MAX_BLOCK / 64];
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63u) == 0u) wave_total[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = wave_total[0];
  for (uint32_t w = 1; w < blockDim.x / 64u; ++w) total += wave_total[w];
  return total;
}

template <bool FIRST, bool WIDE>
__device__ __forceinline__ double tile_body(const AdaptArgs& a, double passes, uint32_t k, uint32_t x0, uint32_t y0, uint32_t w_in,
                                            uint32_t h_in) {
  const uint32_t half = (a.tile_w + 1u) / 2u;
  const uint32_t items = a.tile_h * half;
  double d = 0.0;  // this lane's noise terms, in item order
  for (uint32_t it = threadIdx.x; it < items; it += blockDim.x) {
    const uint32_t r = it / half, x = 2u * (it % half);
    if (r >= h_in || x >= w_in) continue;
    const size_t f = (static_cast<size_t>(k) * a.tile_h + r) * a.tile_w + x;
    const size_t i = static_cast<size_t>(y0 + r) * a.hsize + (x0 + x);
    if (WIDE) {
      d += accum_pair<FIRST>(a, passes, f, i);  // (w_in is even: both pixels are in the image)
    } else {
      double t = accum_one<FIRST>(a, passes, f, i);
      t += x + 1u < w_in ? accum_one<FIRST>(a, passes, f + 1, i + 1) : 0.0;
      d += t;
    }
  }
  return group_sum(d);
}

template <bool WIDE>
__device__ __forceinline__ void accum_tile(const AdaptArgs& a) {
  const uint32_t k = blockIdx.x;
  const uint32_t t = a.list[k];
  if (t >= a.n_tiles) return;  // (the whole work-group: a tile outside the tiling is not written)
  const uint32_t x0 = (t % a.tiles_x) * a.tile_w, y0 = (t / a.tiles_x) * a.tile_h;
  const uint32_t w_in = min(a.tile_w, a.hsize - x0), h_in = min(a.tile_h, a.vsize - y0);
  const uint32_t p = a.tile_passes[t] + 1u;
  const double passes = static_cast<double>(p);
  const double total = p == 1u ? tile_body<true, WIDE>(a, passes, k, x0, y0, w_in, h_in) : tile_body<false, WIDE>(a, passes, k, x0, y0, w_in, h_in);
  if (threadIdx.x == 0u) {
    const double n_t = static_cast<double>(w_in) * static_cast<double>(h_in);
    a.tile_noise[t] = p >= 2u ? __builtin_sqrt(total / n_t / (3.0 * (passes - 1.0) * passes)) : __builtin_inf();
    a.tile_passes[t] = p;
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256)
rtc_adaptive_begin_kernel(uint32_t* __restrict__ tile_passes, double* __restrict__ tile_noise, uint32_t* __restrict__ active,
                          uint32_t* __restrict__ n_active, double* __restrict__ max_noise, const uint32_t n_tiles) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_tiles; t += gridDim.x * blockDim.x) {
    tile_passes[t] = 0u;
    tile_noise[t] = __builtin_inf();
    active[t] = t;
  }
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    *n_active = n_tiles;
    if (max_noise) *max_noise = __builtin_inf();
  }
}

extern "C" __global__ void __launch_bounds__(RTC_ADAPTIVE_MAX_BLOCK) rtc_adaptive_accum_kernel(const AdaptArgs a) { accum_tile<true>(a); }
extern "C" __global__ void __launch_bounds__(RTC_ADAPTIVE_MAX_BLOCK) rtc_adaptive_accum_narrow_kernel(const AdaptArgs a) {
  accum_tile<false>(a);
}

extern "C" __global__ void __launch_bounds__(RTC_ADAPTIVE_COMPACT_BLOCK)
rtc_adaptive_compact_kernel(const uint32_t* __restrict__ tile_passes, const double* __restrict__ tile_noise, const uint32_t n_tiles,
                            const uint32_t min_passes, const uint32_t max_passes, const double threshold, uint32_t* __restrict__ active,
                            uint32_t* __restrict__ n_active, double* __restrict__ max_noise) {
  constexpr uint32_t n_waves = RTC_ADAPTIVE_COMPACT_BLOCK / 64u;
  __shared__ uint32_t wave_count[n_waves];
  __shared__ double wave_max[n_waves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t base_count = 0;  // active tiles of the strips before (the same in every lane)
  double most = 0.0;        // this lane's largest noise
  for (uint32_t base = 0; base < n_tiles; base += RTC_ADAPTIVE_COMPACT_BLOCK) {
    const uint32_t t = base + threadIdx.x;
    bool on = false;
    if (t < n_tiles) {
      const uint32_t p = tile_passes[t];
      const double noise = tile_noise[t];
      on = p < min_passes || (p < max_passes && noise > threshold);
      most = noise > most ? noise : most;
    }
    const uint64_t mask = __ballot(on);
    const uint32_t below = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0u) wave_count[wave] = __popcll(mask);
    __syncthreads();
    uint32_t offset = base_count, strip = 0;
    for (uint32_t w = 0; w < n_waves; ++w) {
      const uint32_t c = wave_count[w];
      if (w < wave) offset += c;
      strip += c;
    }
    if (on) active[offset + below] = t;
    base_count += strip;
    __syncthreads();  // (wave_count is rewritten by the next strip)
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(most, off, 64);
    most = o > most ? o : most;
  }
  if (lane == 0u) wave_max[wave] = most;
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (uint32_t w = 1; w < n_waves; ++w) most = wave_max[w] > most ? wave_max[w] : most;
    *n_active = base_count;
    if (max_noise) *max_noise = most;
  }
}

// ---- the host side (rtc_capi.hip calls it after validating the arguments and ordering the stream)
// Lanes of the accumulation's work-group for a tile shape: its items (pixel pairs) rounded up to whole waves, at most 1024.
uint32_t rtcAdaptiveBlock(uint32_t tile_w, uint32_t tile_h) {
  const uint64_t items = static_cast<uint64_t>(tile_h) * ((tile_w + 1u) / 2u);
  const uint64_t b = (items + 63u) / 64u * 64u;
  return static_cast<uint32_t>(b < RTC_ADAPTIVE_MAX_BLOCK ? b : RTC_ADAPTIVE_MAX_BLOCK);
}

hipError_t rtcAdaptiveBeginLaunch(uint32_t n_tiles, uint32_t* tile_passes, double* tile_noise, uint32_t* active, uint32_t* n_active,
                                  double* max_noise, hipStream_t stream) {
  const uint32_t blocks = (n_tiles + 255u) / 256u;
  hipLaunchKernelGGL(rtc_adaptive_begin_kernel, dim3(blocks < 1024u ? blocks : 1024u), dim3(256), 0, stream, tile_passes, tile_noise,
                     active, n_active, max_noise, n_tiles);
  return hipGetLastError();
}

hipError_t rtcAdaptiveAccumLaunch(const double* frame, const uint32_t* list, uint32_t n_list, uint32_t hsize, uint32_t vsize,
                                  uint32_t tile_w, uint32_t tile_h, uint32_t min_passes, uint32_t max_passes, double threshold,
                                  double* sum, double* sumsq, double* mean, uint32_t* rgba, uint32_t* tile_passes, double* tile_noise,
                                  uint32_t* active, uint32_t* n_active, double* max_noise, hipStream_t stream) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; };
  const bool wide = (tile_w % 2u) == 0u && (hsize % 2u) == 0u && a16(frame) && a16(sum) && a16(sumsq) && (!mean || a16(mean)) &&
                    (!rgba || (reinterpret_cast<uintptr_t>(rgba) & 7u) == 0u);
  const uint32_t tiles_x = (hsize + tile_w - 1u) / tile_w;
  const uint32_t n_tiles = tiles_x * ((vsize + tile_h - 1u) / tile_h);
  const AdaptArgs a{frame, list, sum, sumsq, mean, rgba, tile_passes, tile_noise, hsize, vsize, tile_w, tile_h, tiles_x, n_tiles};
  const uint32_t block = rtcAdaptiveBlock(tile_w, tile_h);
  if (n_list > 0u) {
    if (wide) hipLaunchKernelGGL(rtc_adaptive_accum_kernel, dim3(n_list), dim3(block), 0, stream, a);
    else hipLaunchKernelGGL(rtc_adaptive_accum_narrow_kernel, dim3(n_list), dim3(block), 0, stream, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rtc_adaptive_compact_kernel, dim3(1), dim3(RTC_ADAPTIVE_COMPACT_BLOCK), 0, stream,
                     static_cast<const uint32_t*>(tile_passes), static_cast<const double*>(tile_noise), n_tiles, min_passes, max_passes,
                     threshold, active, n_active, max_noise);
  return hipGetLastError();
}
