// rtc_accum.hip — progressive rendering's accumulation (rtc_scene_accumulate_device).
//
// One streaming pass over memory per call: the pass just rendered (`frame`) and the old sums are read, the new sums and the
// optional outputs (mean, rgba, the noise partials) are written.  A translation unit of its own, so that the render
// kernels' code objects do not change with it.
//
//   rtc_accum_kernel / rtc_accum_first_kernel   (passes >= 2 / passes == 1: overwrite, nothing read but the frame)
//     WIDE: every pointer 16-byte aligned (8 for rgba) - a lane takes a pair of pixels, 48 B of [n][3] f64 as three
//     16-byte loads (global_load_dwordx4); otherwise one pixel a lane, 8-byte loads.  Grid-stride over a grid whose
//     size depends on n only, so that each block's noise partial covers the same pixels every time.
//   rtc_accum_noise_kernel   one block: the partials in a fixed order -> sqrt(total / n / (3 (P - 1) P)).
//
// Plain adds and one correctly rounded divide (-ffp-contract=off): after P calls `sum` is the in-order sum of the P frames
// to the bit, `mean` is sum / P, `rgba` is rtc_rgba8_kernel's clamp of mean.  No floating-point atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtc_device.h"

// (a 1080p frame is 1.04 M pixel pairs: two per lane at this cap; 256 CUs hold 8 such blocks each)
#define RTC_ACCUM_MAX_BLOCKS 2048u

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

struct AccumArgs {
  const double* frame;
  double* sum;
  double* sumsq;
  double* mean;
  uint32_t* rgba;
  double* partials;  // [gridDim.x], or nullptr: no noise
  size_t n_pixels;
  double passes;
};

// clamp() of color.zig:61-71, as rtc_rgba8_kernel (rtc_kernels.hip) has it: @round of channel * 255, clamped to 0..255
__device__ __forceinline__ uint32_t clamp8(double channel) {
  const double t = round(channel * 255);
  if (!(t >= 0)) return 0u;
  if (t > 255) return 255u;
  return static_cast<uint32_t>(t);
}

// One pixel: the new sums from the old (FIRST: from nothing), and its outputs.  Returns its noise term.
template <bool FIRST>
__device__ __forceinline__ double accum_pixel(const AccumArgs& a, double c[3], double sum_old[3], double sq_old, double sum_new[3],
                                              double& sq_new, double m[3]) {
  const double sq = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  for (int i = 0; i < 3; ++i) sum_new[i] = FIRST ? c[i] : sum_old[i] + c[i];
  sq_new = FIRST ? sq : sq_old + sq;
  for (int i = 0; i < 3; ++i) m[i] = sum_new[i] / a.passes;
  if (FIRST) return 0.0;
  const double d = sq_new - a.passes * ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  return d > 0.0 ? d : 0.0;
}

__device__ __forceinline__ uint32_t rgba_of(const double m[3]) {
  return clamp8(m[0]) | (clamp8(m[1]) << 8) | (clamp8(m[2]) << 16) | 0xFF000000u;
}

// The scalar form: pixel i alone (the odd last pixel of the wide form, every pixel of the other)
template <bool FIRST>
__device__ __forceinline__ double accum_one(const AccumArgs& a, size_t i) {
  double c[3], so[3] = {0.0, 0.0, 0.0}, sn[3], m[3], sq_old = 0.0, sq_new;
  for (int k = 0; k < 3; ++k) c[k] = __builtin_nontemporal_load(a.frame + 3 * i + k);  // (read once)
  if (!FIRST) {
    for (int k = 0; k < 3; ++k) so[k] = a.sum[3 * i + k];
    if (a.sumsq) sq_old = a.sumsq[i];
  }
  const double d = accum_pixel<FIRST>(a, c, so, sq_old, sn, sq_new, m);
  for (int k = 0; k < 3; ++k) a.sum[3 * i + k] = sn[k];
  if (a.sumsq) a.sumsq[i] = sq_new;
  if (a.mean)
    for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(m[k], a.mean + 3 * i + k);  // (not read back)
  if (a.rgba) __builtin_nontemporal_store(rgba_of(m), a.rgba + i);
  return d;
}

// The wide form: pixels 2q and 2q + 1, three 16-byte accesses per [n][3] array
template <bool FIRST>
__device__ __forceinline__ double accum_pair(const AccumArgs& a, size_t q) {
  const d2* f2 = reinterpret_cast<const d2*>(a.frame) + 3 * q;
  const d2 f[3] = {__builtin_nontemporal_load(f2), __builtin_nontemporal_load(f2 + 1), __builtin_nontemporal_load(f2 + 2)};
  d2* s2 = reinterpret_cast<d2*>(a.sum) + 3 * q;
  d2 so2[3] = {d2{0.0, 0.0}, d2{0.0, 0.0}, d2{0.0, 0.0}};
  d2 sq2 = d2{0.0, 0.0};
  if (!FIRST) {
    so2[0] = s2[0], so2[1] = s2[1], so2[2] = s2[2];
    if (a.sumsq) sq2 = reinterpret_cast<const d2*>(a.sumsq)[q];
  }
  // [r0 g0] [b0 r1] [g1 b1]
  double c0[3] = {f[0].x, f[0].y, f[1].x}, c1[3] = {f[1].y, f[2].x, f[2].y};
  double o0[3] = {so2[0].x, so2[0].y, so2[1].x}, o1[3] = {so2[1].y, so2[2].x, so2[2].y};
  double n0[3], n1[3], m0[3], m1[3], q0, q1;
  const double d = accum_pixel<FIRST>(a, c0, o0, sq2.x, n0, q0, m0) + accum_pixel<FIRST>(a, c1, o1, sq2.y, n1, q1, m1);
  s2[0] = d2{n0[0], n0[1]};
  s2[1] = d2{n0[2], n1[0]};
  s2[2] = d2{n1[1], n1[2]};
  if (a.sumsq) reinterpret_cast<d2*>(a.sumsq)[q] = d2{q0, q1};
  if (a.mean) {
    d2* m2 = reinterpret_cast<d2*>(a.mean) + 3 * q;
    __builtin_nontemporal_store(d2{m0[0], m0[1]}, m2);
    __builtin_nontemporal_store(d2{m0[2], m1[0]}, m2 + 1);
    __builtin_nontemporal_store(d2{m1[1], m1[2]}, m2 + 2);
  }
  if (a.rgba) __builtin_nontemporal_store(u2{rgba_of(m0), rgba_of(m1)}, reinterpret_cast<u2*>(a.rgba) + q);
  return d;
}

// A block's sum of its lanes' values in a fixed order (xor butterfly in each wave, then the waves in order): the same
// bits every time.  Valid in thread 0.
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double wave_total[4];
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63u) == 0u) wave_total[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_total[0] + wave_total[1]) + wave_total[2]) + wave_total[3];
}

template <bool FIRST, bool WIDE>
__device__ __forceinline__ void accum_body(const AccumArgs& a) {
  const size_t n_items = WIDE ? (a.n_pixels + 1) / 2 : a.n_pixels;
  double d = 0.0;  // this lane's noise terms, in item order
  for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_items;
       t += static_cast<size_t>(gridDim.x) * blockDim.x) {
    if (WIDE && 2 * t + 1 < a.n_pixels) d += accum_pair<FIRST>(a, t);
    else d += accum_one<FIRST>(a, WIDE ? 2 * t : t);
  }
  if (!FIRST && a.partials) {
    const double b = block_sum(d);
    if (threadIdx.x == 0u) a.partials[blockIdx.x] = b;
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) rtc_accum_kernel(const AccumArgs a) { accum_body<false, true>(a); }
extern "C" __global__ void __launch_bounds__(256) rtc_accum_narrow_kernel(const AccumArgs a) { accum_body<false, false>(a); }
extern "C" __global__ void __launch_bounds__(256) rtc_accum_first_kernel(const AccumArgs a) { accum_body<true, true>(a); }
extern "C" __global__ void __launch_bounds__(256) rtc_accum_first_narrow_kernel(const AccumArgs a) { accum_body<true, false>(a); }

// One block of 256: lane t sums partials t, t + 256, ... in order, then block_sum; thread 0 writes the estimate.
extern "C" __global__ void __launch_bounds__(256)
rtc_accum_noise_kernel(const double* __restrict__ partials, const uint32_t n_partials, const size_t n_pixels, const double passes,
                       double* __restrict__ noise) {
  double v = 0.0;
  for (uint32_t i = threadIdx.x; i < n_partials; i += blockDim.x) v += partials[i];
  const double total = block_sum(v);
  if (threadIdx.x == 0u) *noise = __builtin_sqrt(total / static_cast<double>(n_pixels) / (3.0 * (passes - 1.0) * passes));
}

// ---- the host side (rtc_capi.hip calls it after validating the arguments and ordering the stream)
// Blocks of the accumulation's grid: a function of n alone (the partials' cover does not depend on the device).
uint32_t rtcAccumBlocks(size_t n_pixels, bool wide) {
  const size_t items = wide ? (n_pixels + 1) / 2 : n_pixels;
  const size_t b = (items + 255) / 256;
  return static_cast<uint32_t>(b < RTC_ACCUM_MAX_BLOCKS ? b : RTC_ACCUM_MAX_BLOCKS);
}

hipError_t rtcAccumLaunch(const double* frame, size_t n_pixels, uint32_t passes, double* sum, double* sumsq, double* mean,
                          uint32_t* rgba, double* noise, double* partials, hipStream_t stream) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; };
  const bool wide = a16(frame) && a16(sum) && (!sumsq || a16(sumsq)) && (!mean || a16(mean)) &&
                    (!rgba || (reinterpret_cast<uintptr_t>(rgba) & 7u) == 0u);
  AccumArgs a{frame, sum, sumsq, mean, rgba, noise ? partials : nullptr, n_pixels, static_cast<double>(passes)};
  const uint32_t blocks = rtcAccumBlocks(n_pixels, wide);
  if (passes == 1u) {
    if (wide) hipLaunchKernelGGL(rtc_accum_first_kernel, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(rtc_accum_first_narrow_kernel, dim3(blocks), dim3(256), 0, stream, a);
  } else {
    if (wide) hipLaunchKernelGGL(rtc_accum_kernel, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(rtc_accum_narrow_kernel, dim3(blocks), dim3(256), 0, stream, a);
  }
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (noise) {
    hipLaunchKernelGGL(rtc_accum_noise_kernel, dim3(1), dim3(256), 0, stream, static_cast<const double*>(partials), blocks, n_pixels,
                       static_cast<double>(passes), noise);
    return hipGetLastError();
  }
  return hipSuccess;
}
