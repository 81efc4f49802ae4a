// rtc_robust.hip — robust accumulation's resolve (rtc_robust_device): the Gini-weighted median of
// means of Buisine, Delepoulle and Renaud (2021) over M bucket sums [M][n][3] on the device, taken on luminance.
// include/rtc.h states the operations; the register form and the literal form here do the same operations in the same order
// and give the same bits.  No library function is involved.
//
// A translation unit of its own, so that the render kernels', the accumulations', the denoiser's and the film stage's code
// objects do not change with it.
//
//   rtc_robust_m<M>_kernel / rtc_robust_m<M>_narrow_kernel   M = 3, 5 .. 15: one instantiation of robust_body<M, WIDE> each.
//     The M bucket means, keys and ranks of a pixel are arrays that only fully unrolled loops index: they live in registers.
//     The rank of a bucket is counted over the M (M - 1) / 2 pairs of keys (one comparison a pair: keys are never NaN), so
//     there is no sort and no gather by rank; the kept sums are selects in bucket order.  `sums` is streamed once.
//     WIDE: sums, the bucket stride n * 24 B, mean_out and sumsq_out 16-byte aligned (8 for rejected_out and rgba) - a lane
//     takes a pair of pixels, 48 B a bucket as three 16-byte loads, as rtc_accum.hip; otherwise one pixel a lane, 8-byte
//     accesses.  Grid-stride over a grid whose size depends on n alone.
//   rtc_robust_naive_kernel   the literal form (option "robust_naive"): one thread a pixel, M a run-time value, the
//     contract's loops, every bucket mean formed again from `sums` wherever it is used.  The second implementation the tests
//     hold the first to, and the baseline its time is reported against.
//
// Plain IEEE operations (-ffp-contract=off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rtc.h"

// (the grid, as rtc_accum.hip's: a function of n alone)
#define RTC_ROBUST_MAX_BLOCKS 2048u

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

struct RobustArgs {
  const double* sums;
  double* mean;
  double* sumsq;       // or nullptr
  uint32_t* rejected;  // or nullptr
  uint32_t* rgba;      // or nullptr
  size_t n_pixels;
  uint32_t buckets;    // M (the literal form reads it; the register forms have it as a template argument)
  uint32_t more;       // passes % M: buckets below it hold one frame more
  double frames_lo, frames_hi;  // (double)(passes / M) and (double)(passes / M + 1)
  double passes;
  double gain;
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

// k_j of a bucket mean: its luminance, 0 where that is negative, +infinity where it is not finite
__device__ __forceinline__ double key_of(const double m[3]) {
  const double y = (0.2126 * m[0] + 0.7152 * m[1]) + 0.0722 * m[2];
  return (y - y == 0.0) ? (y > 0.0 ? y : 0.0) : INFINITY;
}

// G0 -> c (steps 3 and 4 of the contract, from T and A)
__device__ __forceinline__ uint32_t half_width(double T, double A, uint32_t M, double gain) {
  const uint32_t h = (M - 1u) / 2u;
  const double G0 = (T > 0.0 && T < INFINITY) ? (2.0 * A) / (static_cast<double>(M) * T) - static_cast<double>(M + 1u) / static_cast<double>(M)
                                               : (T > 0.0 ? 1.0 : 0.0);
  const double g = gain * G0;
  const double G = g > 0.0 ? (g < 1.0 ? g : 1.0) : 0.0;
  const uint32_t c = static_cast<uint32_t>(__builtin_floor((1.0 - G) * static_cast<double>(h) + 0.5));
  return c < h ? c : h;
}

// sumsq_out from the mean u and D (step 6)
__device__ __forceinline__ double sumsq_of(const RobustArgs& a, const double u[3], double D, uint32_t kv) {
  const double v = D / (3.0 * (static_cast<double>(kv - 1u) * static_cast<double>(kv)));
  const double P = a.passes;
  return P * ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + (3.0 * ((P - 1.0) * P)) * v;
}

// One pixel from its M bucket means in registers: the mean u, the sum of squares and the rejected count
template <int M>
__device__ __forceinline__ void resolve(const RobustArgs& a, const double (&m)[M][3], double u[3], double& sq, uint32_t& rejected) {
  constexpr uint32_t h = (M - 1) / 2;
  double k[M];
  uint32_t rank[M];
#pragma unroll
  for (int j = 0; j < M; ++j) k[j] = key_of(m[j]), rank[j] = 0u;
  // (i < j: bucket i is before j where k_i <= k_j, else j is before i - the contract's count, one comparison a pair)
#pragma unroll
  for (int j = 1; j < M; ++j) {
#pragma unroll
    for (int i = 0; i < j; ++i) {
      const bool before = k[i] <= k[j];
      rank[j] += before ? 1u : 0u;
      rank[i] += before ? 0u : 1u;
    }
  }
  double T = 0.0, A = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) T = T + k[j];
#pragma unroll
  for (int j = 0; j < M; ++j) A = A + static_cast<double>(rank[j] + 1u) * k[j];
  const uint32_t c = half_width(T, A, M, a.gain);
  const uint32_t kept = 2u * c + 1u;
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const bool keep = rank[j] >= h - c && rank[j] <= h + c;
    for (int ch = 0; ch < 3; ++ch) s[ch] = keep ? s[ch] + m[j][ch] : s[ch];
  }
  for (int ch = 0; ch < 3; ++ch) u[ch] = s[ch] / static_cast<double>(kept);
  rejected = static_cast<uint32_t>(M) - kept;
  const uint32_t cv = c > 1u ? c : 1u;
  double D = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const bool in = rank[j] >= h - cv && rank[j] <= h + cv;
    const double d[3] = {m[j][0] - u[0], m[j][1] - u[1], m[j][2] - u[2]};
    const double t = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    D = in ? D + t : D;
  }
  sq = sumsq_of(a, u, D, 2u * cv + 1u);
}

// The scalar form: pixel i alone
template <int M>
__device__ __forceinline__ void robust_one(const RobustArgs& a, size_t i) {
  double m[M][3];
  const double* p = a.sums + 3 * i;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    for (int ch = 0; ch < 3; ++ch) m[j][ch] = __builtin_nontemporal_load(p + ch);  // (read once)
    p += 3 * a.n_pixels;
  }
  // (every load is issued before the first quotient)
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double frames = static_cast<uint32_t>(j) < a.more ? a.frames_hi : a.frames_lo;
    for (int ch = 0; ch < 3; ++ch) m[j][ch] = m[j][ch] / frames;
  }
  double u[3], sq;
  uint32_t rejected;
  resolve<M>(a, m, u, sq, rejected);
  for (int ch = 0; ch < 3; ++ch) __builtin_nontemporal_store(u[ch], a.mean + 3 * i + ch);  // (not read back)
  if (a.sumsq) __builtin_nontemporal_store(sq, a.sumsq + i);
  if (a.rejected) __builtin_nontemporal_store(rejected, a.rejected + i);
  if (a.rgba) __builtin_nontemporal_store(rgba_of(u), a.rgba + i);
}

// The wide form: pixels 2q and 2q + 1 (n is even here), three 16-byte loads a bucket
template <int M>
__device__ __forceinline__ void robust_pair(const RobustArgs& a, size_t q) {
  double m0[M][3], m1[M][3];
  const d2* p = reinterpret_cast<const d2*>(a.sums) + 3 * q;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const d2 f[3] = {__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1), __builtin_nontemporal_load(p + 2)};
    // [r0 g0] [b0 r1] [g1 b1]
    m0[j][0] = f[0].x, m0[j][1] = f[0].y, m0[j][2] = f[1].x;
    m1[j][0] = f[1].y, m1[j][1] = f[2].x, m1[j][2] = f[2].y;
    p += 3 * (a.n_pixels / 2);
  }
  // (every load is issued before the first quotient, as robust_one)
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double frames = static_cast<uint32_t>(j) < a.more ? a.frames_hi : a.frames_lo;
    for (int ch = 0; ch < 3; ++ch) m0[j][ch] = m0[j][ch] / frames, m1[j][ch] = m1[j][ch] / frames;
  }
  double u0[3], u1[3], sq0, sq1;
  uint32_t r0, r1;
  resolve<M>(a, m0, u0, sq0, r0);
  resolve<M>(a, m1, u1, sq1, r1);
  d2* o2 = reinterpret_cast<d2*>(a.mean) + 3 * q;
  __builtin_nontemporal_store(d2{u0[0], u0[1]}, o2);
  __builtin_nontemporal_store(d2{u0[2], u1[0]}, o2 + 1);
  __builtin_nontemporal_store(d2{u1[1], u1[2]}, o2 + 2);
  if (a.sumsq) __builtin_nontemporal_store(d2{sq0, sq1}, reinterpret_cast<d2*>(a.sumsq) + q);
  if (a.rejected) __builtin_nontemporal_store(u2{r0, r1}, reinterpret_cast<u2*>(a.rejected) + q);
  if (a.rgba) __builtin_nontemporal_store(u2{rgba_of(u0), rgba_of(u1)}, reinterpret_cast<u2*>(a.rgba) + q);
}

template <int M, bool WIDE>
__device__ __forceinline__ void robust_body(const RobustArgs& a) {
  const size_t n_items = WIDE ? a.n_pixels / 2 : a.n_pixels;
  for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_items;
       t += static_cast<size_t>(gridDim.x) * blockDim.x) {
    if (WIDE) robust_pair<M>(a, t);
    else robust_one<M>(a, t);
  }
}

// ---- the literal form's pieces: everything from `sums` again
__device__ __forceinline__ void naive_mean(const RobustArgs& a, size_t i, uint32_t j, double m[3]) {
  const double frames = j < a.more ? a.frames_hi : a.frames_lo;
  for (int ch = 0; ch < 3; ++ch) m[ch] = a.sums[(static_cast<size_t>(j) * a.n_pixels + i) * 3 + ch] / frames;
}

__device__ __forceinline__ double naive_key(const RobustArgs& a, size_t i, uint32_t j) {
  double m[3];
  naive_mean(a, i, j, m);
  return key_of(m);
}

__device__ __forceinline__ uint32_t naive_rank(const RobustArgs& a, size_t i, uint32_t j) {
  const double kj = naive_key(a, i, j);
  uint32_t rank = 0u;
  for (uint32_t o = 0; o < a.buckets; ++o) {
    if (o == j) continue;
    const double ko = naive_key(a, i, o);
    if (ko < kj || (ko == kj && o < j)) ++rank;
  }
  return rank;
}

}  // namespace

#define RTC_ROBUST_KERNELS(M)                                                                                                   \
  extern "C" __global__ void __launch_bounds__(256) rtc_robust_m##M##_kernel(const RobustArgs a) { robust_body<M, true>(a); }   \
  extern "C" __global__ void __launch_bounds__(256) rtc_robust_m##M##_narrow_kernel(const RobustArgs a) { robust_body<M, false>(a); }
RTC_ROBUST_KERNELS(3)
RTC_ROBUST_KERNELS(5)
RTC_ROBUST_KERNELS(7)
RTC_ROBUST_KERNELS(9)
RTC_ROBUST_KERNELS(11)
RTC_ROBUST_KERNELS(13)
RTC_ROBUST_KERNELS(15)
#undef RTC_ROBUST_KERNELS

extern "C" __global__ void __launch_bounds__(256) rtc_robust_naive_kernel(const RobustArgs a) {
  const uint32_t M = a.buckets, h = (M - 1u) / 2u;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n_pixels;
       i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    double T = 0.0, A = 0.0;
    for (uint32_t j = 0; j < M; ++j) T = T + naive_key(a, i, j);
    for (uint32_t j = 0; j < M; ++j) A = A + static_cast<double>(naive_rank(a, i, j) + 1u) * naive_key(a, i, j);
    const uint32_t c = half_width(T, A, M, a.gain);
    const uint32_t kept = 2u * c + 1u;
    double s[3] = {0.0, 0.0, 0.0}, u[3];
    for (uint32_t j = 0; j < M; ++j) {
      const uint32_t rank = naive_rank(a, i, j);
      if (rank < h - c || rank > h + c) continue;
      double m[3];
      naive_mean(a, i, j, m);
      for (int ch = 0; ch < 3; ++ch) s[ch] = s[ch] + m[ch];
    }
    for (int ch = 0; ch < 3; ++ch) u[ch] = s[ch] / static_cast<double>(kept);
    const uint32_t cv = c > 1u ? c : 1u;
    double D = 0.0;
    for (uint32_t j = 0; j < M; ++j) {
      const uint32_t rank = naive_rank(a, i, j);
      if (rank < h - cv || rank > h + cv) continue;
      double m[3];
      naive_mean(a, i, j, m);
      const double d[3] = {m[0] - u[0], m[1] - u[1], m[2] - u[2]};
      D = D + ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    }
    for (int ch = 0; ch < 3; ++ch) a.mean[3 * i + ch] = u[ch];
    if (a.sumsq) a.sumsq[i] = sumsq_of(a, u, D, 2u * cv + 1u);
    if (a.rejected) a.rejected[i] = M - kept;
    if (a.rgba) a.rgba[i] = rgba_of(u);
  }
}

// ---- the host side (rtc_capi.hip calls it after validating the arguments)
void rtcRobustGrid(uint32_t* max_blocks, uint32_t* block) { *max_blocks = RTC_ROBUST_MAX_BLOCKS, *block = 256u; }

// Blocks of the grid: a function of the items alone
static uint32_t robustBlocks(size_t items) {
  const size_t b = (items + 255) / 256;
  return static_cast<uint32_t>(b < RTC_ROBUST_MAX_BLOCKS ? b : RTC_ROBUST_MAX_BLOCKS);
}

hipError_t rtcRobustLaunch(const rtc_robust* r, bool naive, hipStream_t stream) {
  const uint32_t M = r->setting.buckets;
  RobustArgs a{};
  a.sums = r->sums, a.mean = r->mean_out, a.sumsq = r->sumsq_out, a.rejected = r->rejected_out, a.rgba = r->rgba;
  a.n_pixels = r->n_pixels, a.buckets = M, a.more = r->passes % M;
  a.frames_lo = static_cast<double>(r->passes / M), a.frames_hi = static_cast<double>(r->passes / M + 1u);
  a.passes = static_cast<double>(r->passes), a.gain = r->setting.gain;
  if (naive) {
    hipLaunchKernelGGL(rtc_robust_naive_kernel, dim3(robustBlocks(a.n_pixels)), dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  auto aligned = [](const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1u)) == 0u; };
  // (an even n: every bucket of [M][n][3] then starts 16-byte aligned where the first does, and no pair is split)
  const bool wide = aligned(r->sums, 16u) && a.n_pixels % 2u == 0u && aligned(r->mean_out, 16u) &&
                    (!r->sumsq_out || aligned(r->sumsq_out, 16u)) && (!r->rejected_out || aligned(r->rejected_out, 8u)) &&
                    (!r->rgba || aligned(r->rgba, 8u));
  const dim3 grid(robustBlocks(wide ? a.n_pixels / 2u : a.n_pixels));
#define RTC_ROBUST_CASE(M)                                                                                  \
  case M:                                                                                                   \
    if (wide) hipLaunchKernelGGL(rtc_robust_m##M##_kernel, grid, dim3(256), 0, stream, a);                  \
    else hipLaunchKernelGGL(rtc_robust_m##M##_narrow_kernel, grid, dim3(256), 0, stream, a);                \
    break;
  switch (M) {
    RTC_ROBUST_CASE(3)
    RTC_ROBUST_CASE(5)
    RTC_ROBUST_CASE(7)
    RTC_ROBUST_CASE(9)
    RTC_ROBUST_CASE(11)
    RTC_ROBUST_CASE(13)
    RTC_ROBUST_CASE(15)
    default: return hipErrorInvalidValue;  // (rtc_robust_device has refused every other M)
  }
#undef RTC_ROBUST_CASE
  return hipGetLastError();
}
