// rtc_denoise.hip — the denoiser (rtc_denoise_device): variance-guided non-local means over an
// accumulated image, guided only by the mean and the sum of squares the accumulation keeps.  include/rtc.h states the
// operations; both kernels here add the same terms in the same order and give the same bits.
//
// A translation unit of its own, so that the render kernels' and the accumulations' code objects do not change with it.
//
//   rtc_denoise_kernel_p<F>   the tiled form, one kernel per patch size F = 0 .. 3.  One 256-thread work-group per 16 x 16 output tile.  The mean and the derived
//     variance of the tile and a halo of radius + patch are staged in LDS once (four planes: r, g, b, v; zeros outside the
//     image).  A term t / (eps + k2 (v(a) + v(b))) belongs to the pair (a, b = a + (dx, dy)), not to a patch: for one
//     search offset every pixel's patch sum is a box sum over the same pair image.  So per offset - the loop is uniform -
//     the work-group computes the term at the (16 + 2 patch)^2 positions a around the tile once, one division each, 0.0
//     where a or b is outside the image, into one of two LDS planes (one barrier per offset), and every thread adds its
//     (2 patch + 1)^2 window from LDS in the contract's oy, ox order.  A 0.0 added where the contract skips a pair does
//     not change a sum; n is the closed-form overlap count.  One exp per thread and offset.
//     Lanes: a half-wave (the 32 lanes one ds_read_b64 cycle serves) is 8 columns x 4 rows, of the output tile and of the
//     pair positions alike.  The pair planes' row stride is 24 doubles: rows 24 apart start 24, 16 and 8 double-banks on,
//     so the four 8-wide rows of a half-wave fall on all 32 double-banks once - the window reads, the bulk of the LDS
//     traffic, are conflict-free.  The staged planes' stride is the next value >= their width that is 8 mod 16, for the
//     same reason, where that fits in 64 KB (every setting but radius + patch = 13, which takes the width itself, 42).
//   rtc_denoise_naive_kernel  the literal form (option "denoise_naive"): one thread per pixel, the quadruple loop, global
//     loads, the variances formed again for every term.  The second implementation the tests hold the first to, and the
//     baseline its time is reported against.
//
// Plain IEEE operations (-ffp-contract=off); exp is the device library's.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtc.h"

#define RTC_DENOISE_TILE 16
#define RTC_DENOISE_PAIR_STRIDE 24
// (grid-stride above this many work-groups: a 1080p image has 8160 tiles)
#define RTC_DENOISE_MAX_BLOCKS 1048576u

namespace {

struct DenoiseArgs {
  const double* mean;
  const double* sumsq;
  const uint32_t* tile_passes;  // or nullptr: `passes` everywhere
  double* out;
  uint32_t* rgba;  // or nullptr
  uint32_t hsize, vsize, passes, tile_w, tile_h, tiles_x;
  uint32_t radius, patch;
  double k2, c3;
  uint32_t blocks_x;      // 16 x 16 output tiles per row
  uint32_t stage_stride;  // doubles between rows of a staged plane
  uint64_t n_blocks;      // output tiles
};

constexpr int kMaxHalo = static_cast<int>(RTC_DENOISE_MAX_RADIUS + RTC_DENOISE_MAX_PATCH);
constexpr int kMaxStage = RTC_DENOISE_TILE + 2 * kMaxHalo;
constexpr int kMaxPair = RTC_DENOISE_TILE + 2 * static_cast<int>(RTC_DENOISE_MAX_PATCH);
constexpr size_t kLdsLimit = 65536;

// Doubles of LDS for a setting: four staged planes, two pair planes
constexpr size_t ldsDoubles(int stage_width, int stage_stride, int pair_width) {
  return 4u * static_cast<size_t>(stage_width) * stage_stride + 2u * static_cast<size_t>(pair_width) * RTC_DENOISE_PAIR_STRIDE;
}
static_assert(kMaxPair + 2 <= RTC_DENOISE_PAIR_STRIDE, "a pair plane's row and two spare columns fit its stride");
static_assert(ldsDoubles(kMaxStage, kMaxStage, kMaxPair) * sizeof(double) <= kLdsLimit,
              "the staged tile and the pair planes of the largest setting fit in 64 KB of LDS");

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

// P(x, y)
__device__ __forceinline__ uint32_t passes_at(const DenoiseArgs& a, uint32_t x, uint32_t y) {
  return a.tile_passes ? a.tile_passes[static_cast<size_t>(y / a.tile_h) * a.tiles_x + x / a.tile_w] : a.passes;
}

// v(x, y): the term of rtc_accum.hip's accum_pixel over 3 (P - 1) P
__device__ __forceinline__ double variance_of(double s, double r, double g, double b, uint32_t p) {
  if (p < 2u) return 0.0;
  const double passes = static_cast<double>(p);
  const double d = s - passes * ((r * r + g * g) + b * b);
  return (d > 0.0 ? d : 0.0) / (3.0 * ((passes - 1.0) * passes));
}

// t / (eps + k2 (v(a) + v(b)))
__device__ __forceinline__ double pair_term(const double ua[3], double va, const double ub[3], double vb, double k2, double c3) {
  const double dr = ua[0] - ub[0], dg = ua[1] - ub[1], db = ua[2] - ub[2];
  const double vmin = vb < va ? vb : va;
  const double t = ((dr * dr + dg * dg) + db * db) - c3 * (va + vmin);
  return t / (RTC_DENOISE_EPS + k2 * (va + vb));
}

// exp(-max(0, S / (3 n)))
__device__ __forceinline__ double weight_of(double S, int n) {
  const double q = S / (3.0 * static_cast<double>(n));
  return exp(-(q > 0.0 ? q : 0.0));
}

// The displacements d that keep coordinate c + d inside [0, size), cut to -64 .. 64 (every displacement here is smaller)
__device__ __forceinline__ void reach(int64_t c, uint32_t size, int& lo, int& hi) {
  const int64_t l = -c, h = static_cast<int64_t>(size) - 1 - c;
  lo = static_cast<int>(l < -64 ? -64 : (l > 64 ? 64 : l));
  hi = static_cast<int>(h > 64 ? 64 : (h < -64 ? -64 : h));
}

// The o in -F .. F with c + o and c + d + o both inside, for a c whose reach is lo .. hi (c and c + d inside: >= 1)
__device__ __forceinline__ int overlap(int lo, int hi, int d, int F) {
  const int first = max(-F, max(lo, lo - d)), last = min(F, min(hi, hi - d));
  return last - first + 1;
}

template <int F>
__device__ __forceinline__ void denoise_tile(const DenoiseArgs& a, double* __restrict__ lds, uint64_t tile) {
  constexpr int T = RTC_DENOISE_TILE, PS = RTC_DENOISE_PAIR_STRIDE;
  constexpr int WP = T + 2 * F;                               // pair positions per row
  constexpr int BC = (WP + 7) / 8, BR = (WP + 3) / 4;         // 8 x 4 blocks of pair positions
  constexpr int ROUNDS = (BC * BR * 32 + 255) / 256;          // positions per thread
  const int t = static_cast<int>(threadIdx.x);
  const int R = static_cast<int>(a.radius), H = R + F, WS = T + 2 * H, SS = static_cast<int>(a.stage_stride);
  const int64_t x0 = static_cast<int64_t>(tile % a.blocks_x) * T, y0 = static_cast<int64_t>(tile / a.blocks_x) * T;
  double* const ur = lds;
  double* const ug = ur + WS * SS;
  double* const ub = ug + WS * SS;
  double* const vv = ub + WS * SS;
  double* const pair = vv + WS * SS;

  // the tile and its halo: u and the derived v, zeros outside the image
  for (int i = t; i < WS * WS; i += 256) {
    const int sy = i / WS, sx = i - sy * WS;
    const int64_t x = x0 - H + sx, y = y0 - H + sy;
    double r = 0.0, g = 0.0, b = 0.0, v = 0.0;
    if (x >= 0 && x < static_cast<int64_t>(a.hsize) && y >= 0 && y < static_cast<int64_t>(a.vsize)) {
      const size_t p = static_cast<size_t>(y) * a.hsize + static_cast<size_t>(x);
      r = a.mean[3 * p], g = a.mean[3 * p + 1], b = a.mean[3 * p + 2];
      v = variance_of(a.sumsq[p], r, g, b, passes_at(a, static_cast<uint32_t>(x), static_cast<uint32_t>(y)));
    }
    const int o = sy * SS + sx;
    ur[o] = r, ug[o] = g, ub[o] = b, vv[o] = v;
  }
  __syncthreads();

  // this thread's output pixel: half-wave h is columns 8 (h & 1) .., rows 4 (h >> 1) ..
  const int half = t >> 5, lane = t & 31;
  const int tx = (half & 1) * 8 + (lane & 7), ty = (half >> 1) * 4 + (lane >> 3);
  const int64_t px = x0 + tx, py = y0 + ty;
  int qx_lo, qx_hi, qy_lo, qy_hi;
  reach(px, a.hsize, qx_lo, qx_hi);
  reach(py, a.vsize, qy_lo, qy_hi);
  if (px >= static_cast<int64_t>(a.hsize) || py >= static_cast<int64_t>(a.vsize)) qx_lo = 1, qx_hi = 0;  // (a thread beyond the image: no q)

  // this thread's pair positions a (the same 8 x 4 blocks over the WP x WP positions), with u(a) and v(a) in registers
  // (a position beyond the WP x WP square, or outside the image, gets an empty reach: its term is 0.0 at every offset; the
  // former writes to the spare columns of the plane's first row, which no window reads)
  int stage_at[ROUNDS], pair_at[ROUNDS], bx_lo[ROUNDS], bx_hi[ROUNDS], by_lo[ROUNDS], by_hi[ROUNDS];
  double ua[ROUNDS][3], va[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int i = t + 256 * r, blk = i >> 5, l = i & 31;
    const int ax = (blk % BC) * 8 + (l & 7), ay = (blk / BC) * 4 + (l >> 3);
    const bool on = ax < WP && ay < WP;
    const int64_t x = x0 - F + ax, y = y0 - F + ay;
    reach(x, a.hsize, bx_lo[r], bx_hi[r]);
    reach(y, a.vsize, by_lo[r], by_hi[r]);
    if (!on || x < 0 || x >= static_cast<int64_t>(a.hsize) || y < 0 || y >= static_cast<int64_t>(a.vsize)) bx_lo[r] = 1, bx_hi[r] = 0;
    stage_at[r] = on ? (R + ay) * SS + (R + ax) : R * SS + R;
    pair_at[r] = on ? ay * PS + ax : WP + (l & 1);
    ua[r][0] = ur[stage_at[r]], ua[r][1] = ug[stage_at[r]], ua[r][2] = ub[stage_at[r]], va[r] = vv[stage_at[r]];
  }

  double W = 0.0, A[3] = {0.0, 0.0, 0.0};
  // the offsets with a q of the tile in the image (uniform): every other one is skipped whole
  int ty_lo, ty_hi, tx_lo, tx_hi;
  reach(y0, a.vsize, ty_lo, ty_hi);
  reach(x0, a.hsize, tx_lo, tx_hi);
  const int dy_first = max(-R, ty_lo - (T - 1)), dy_last = min(R, ty_hi), dx_first = max(-R, tx_lo - (T - 1)), dx_last = min(R, tx_hi);
  int k = 0;  // offsets done: the pair plane in use alternates
  for (int dy = dy_first; dy <= dy_last; ++dy) {
    for (int dx = dx_first; dx <= dx_last; ++dx) {
      double* const plane = pair + (k & 1) * (WP * PS);
      ++k;
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        double term = 0.0;
        if (dx >= bx_lo[r] && dx <= bx_hi[r] && dy >= by_lo[r] && dy <= by_hi[r]) {
          const int sb = stage_at[r] + dy * SS + dx;
          const double ubv[3] = {ur[sb], ug[sb], ub[sb]};
          term = pair_term(ua[r], va[r], ubv, vv[sb], a.k2, a.c3);
        }
        plane[pair_at[r]] = term;
      }
      // (one barrier per offset: the plane written two offsets on was last read before the barrier of the offset between)
      __syncthreads();
      if (dx >= qx_lo && dx <= qx_hi && dy >= qy_lo && dy <= qy_hi) {
        double S = 0.0;
#pragma unroll
        for (int oy = 0; oy <= 2 * F; ++oy)
#pragma unroll
          for (int ox = 0; ox <= 2 * F; ++ox) S += plane[(ty + oy) * PS + (tx + ox)];
        const int n = overlap(qx_lo, qx_hi, dx, F) * overlap(qy_lo, qy_hi, dy, F);
        const double w = weight_of(S, n);
        const int sq = (H + ty + dy) * SS + (H + tx + dx);
        W += w;
        A[0] += w * ur[sq], A[1] += w * ug[sq], A[2] += w * ub[sq];
      }
    }
  }
  if (qx_lo <= qx_hi) {  // (in the image)
    const size_t p = static_cast<size_t>(py) * a.hsize + static_cast<size_t>(px);
    const double o[3] = {A[0] / W, A[1] / W, A[2] / W};
    for (int c = 0; c < 3; ++c) a.out[3 * p + c] = o[c];
    if (a.rgba) a.rgba[p] = rgba_of(o);
  }
}

}  // namespace

// One kernel per patch size, so that the window sum unrolls and each has the registers of its own size only
template <int F>
__device__ __forceinline__ void denoise_tiles(const DenoiseArgs& a) {
  extern __shared__ double denoise_lds[];
  for (uint64_t tile = blockIdx.x; tile < a.n_blocks; tile += gridDim.x) {
    denoise_tile<F>(a, denoise_lds, tile);
    __syncthreads();  // (the next tile is staged over this one)
  }
}
extern "C" __global__ void __launch_bounds__(256) rtc_denoise_kernel_p0(const DenoiseArgs a) { denoise_tiles<0>(a); }
extern "C" __global__ void __launch_bounds__(256) rtc_denoise_kernel_p1(const DenoiseArgs a) { denoise_tiles<1>(a); }
extern "C" __global__ void __launch_bounds__(256) rtc_denoise_kernel_p2(const DenoiseArgs a) { denoise_tiles<2>(a); }
extern "C" __global__ void __launch_bounds__(256) rtc_denoise_kernel_p3(const DenoiseArgs a) { denoise_tiles<3>(a); }

extern "C" __global__ void __launch_bounds__(256) rtc_denoise_naive_kernel(const DenoiseArgs a) {
  const size_t n_pixels = static_cast<size_t>(a.hsize) * a.vsize;
  const int64_t w = a.hsize, h = a.vsize;
  const int R = static_cast<int>(a.radius), F = static_cast<int>(a.patch);
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_pixels; i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const int64_t px = static_cast<int64_t>(i % a.hsize), py = static_cast<int64_t>(i / a.hsize);
    double W = 0.0, A[3] = {0.0, 0.0, 0.0};
    for (int dy = -R; dy <= R; ++dy) {
      const int64_t qy = py + dy;
      if (qy < 0 || qy >= h) continue;
      for (int dx = -R; dx <= R; ++dx) {
        const int64_t qx = px + dx;
        if (qx < 0 || qx >= w) continue;
        double S = 0.0;
        int n = 0;
        for (int oy = -F; oy <= F; ++oy) {
          const int64_t ay = py + oy, by = qy + oy;
          if (ay < 0 || ay >= h || by < 0 || by >= h) continue;
          for (int ox = -F; ox <= F; ++ox) {
            const int64_t ax = px + ox, bx = qx + ox;
            if (ax < 0 || ax >= w || bx < 0 || bx >= w) continue;
            const size_t ia = static_cast<size_t>(ay) * a.hsize + static_cast<size_t>(ax);
            const size_t ib = static_cast<size_t>(by) * a.hsize + static_cast<size_t>(bx);
            const double ua[3] = {a.mean[3 * ia], a.mean[3 * ia + 1], a.mean[3 * ia + 2]};
            const double ub[3] = {a.mean[3 * ib], a.mean[3 * ib + 1], a.mean[3 * ib + 2]};
            const double va = variance_of(a.sumsq[ia], ua[0], ua[1], ua[2], passes_at(a, static_cast<uint32_t>(ax), static_cast<uint32_t>(ay)));
            const double vb = variance_of(a.sumsq[ib], ub[0], ub[1], ub[2], passes_at(a, static_cast<uint32_t>(bx), static_cast<uint32_t>(by)));
            S += pair_term(ua, va, ub, vb, a.k2, a.c3);
            ++n;
          }
        }
        const double wq = weight_of(S, n);
        const size_t iq = static_cast<size_t>(qy) * a.hsize + static_cast<size_t>(qx);
        W += wq;
        for (int c = 0; c < 3; ++c) A[c] += wq * a.mean[3 * iq + c];
      }
    }
    const double o[3] = {A[0] / W, A[1] / W, A[2] / W};
    for (int c = 0; c < 3; ++c) a.out[3 * i + c] = o[c];
    if (a.rgba) a.rgba[i] = rgba_of(o);
  }
}

// ---- the host side (rtc_capi.hip calls it after validating the arguments)
void rtcDenoiseTile(uint32_t* w, uint32_t* h) { *w = RTC_DENOISE_TILE, *h = RTC_DENOISE_TILE; }

// The staged planes' row stride for a setting: the next value >= the width that is 8 mod 16, where the planes then fit
static uint32_t denoiseStageStride(uint32_t radius, uint32_t patch) {
  const int width = RTC_DENOISE_TILE + 2 * static_cast<int>(radius + patch), pair_width = RTC_DENOISE_TILE + 2 * static_cast<int>(patch);
  const int padded = (width + 7) / 16 * 16 + 8;
  return static_cast<uint32_t>(ldsDoubles(width, padded, pair_width) * sizeof(double) <= kLdsLimit ? padded : width);
}

hipError_t rtcDenoiseLaunch(const rtc_denoise* d, bool naive, hipStream_t stream) {
  DenoiseArgs a{};
  a.mean = d->mean, a.sumsq = d->sumsq, a.tile_passes = d->tile_passes, a.out = d->out, a.rgba = d->rgba;
  a.hsize = d->hsize, a.vsize = d->vsize, a.passes = d->passes;
  a.tile_w = d->tile_passes ? d->tile_w : 1u, a.tile_h = d->tile_passes ? d->tile_h : 1u;
  a.tiles_x = d->tile_passes ? (d->hsize + d->tile_w - 1u) / d->tile_w : 0u;
  a.radius = d->setting.radius, a.patch = d->setting.patch;
  a.k2 = d->setting.strength * d->setting.strength, a.c3 = 3.0 * d->setting.cancel;
  a.blocks_x = (d->hsize + RTC_DENOISE_TILE - 1u) / RTC_DENOISE_TILE;
  a.n_blocks = static_cast<uint64_t>(a.blocks_x) * ((d->vsize + RTC_DENOISE_TILE - 1u) / RTC_DENOISE_TILE);
  a.stage_stride = denoiseStageStride(a.radius, a.patch);
  if (naive) {
    const uint64_t blocks = (static_cast<uint64_t>(d->hsize) * d->vsize + 255u) / 256u;
    hipLaunchKernelGGL(rtc_denoise_naive_kernel, dim3(static_cast<uint32_t>(blocks < RTC_DENOISE_MAX_BLOCKS ? blocks : RTC_DENOISE_MAX_BLOCKS)),
                       dim3(256), 0, stream, a);
  } else {
    const int width = RTC_DENOISE_TILE + 2 * static_cast<int>(a.radius + a.patch), pair_width = RTC_DENOISE_TILE + 2 * static_cast<int>(a.patch);
    const size_t lds = ldsDoubles(width, static_cast<int>(a.stage_stride), pair_width) * sizeof(double);
    void (*const kernels[4])(const DenoiseArgs) = {rtc_denoise_kernel_p0, rtc_denoise_kernel_p1, rtc_denoise_kernel_p2, rtc_denoise_kernel_p3};
    hipLaunchKernelGGL(kernels[a.patch], dim3(static_cast<uint32_t>(a.n_blocks < RTC_DENOISE_MAX_BLOCKS ? a.n_blocks : RTC_DENOISE_MAX_BLOCKS)),
                       dim3(256), lds, stream, a);
  }
  return hipGetLastError();
}
