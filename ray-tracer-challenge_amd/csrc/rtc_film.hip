// rtc_film.hip — the film stage (rtc_film_device): exposure (manual, or from the image's log-average
// luminance), a bloom (a bright pass, blurred by a separable Gaussian and added back), a tone curve, a transfer function and
// the 8-bit clamp, over an image on the device.  include/rtc.h states the operations; the tiled and the literal kernels here
// add the same terms in the same order and give the same bits.
//
// A translation unit of its own, so that the render kernels', the accumulations' and the denoiser's code objects do not
// change with it.
//
//   rtc_film_log_kernel       (automatic exposure) grid-stride over a grid whose size depends on n alone, one pixel an item:
//     a lane adds log(eps + max(0, Y)) of its pixels in order, the block adds its lanes in a fixed order: one partial a block.
//   rtc_film_exposure_kernel  one block: the partials in a fixed order -> E = (exposure * key) / exp(T / n), to scratch and
//     to scale_out.  No floating-point atomics; the same bits on every run.
//   rtc_film_point_kernel / rtc_film_point_narrow_kernel   (no bloom) one streaming pass.  WIDE: `in` and `out` 16-byte
//     aligned (8 for rgba) - a lane takes a pair of pixels, 48 B of [n][3] f64 as three 16-byte accesses, as rtc_accum.hip;
//     otherwise one pixel a lane, 8-byte accesses.
//   rtc_film_row_kernel       (bloom) one work-group per 256 pixels of a row: x and the bright pass b once per pixel, a halo
//     of `radius` on both sides included, into three LDS planes (zeros outside the image); every thread adds its window in
//     the contract's order; H goes to scratch as three planes [3][vsize][hsize], so that the resolve kernel reads rows of it.
//   rtc_film_resolve_kernel   (bloom) one work-group per 32 x 32 output tile.  One plane of H at a time: 32 + 2 radius rows
//     of 32 doubles are staged in LDS (256-byte rows of global memory; zeros outside the image), a thread adds the column
//     windows of its 4 pixels (rows ty, ty + 8, ...) in the contract's order.  Then x(p) again from in(p), the combine, the
//     curve, the transfer and the clamp.
//     Lanes: a half-wave (the 32 lanes one ds_read_b64 cycle serves) is 32 consecutive columns of one row in both kernels, so
//     every window read and every staging write touches 32 consecutive doubles: all 32 double-banks once, no conflict.  The
//     weights g[] are read from the kernel's arguments by a uniform index (scalar loads), not from LDS.
//   rtc_film_naive_row_kernel / rtc_film_naive_resolve_kernel   the literal forms (option "film_naive"): one thread per pixel,
//     the contract's loops, global loads, no LDS.  The second implementation the tests hold the first to.
//
// Plain IEEE operations (-ffp-contract=off); exp, log and pow are the device library's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/rtc.h"

#define RTC_FILM_ROW_W 256
#define RTC_FILM_COL_W 32
#define RTC_FILM_COL_H 32
// (the streaming kernels' grid, as rtc_accum.hip's: a function of n alone)
#define RTC_FILM_MAX_BLOCKS 2048u
// (grid-stride above this many tiles: a 1080p image has 8640 row tiles)
#define RTC_FILM_MAX_TILE_BLOCKS 1048576u

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

struct FilmArgs {
  const double* in;
  double* out;
  uint32_t* rgba;      // or nullptr
  double* scale_out;   // or nullptr
  const double* e_dev; // automatic exposure: where rtc_film_exposure_kernel leaves E; nullptr: `exposure`
  double* h;           // bloom: H as planes [3][vsize][hsize]
  size_t n_pixels;
  uint32_t hsize, vsize;
  double exposure, threshold, intensity;
  double white2, hable_white, inv_power;  // white * white, f(white), 1 / 2.4 or 1 / gamma: formed on the host
  uint32_t curve, transfer, radius;
  uint32_t row_tiles_x, col_tiles_x;
  uint64_t row_tiles, col_tiles;
  double g[RTC_FILM_MAX_RADIUS + 1];
};

constexpr size_t kLdsLimit = 65536;
constexpr int kColThreadRows = 256 / RTC_FILM_COL_W;            // rows of threads in a resolve work-group
constexpr int kColPixels = RTC_FILM_COL_H / kColThreadRows;     // pixels per thread
// Doubles of LDS of the resolve kernel: one plane of the tile and its halo
constexpr size_t resolveLdsDoubles(uint32_t radius) { return static_cast<size_t>(RTC_FILM_COL_H + 2u * radius) * RTC_FILM_COL_W; }
static_assert(RTC_FILM_COL_W == 32 && RTC_FILM_COL_H % kColThreadRows == 0, "a half-wave is one row of the tile's columns");
static_assert(resolveLdsDoubles(RTC_FILM_MAX_RADIUS) * sizeof(double) <= kLdsLimit,
              "one plane of the resolve tile and its halo at the largest radius fits in 64 KB of LDS");
static_assert(3u * (RTC_FILM_ROW_W + 2u * RTC_FILM_MAX_RADIUS) * sizeof(double) <= kLdsLimit, "the row kernel's three planes fit in 64 KB of LDS");

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

__device__ __forceinline__ double luminance(const double c[3]) { return (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]; }

__device__ __forceinline__ double exposure_of(const FilmArgs& a) { return a.e_dev ? *a.e_dev : a.exposure; }

// b(p) of an exposed pixel x
__device__ __forceinline__ void bright_pass(const FilmArgs& a, const double x[3], double b[3]) {
  const double y = luminance(x);
  const double over = y - a.threshold;
  const double w = (over > 0.0 ? over : 0.0) / (y > RTC_FILM_EPS ? y : RTC_FILM_EPS);
  for (int k = 0; k < 3; ++k) b[k] = x[k] * w;
}

__device__ __forceinline__ double hable(double v) {
  return ((v * (0.15 * v + 0.05) + 0.004) / (v * (0.15 * v + 0.5) + 0.06)) - 0.02 / 0.3;
}

// The curve and the transfer of one channel (uniform branches: a setting without pow runs none)
__device__ __forceinline__ double develop(const FilmArgs& a, double c) {
  double t = c;
  if (a.curve == RTC_FILM_CURVE_REINHARD) t = (c * (1.0 + c / a.white2)) / (1.0 + c);
  else if (a.curve == RTC_FILM_CURVE_ACES) t = (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14);
  else if (a.curve == RTC_FILM_CURVE_HABLE) t = hable(c) / a.hable_white;
  if (a.transfer == RTC_FILM_TRANSFER_SRGB) return t <= 0.0031308 ? 12.92 * t : 1.055 * pow(t, a.inv_power) - 0.055;
  if (a.transfer == RTC_FILM_TRANSFER_GAMMA) return t > 0.0 ? pow(t, a.inv_power) : 0.0;
  return t;
}

// A block's sum of its lanes' values in a fixed order, as rtc_accum.hip's.  Valid in thread 0.
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double wave_total[4];
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63u) == 0u) wave_total[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_total[0] + wave_total[1]) + wave_total[2]) + wave_total[3];
}

// Pixel i without bloom
__device__ __forceinline__ void point_one(const FilmArgs& a, double E, size_t i) {
  double o[3];
  for (int k = 0; k < 3; ++k) o[k] = develop(a, E * __builtin_nontemporal_load(a.in + 3 * i + k));
  for (int k = 0; k < 3; ++k) __builtin_nontemporal_store(o[k], a.out + 3 * i + k);
  if (a.rgba) __builtin_nontemporal_store(rgba_of(o), a.rgba + i);
}

// Pixels 2q and 2q + 1 without bloom: three 16-byte accesses per image
__device__ __forceinline__ void point_pair(const FilmArgs& a, double E, size_t q) {
  const d2* f2 = reinterpret_cast<const d2*>(a.in) + 3 * q;
  const d2 f[3] = {__builtin_nontemporal_load(f2), __builtin_nontemporal_load(f2 + 1), __builtin_nontemporal_load(f2 + 2)};
  // [r0 g0] [b0 r1] [g1 b1]
  const double o0[3] = {develop(a, E * f[0].x), develop(a, E * f[0].y), develop(a, E * f[1].x)};
  const double o1[3] = {develop(a, E * f[1].y), develop(a, E * f[2].x), develop(a, E * f[2].y)};
  d2* o2 = reinterpret_cast<d2*>(a.out) + 3 * q;
  __builtin_nontemporal_store(d2{o0[0], o0[1]}, o2);
  __builtin_nontemporal_store(d2{o0[2], o1[0]}, o2 + 1);
  __builtin_nontemporal_store(d2{o1[1], o1[2]}, o2 + 2);
  if (a.rgba) __builtin_nontemporal_store(u2{rgba_of(o0), rgba_of(o1)}, reinterpret_cast<u2*>(a.rgba) + q);
}

template <bool WIDE>
__device__ __forceinline__ void point_body(const FilmArgs& a) {
  const double E = exposure_of(a);
  if (a.scale_out && !a.e_dev && blockIdx.x == 0u && threadIdx.x == 0u) *a.scale_out = E;
  const size_t n_items = WIDE ? (a.n_pixels + 1) / 2 : a.n_pixels;
  for (size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_items;
       t += static_cast<size_t>(gridDim.x) * blockDim.x) {
    if (WIDE && 2 * t + 1 < a.n_pixels) point_pair(a, E, t);
    else point_one(a, E, WIDE ? 2 * t : t);
  }
}

// Pixel p with its bloom B: the combine, the curve, the transfer and the clamp
__device__ __forceinline__ void resolve_pixel(const FilmArgs& a, double E, size_t p, const double B[3]) {
  double o[3];
  for (int k = 0; k < 3; ++k) o[k] = develop(a, E * a.in[3 * p + k] + a.intensity * B[k]);
  for (int k = 0; k < 3; ++k) a.out[3 * p + k] = o[k];
  if (a.rgba) a.rgba[p] = rgba_of(o);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256)
rtc_film_log_kernel(const double* __restrict__ in, const size_t n_pixels, double* __restrict__ partials) {
  double v = 0.0;  // this lane's terms, in pixel order
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_pixels; i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const double c[3] = {in[3 * i], in[3 * i + 1], in[3 * i + 2]};
    const double y = luminance(c);
    v += log(RTC_FILM_EPS + (y > 0.0 ? y : 0.0));
  }
  const double b = block_sum(v);
  if (threadIdx.x == 0u) partials[blockIdx.x] = b;
}

// One block of 256: lane t sums partials t, t + 256, ... in order, then block_sum; thread 0 writes E.
extern "C" __global__ void __launch_bounds__(256)
rtc_film_exposure_kernel(const double* __restrict__ partials, const uint32_t n_partials, const size_t n_pixels, const double scale,
                         double* __restrict__ e_dev, double* __restrict__ scale_out) {
  double v = 0.0;
  for (uint32_t i = threadIdx.x; i < n_partials; i += blockDim.x) v += partials[i];
  const double total = block_sum(v);
  if (threadIdx.x == 0u) {
    const double E = scale / exp(total / static_cast<double>(n_pixels));
    *e_dev = E;
    if (scale_out) *scale_out = E;
  }
}

extern "C" __global__ void __launch_bounds__(256) rtc_film_point_kernel(const FilmArgs a) { point_body<true>(a); }
extern "C" __global__ void __launch_bounds__(256) rtc_film_point_narrow_kernel(const FilmArgs a) { point_body<false>(a); }

extern "C" __global__ void __launch_bounds__(256) rtc_film_row_kernel(const FilmArgs a) {
  constexpr int W = RTC_FILM_ROW_W;
  __shared__ double plane[3][W + 2 * RTC_FILM_MAX_RADIUS];
  const double E = exposure_of(a);
  const int R = static_cast<int>(a.radius), t = static_cast<int>(threadIdx.x);
  for (uint64_t tile = blockIdx.x; tile < a.row_tiles; tile += gridDim.x) {
    const size_t row = static_cast<size_t>(tile / a.row_tiles_x) * a.hsize;
    const int64_t x0 = static_cast<int64_t>(tile % a.row_tiles_x) * W;
    // x and the bright pass, once per pixel of the tile and its halo; zeros outside the image
    for (int i = t; i < W + 2 * R; i += 256) {
      const int64_t x = x0 - R + i;
      double b[3] = {0.0, 0.0, 0.0};
      if (x >= 0 && x < static_cast<int64_t>(a.hsize)) {
        const size_t p = row + static_cast<size_t>(x);
        const double e[3] = {E * a.in[3 * p], E * a.in[3 * p + 1], E * a.in[3 * p + 2]};
        bright_pass(a, e, b);
      }
      plane[0][i] = b[0], plane[1][i] = b[1], plane[2][i] = b[2];
    }
    __syncthreads();
    if (x0 + t < static_cast<int64_t>(a.hsize)) {
      double s[3] = {0.0, 0.0, 0.0};
      for (int i = -R; i <= R; ++i) {
        const double g = a.g[i < 0 ? -i : i];
        for (int k = 0; k < 3; ++k) s[k] += g * plane[k][t + R + i];
      }
      const size_t p = row + static_cast<size_t>(x0 + t);
      for (int k = 0; k < 3; ++k) a.h[k * a.n_pixels + p] = s[k];
    }
    __syncthreads();  // (the next tile is staged over this one)
  }
}

extern "C" __global__ void __launch_bounds__(256) rtc_film_resolve_kernel(const FilmArgs a) {
  constexpr int CW = RTC_FILM_COL_W, CH = RTC_FILM_COL_H, TR = kColThreadRows, NP = kColPixels;
  extern __shared__ double film_lds[];
  const double E = exposure_of(a);
  if (a.scale_out && !a.e_dev && blockIdx.x == 0u && threadIdx.x == 0u) *a.scale_out = E;
  const int R = static_cast<int>(a.radius), t = static_cast<int>(threadIdx.x);
  const int tx = t & (CW - 1), ty = t / CW;
  for (uint64_t tile = blockIdx.x; tile < a.col_tiles; tile += gridDim.x) {
    const int64_t x = static_cast<int64_t>(tile % a.col_tiles_x) * CW + tx, y0 = static_cast<int64_t>(tile / a.col_tiles_x) * CH;
    const bool x_in = x < static_cast<int64_t>(a.hsize);
    double B[NP][3];
    for (int k = 0; k < 3; ++k) {
      const double* const hp = a.h + k * a.n_pixels;
      for (int r = ty; r < CH + 2 * R; r += TR) {
        const int64_t y = y0 - R + r;
        film_lds[r * CW + tx] = x_in && y >= 0 && y < static_cast<int64_t>(a.vsize) ? hp[static_cast<size_t>(y) * a.hsize + static_cast<size_t>(x)] : 0.0;
      }
      __syncthreads();
      double s[NP];
#pragma unroll
      for (int q = 0; q < NP; ++q) s[q] = 0.0;
      for (int j = -R; j <= R; ++j) {
        const double g = a.g[j < 0 ? -j : j];
        const double* const at = film_lds + (ty + R + j) * CW + tx;
#pragma unroll
        for (int q = 0; q < NP; ++q) s[q] += g * at[q * TR * CW];
      }
#pragma unroll
      for (int q = 0; q < NP; ++q) B[q][k] = s[q];
      __syncthreads();  // (the next plane is staged over this one)
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const int64_t y = y0 + ty + q * TR;
      if (x_in && y < static_cast<int64_t>(a.vsize)) resolve_pixel(a, E, static_cast<size_t>(y) * a.hsize + static_cast<size_t>(x), B[q]);
    }
  }
}

extern "C" __global__ void __launch_bounds__(256) rtc_film_naive_row_kernel(const FilmArgs a) {
  const double E = exposure_of(a);
  const int R = static_cast<int>(a.radius);
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < a.n_pixels; p += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const int64_t x = static_cast<int64_t>(p % a.hsize);
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = -R; i <= R; ++i) {
      if (x + i < 0 || x + i >= static_cast<int64_t>(a.hsize)) continue;
      const size_t q = static_cast<size_t>(static_cast<int64_t>(p) + i);
      const double e[3] = {E * a.in[3 * q], E * a.in[3 * q + 1], E * a.in[3 * q + 2]};
      double b[3];
      bright_pass(a, e, b);
      const double g = a.g[i < 0 ? -i : i];
      for (int k = 0; k < 3; ++k) s[k] += g * b[k];
    }
    for (int k = 0; k < 3; ++k) a.h[k * a.n_pixels + p] = s[k];
  }
}

extern "C" __global__ void __launch_bounds__(256) rtc_film_naive_resolve_kernel(const FilmArgs a) {
  const double E = exposure_of(a);
  if (a.scale_out && !a.e_dev && blockIdx.x == 0u && threadIdx.x == 0u) *a.scale_out = E;
  const int R = static_cast<int>(a.radius);
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < a.n_pixels; p += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const int64_t y = static_cast<int64_t>(p / a.hsize);
    double B[3] = {0.0, 0.0, 0.0};
    for (int j = -R; j <= R; ++j) {
      if (y + j < 0 || y + j >= static_cast<int64_t>(a.vsize)) continue;
      const size_t q = static_cast<size_t>(static_cast<int64_t>(p) + static_cast<int64_t>(j) * a.hsize);
      const double g = a.g[j < 0 ? -j : j];
      for (int k = 0; k < 3; ++k) B[k] += g * a.h[k * a.n_pixels + q];
    }
    resolve_pixel(a, E, p, B);
  }
}

// ---- the host side (rtc_capi.hip calls it after validating the arguments)
void rtcFilmTile(uint32_t* row_w, uint32_t* col_w, uint32_t* col_h) { *row_w = RTC_FILM_ROW_W, *col_w = RTC_FILM_COL_W, *col_h = RTC_FILM_COL_H; }

static bool filmBlooms(const rtc_film_setting& s) { return s.bloom_radius >= 1u && s.bloom_intensity > 0.0; }

// Blocks of the streaming kernels' grid: a function of the items alone
static uint32_t filmBlocks(size_t items) {
  const size_t b = (items + 255) / 256;
  return static_cast<uint32_t>(b < RTC_FILM_MAX_BLOCKS ? b : RTC_FILM_MAX_BLOCKS);
}

// scratch: E (16 bytes) and the partials where the exposure is automatic, then H where the setting blooms
static size_t filmPartialBytes(size_t n_pixels) { return 16u + ((filmBlocks(n_pixels) * sizeof(double) + 15u) & ~static_cast<size_t>(15u)); }

size_t rtcFilmScratchBytes(uint32_t hsize, uint32_t vsize, const rtc_film_setting* s) {
  const size_t n = static_cast<size_t>(hsize) * vsize;
  return (s->auto_key > 0.0 ? filmPartialBytes(n) : 0u) + (filmBlooms(*s) ? 3u * n * sizeof(double) : 0u);
}

static double hableHost(double v) { return ((v * (0.15 * v + 0.05) + 0.004) / (v * (0.15 * v + 0.5) + 0.06)) - 0.02 / 0.3; }

hipError_t rtcFilmLaunch(const rtc_film* f, bool naive, hipStream_t stream) {
  const rtc_film_setting& s = f->setting;
  FilmArgs a{};
  a.in = f->in, a.out = f->out, a.rgba = f->rgba, a.scale_out = f->scale_out;
  a.n_pixels = static_cast<size_t>(f->hsize) * f->vsize, a.hsize = f->hsize, a.vsize = f->vsize;
  a.exposure = s.exposure, a.threshold = s.bloom_threshold, a.intensity = s.bloom_intensity;
  a.white2 = s.white * s.white, a.hable_white = hableHost(s.white);
  a.inv_power = s.transfer == RTC_FILM_TRANSFER_GAMMA ? 1.0 / s.gamma : 1.0 / 2.4;
  a.curve = s.curve, a.transfer = s.transfer;
  char* scratch = static_cast<char*>(f->scratch);
  if (s.auto_key > 0.0) {
    double* const e_dev = reinterpret_cast<double*>(scratch);
    double* const partials = reinterpret_cast<double*>(scratch + 16);
    const uint32_t blocks = filmBlocks(a.n_pixels);
    hipLaunchKernelGGL(rtc_film_log_kernel, dim3(blocks), dim3(256), 0, stream, f->in, a.n_pixels, partials);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(rtc_film_exposure_kernel, dim3(1), dim3(256), 0, stream, static_cast<const double*>(partials), blocks, a.n_pixels,
                       s.exposure * s.auto_key, e_dev, f->scale_out);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    a.e_dev = e_dev;
    scratch += filmPartialBytes(a.n_pixels);
  }
  if (!filmBlooms(s)) {
    auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; };
    const bool wide = a16(f->in) && a16(f->out) && (!f->rgba || (reinterpret_cast<uintptr_t>(f->rgba) & 7u) == 0u);
    if (wide) hipLaunchKernelGGL(rtc_film_point_kernel, dim3(filmBlocks((a.n_pixels + 1) / 2)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(rtc_film_point_narrow_kernel, dim3(filmBlocks(a.n_pixels)), dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  // the weights: formed here in doubles, handed to the kernels by value
  const uint32_t R = s.bloom_radius;
  double raw[RTC_FILM_MAX_RADIUS + 1];
  for (uint32_t i = 0; i <= R; ++i) raw[i] = std::exp(-static_cast<double>(i * i) / (2.0 * s.bloom_sigma * s.bloom_sigma));
  double norm = raw[0];
  for (uint32_t i = 1; i <= R; ++i) norm = norm + 2.0 * raw[i];
  for (uint32_t i = 0; i <= R; ++i) a.g[i] = raw[i] / norm;
  a.radius = R;
  a.h = reinterpret_cast<double*>(scratch);
  a.row_tiles_x = (f->hsize + RTC_FILM_ROW_W - 1u) / RTC_FILM_ROW_W;
  a.row_tiles = static_cast<uint64_t>(a.row_tiles_x) * f->vsize;
  a.col_tiles_x = (f->hsize + RTC_FILM_COL_W - 1u) / RTC_FILM_COL_W;
  a.col_tiles = static_cast<uint64_t>(a.col_tiles_x) * ((f->vsize + RTC_FILM_COL_H - 1u) / RTC_FILM_COL_H);
  auto capped = [](uint64_t blocks) { return dim3(static_cast<uint32_t>(blocks < RTC_FILM_MAX_TILE_BLOCKS ? blocks : RTC_FILM_MAX_TILE_BLOCKS)); };
  if (naive) {
    const dim3 grid = capped((static_cast<uint64_t>(a.n_pixels) + 255u) / 256u);
    hipLaunchKernelGGL(rtc_film_naive_row_kernel, grid, dim3(256), 0, stream, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(rtc_film_naive_resolve_kernel, grid, dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(rtc_film_row_kernel, capped(a.row_tiles), dim3(256), 0, stream, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(rtc_film_resolve_kernel, capped(a.col_tiles), dim3(256), resolveLdsDoubles(R) * sizeof(double), stream, a);
  }
  return hipGetLastError();
}
