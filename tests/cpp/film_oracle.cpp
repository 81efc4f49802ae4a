// film_oracle.cpp — the film stage's checker.  TEST INFRASTRUCTURE: include/rtc.h's contract of rtc_film_device (DESIGN.md
// section 30) restated as plain loops in doubles, built with -ffp-contract=off; it includes and links nothing of the product.
//
// The one sum whose order the contract leaves open, T, is taken in long double, so that the checker's own error does not
// count; `e_given`, where not NULL, is used in place of the checker's own E.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

constexpr double kEps = 1e-10;        // RTC_FILM_EPS
constexpr uint32_t kMaxRadius = 32u;  // RTC_FILM_MAX_RADIUS
enum { CURVE_LINEAR = 0, CURVE_REINHARD = 1, CURVE_ACES = 2, CURVE_HABLE = 3 };
enum { TRANSFER_LINEAR = 0, TRANSFER_SRGB = 1, TRANSFER_GAMMA = 2 };

double luminance(const double* c) { return (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]; }

double max0(double x) { return x > 0 ? x : 0; }

double hable(double v) { return ((v * (0.15 * v + 0.05) + 0.004) / (v * (0.15 * v + 0.5) + 0.06)) - 0.02 / 0.3; }

double curveOf(uint32_t curve, double white, double c) {
  switch (curve) {
    case CURVE_REINHARD: return (c * (1.0 + c / (white * white))) / (1.0 + c);
    case CURVE_ACES: return (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14);
    case CURVE_HABLE: return hable(c) / hable(white);
    default: return c;
  }
}

double transferOf(uint32_t transfer, double gamma, double t) {
  switch (transfer) {
    case TRANSFER_SRGB: return t <= 0.0031308 ? 12.92 * t : 1.055 * std::pow(t, 1.0 / 2.4) - 0.055;
    case TRANSFER_GAMMA: return t > 0 ? std::pow(t, 1.0 / gamma) : 0.0;
    default: return t;
  }
}

bool isFinite(double v) { return std::isfinite(v); }

}  // namespace

extern "C" {

// One channel through the curve and the transfer (the known answers of tests/test_film_cpu.py)
double film_oracle_develop(uint32_t curve, double white, uint32_t transfer, double gamma, double c) {
  return transferOf(transfer, gamma, curveOf(curve, white, c));
}

// g[0 .. radius]
int film_oracle_weights(uint32_t radius, double sigma, double* g) {
  if (radius > kMaxRadius) return 1;
  double raw[kMaxRadius + 1];
  for (uint32_t i = 0; i <= radius; ++i) raw[i] = std::exp(-static_cast<double>(i * i) / (2.0 * sigma * sigma));
  double norm = raw[0];
  for (uint32_t i = 1; i <= radius; ++i) norm = norm + 2.0 * raw[i];
  for (uint32_t i = 0; i <= radius; ++i) g[i] = raw[i] / norm;
  return 0;
}

// in, out: [h][w][3]; e_given: NULL, or the E to use; e_out: NULL, or where the E used goes.  1: a setting the contract refuses.
int film_oracle(const double* in, uint32_t w, uint32_t h, double exposure, double auto_key, uint32_t radius, double sigma, double threshold,
                double intensity, uint32_t curve, double white, uint32_t transfer, double gamma, const double* e_given, double* out,
                double* e_out) {
  if (!in || !out || w == 0u || h == 0u) return 1;
  if (!isFinite(exposure) || exposure <= 0 || !isFinite(auto_key) || auto_key < 0 || radius > kMaxRadius) return 1;
  if (radius > 0u && (!isFinite(sigma) || sigma <= 0)) return 1;
  if (!isFinite(threshold) || threshold < 0 || !isFinite(intensity) || intensity < 0) return 1;
  if (curve > CURVE_HABLE || transfer > TRANSFER_GAMMA || !isFinite(white) || white <= 0 || !isFinite(gamma) || gamma <= 0) return 1;
  const size_t n = static_cast<size_t>(w) * h;
  const int64_t W = w, H = h;

  // 1. the exposure
  double E = exposure;
  if (auto_key != 0) {
    long double T = 0.0L;
    for (size_t q = 0; q < n; ++q) T += static_cast<long double>(std::log(kEps + max0(luminance(in + 3 * q))));
    E = (exposure * auto_key) / std::exp(static_cast<double>(T / static_cast<long double>(n)));
  }
  if (e_given) E = *e_given;
  if (e_out) *e_out = E;

  // 2. the exposed image
  std::vector<double> x(3 * n);
  for (size_t i = 0; i < 3 * n; ++i) x[i] = E * in[i];

  // 3. the bloom
  const bool blooms = radius >= 1u && intensity > 0;
  std::vector<double> B;
  if (blooms) {
    double g[kMaxRadius + 1];
    film_oracle_weights(radius, sigma, g);
    const int R = static_cast<int>(radius);
    std::vector<double> b(3 * n), Hh(3 * n);
    B.resize(3 * n);
    for (size_t p = 0; p < n; ++p) {
      const double y = luminance(&x[3 * p]);
      const double wgt = max0(y - threshold) / (y > kEps ? y : kEps);
      for (int c = 0; c < 3; ++c) b[3 * p + c] = x[3 * p + c] * wgt;
    }
    for (int64_t py = 0; py < H; ++py)
      for (int64_t px = 0; px < W; ++px)
        for (int c = 0; c < 3; ++c) {
          double s = 0.0;
          for (int i = -R; i <= R; ++i)
            if (px + i >= 0 && px + i < W) s = s + g[i < 0 ? -i : i] * b[3 * (py * W + px + i) + c];
          Hh[3 * (py * W + px) + c] = s;
        }
    for (int64_t py = 0; py < H; ++py)
      for (int64_t px = 0; px < W; ++px)
        for (int c = 0; c < 3; ++c) {
          double s = 0.0;
          for (int j = -R; j <= R; ++j)
            if (py + j >= 0 && py + j < H) s = s + g[j < 0 ? -j : j] * Hh[3 * ((py + j) * W + px) + c];
          B[3 * (py * W + px) + c] = s;
        }
  }

  // 4 .. 7. the combine, the curve, the transfer
  for (size_t i = 0; i < 3 * n; ++i) {
    const double c = blooms ? x[i] + intensity * B[i] : x[i];
    out[i] = transferOf(transfer, gamma, curveOf(curve, white, c));
  }
  return 0;
}

// rgba [h][w] of out: the clamp (color.zig:61-71), alpha 255
void film_oracle_rgba(const double* out, uint64_t n, uint32_t* rgba) {
  auto clamp8 = [](double channel) -> uint32_t {
    const double t = std::round(channel * 255);
    if (!(t >= 0)) return 0u;
    if (t > 255) return 255u;
    return static_cast<uint32_t>(t);
  };
  for (uint64_t p = 0; p < n; ++p) rgba[p] = clamp8(out[3 * p]) | (clamp8(out[3 * p + 1]) << 8) | (clamp8(out[3 * p + 2]) << 16) | 0xFF000000u;
}

}  // extern "C"
