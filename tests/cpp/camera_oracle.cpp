// camera_oracle.cpp — CPU checker of camera samples per pixel (libcamera_oracle.so).  TEST INFRASTRUCTURE.
//
// Anti-aliasing and focal blur (include/rtc.h rtc_sampling) on top of the area-light checker:
// its scene build, colorAt and Jitter are used as they are (area_oracle.cpp is included, read-only, and with it the
// oracle's sources).  What is restated here is only what sampling adds - the sample's sub-pixel offsets, the lens, the
// camera hash and the mean of the samples - on the same threaded pixel loop.  Nothing of the product is included or
// linked.  The area lights' jitter of sample k of the whole-image pixel p is keyed on p * samples + k.
#include "area_oracle.cpp"

namespace camsmp {

struct Sampling {
  uint32_t grid = 1;
  bool jitter = false;
  double aperture = 0.0, focal = 1.0;
  uint64_t seed = 0;
};

// j(axis) of sample k of pixel p: the splitmix64 finaliser on mix(seed ^ pi) + golden * (c + 1)
double hash(uint64_t seed, uint64_t p, uint64_t k, uint64_t axis) {
  const uint64_t c = (p << 32) | (k << 8) | axis;
  const uint64_t key = area::mix(seed ^ 0x243F6A8885A308D3ull);
  return static_cast<double>(area::mix(key + 0x9E3779B97F4A7C15ull * (c + 1)) >> 11) * 0x1.0p-53;
}

// The primary ray of sample k = j * grid + i of pixel (x, y).  Grid 1, no jitter, no aperture: Camera.rayForPixel.
orc::Ray sampleRay(const orc::Camera& c, const Sampling& s, size_t x, size_t y, uint32_t k) {
  const uint32_t j = k / s.grid, i = k % s.grid;
  const uint64_t p = static_cast<uint64_t>(y) * c.hsize + x;
  const double jx = s.jitter ? hash(s.seed, p, k, 0) : 0.5;
  const double jy = s.jitter ? hash(s.seed, p, k, 1) : 0.5;
  const double n = static_cast<double>(s.grid);
  const double ox = (static_cast<double>(i) + jx) / n;
  const double oy = (static_cast<double>(j) + jy) / n;
  const double xoffset = (static_cast<double>(x) + ox) * c.pixel_size;
  const double yoffset = (static_cast<double>(y) + oy) * c.pixel_size;
  const double world_x = c.half_width - xoffset;
  const double world_y = c.half_height - yoffset;
  if (s.aperture == 0.0) {
    const orc::Tuple pixel = c.inverse.tupleMul(orc::point(world_x, world_y, -1.0));
    const orc::Tuple origin = c.inverse.tupleMul(orc::point(0.0, 0.0, 0.0));
    return {origin, orc::normalized(orc::sub(pixel, origin))};
  }
  double lx = 0.0, ly = 0.0;  // the first of 32 draws inside the unit disc, else its centre
  for (uint32_t t = 0; t < 32; ++t) {
    const double a = 2.0 * hash(s.seed, p, k, 2 + 2 * t) - 1.0;
    const double b = 2.0 * hash(s.seed, p, k, 3 + 2 * t) - 1.0;
    if ((a * a) + (b * b) <= 1.0) {
      lx = a;
      ly = b;
      break;
    }
  }
  const double f = s.focal;
  const orc::Tuple origin = c.inverse.tupleMul(orc::point(s.aperture * lx, s.aperture * ly, 0.0));
  const orc::Tuple pixel = c.inverse.tupleMul(orc::point(world_x * f, world_y * f, -f));
  return {origin, orc::normalized(orc::sub(pixel, origin))};
}

Sampling from(const rtc_sampling* s) {
  Sampling out;
  if (s) {
    if (s->grid < 1 || s->grid > 16) throw std::runtime_error("InvalidArgument: grid");
    out.grid = s->grid;
    out.jitter = s->jitter != 0;
    out.aperture = s->aperture;
    out.focal = s->focal_distance;
    out.seed = s->seed;
  }
  return out;
}

}  // namespace camsmp

extern "C" {

// The scene: area_scene_create / area_scene_destroy of the included checker.
// rgb_out [h][w][3] of the rectangle [x0, x0 + w) x [y0, y0 + h); counters_out [primary, secondary, shadow calls]
int cam_render(void* scene, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
               uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    std::atomic<uint32_t> next_row{0};
    std::vector<orc::Counters> per_thread(n_threads);
    std::string error;
    std::atomic<bool> failed{false};
    auto worker = [&](uint32_t tid) {
      orc::counters() = orc::Counters{};
      try {
        for (;;) {
          const uint32_t r = next_row.fetch_add(1);
          if (r >= h || failed.load()) break;
          const uint32_t y = y0 + r;
          for (uint32_t i = 0; i < w; ++i) {
            const uint32_t x = x0 + i;
            const uint64_t p = static_cast<uint64_t>(y) * cam->hsize + x;
            orc::Color sum{0.0, 0.0, 0.0};
            for (uint32_t k = 0; k < n_samples; ++k) {
              orc::counters().primary++;
              area::Jitter J;
              J.seed = light_seed;
              J.pixel = p * n_samples + k;
              J.n_lights = S.lights.size();
              sum = orc::cadd(sum, area::colorAt(S, camsmp::sampleRay(camera, smp, x, y, k), max_depth, J));
              orc::Arena::mine().reset();
            }
            const double n = static_cast<double>(n_samples);
            double* px = rgb_out + 3 * (static_cast<size_t>(r) * w + i);
            px[0] = sum.r / n;
            px[1] = sum.g / n;
            px[2] = sum.b / n;
          }
        }
      } catch (const std::exception& e) {
        if (!failed.exchange(true)) error = e.what();
      }
      per_thread[tid] = orc::counters();
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; ++t) pool.emplace_back(worker, t);
    worker(0);
    for (auto& t : pool) t.join();
    if (failed.load()) {
      g_error = error;
      return 1;
    }
    if (counters_out) {
      orc::Counters total;
      for (const auto& c : per_thread) total.add(c);
      counters_out[0] = total.primary;
      counters_out[1] = total.secondary;
      counters_out[2] = total.shadow;
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

// ---- KAT hooks: the camera hash, and one sample's ray (origin xyz, direction xyz)
void cam_kat_hash(uint64_t seed, const uint64_t* p, const uint64_t* k, const uint64_t* axis, uint64_t n, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = camsmp::hash(seed, p[i], k[i], axis[i]);
}

int cam_kat_ray(const rtc_camera* cam, const rtc_sampling* sampling, uint32_t x, uint32_t y, uint32_t k, double* out) {
  try {
    const orc::Ray r = camsmp::sampleRay(cameraFrom(*cam), camsmp::from(sampling), x, y, k);
    const double v[6] = {r.origin.x, r.origin.y, r.origin.z, r.direction.x, r.direction.y, r.direction.z};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // extern "C"
