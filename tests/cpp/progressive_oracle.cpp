// progressive_oracle.cpp — CPU checker of sample passes (libprogressive_oracle.so).  TEST INFRASTRUCTURE.
//
// Progressive rendering (include/rtc.h rtc_scene_set_sample_pass) on top of the camera-sampling
// checker: its scene build, colorAt, Jitter and hash are used as they are (camera_oracle.cpp is included, read-only, and
// with it the area-light checker and the oracle's sources).  What is restated here is only what a pass changes: the
// camera hash of sample k is keyed on the global index g = pass * S + k (the sub-pixel stratum stays that of k), and an
// area light's jitter on the pixel (pass * N + p) * S + k, u64 and wrapping - on the same threaded pixel loop.  Pass 0
// is cam_render to the bit.  Nothing of the product is included or linked.
#include "camera_oracle.cpp"

namespace passes {

// camsmp::sampleRay with the hash's sample index `g` apart from the stratum's `k`
orc::Ray passRay(const orc::Camera& c, const camsmp::Sampling& s, size_t x, size_t y, uint32_t k, uint64_t g) {
  const uint32_t j = k / s.grid, i = k % s.grid;
  const uint64_t p = static_cast<uint64_t>(y) * c.hsize + x;
  const double jx = s.jitter ? camsmp::hash(s.seed, p, g, 0) : 0.5;
  const double jy = s.jitter ? camsmp::hash(s.seed, p, g, 1) : 0.5;
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
  double lx = 0.0, ly = 0.0;
  for (uint32_t t = 0; t < 32; ++t) {
    const double a = 2.0 * camsmp::hash(s.seed, p, g, 2 + 2 * t) - 1.0;
    const double b = 2.0 * camsmp::hash(s.seed, p, g, 3 + 2 * t) - 1.0;
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

uint64_t areaKey(uint64_t pass, uint64_t n_pixels, uint64_t p, uint64_t samples, uint64_t k) {
  return (pass * n_pixels + p) * samples + k;  // (u64, wraps)
}

}  // namespace passes

extern "C" {

// cam_render of sample pass `pass`: rgb_out [h][w][3] of the rectangle; counters_out [primary, secondary, shadow calls]
int pass_render(void* scene, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
                uint32_t pass, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out,
                uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if ((static_cast<uint64_t>(pass) + 1) * n_samples > (1ull << 24)) throw std::runtime_error("InvalidArgument: pass");
    const uint64_t n_pixels = static_cast<uint64_t>(cam->hsize) * cam->vsize;
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
              J.pixel = passes::areaKey(pass, n_pixels, p, n_samples, k);
              J.n_lights = S.lights.size();
              const uint64_t g = static_cast<uint64_t>(pass) * n_samples + k;
              sum = orc::cadd(sum, area::colorAt(S, passes::passRay(camera, smp, x, y, k, g), max_depth, J));
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

// ---- KAT hooks: the camera hash of sample k of pass `pass` (S samples a pass), and the area key
void pass_kat_hash(uint64_t seed, uint64_t p, uint32_t pass, uint32_t samples, uint32_t k, uint32_t axis, double* out) {
  *out = camsmp::hash(seed, p, static_cast<uint64_t>(pass) * samples + k, axis);
}

uint64_t pass_kat_area_key(uint32_t pass, uint64_t n_pixels, uint64_t p, uint32_t samples, uint32_t k) {
  return passes::areaKey(pass, n_pixels, p, samples, k);
}

}  // extern "C"
