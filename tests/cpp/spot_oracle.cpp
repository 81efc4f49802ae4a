// spot_oracle.cpp — CPU checker of spot lights (libspot_oracle.so).  TEST INFRASTRUCTURE.
//
// Spot lights (include/rtc.h rtc_scene_set_spots) on top of the motion-blur checker:
// motion_oracle.cpp is included, read-only, and with it the camera-sampling and area-light checkers and the oracle's
// sources.  What is restated here is only what spots change:
//   - shadeHit's point-light branch: the cone's factor f at c = -(point_to_light . axis); f == 0 gives `ambient` with no
//     isShadowed call, otherwise isShadowed as before and Material.lighting with diffuse and specular scaled by f;
//   - through it colorAt, reflectedColor and refractedColor, and the pass loop that calls colorAt.
// Intersection, PreComputations, patterns, isShadowed, area lighting and the sample rays are the motion checker's.
// Nothing of the product is included or linked.
#include "motion_oracle.cpp"

namespace spot {

struct Cone {
  bool on = false;
  orc::Tuple axis = orc::vec3(0.0, 0.0, 0.0);  // unit (tuple.zig's normalize of the given axis)
  double cos_inner = 1.0, cos_outer = 1.0;
};

// Whether an evaluation of the pixel being rendered had a hard-edged cone with c within 1e-9 of its cosine: there one
// rounding of the hit point decides between lit and unlit (the parity tests mask such pixels).
thread_local bool t_hard_edge = false;

// The cone's factor, each operation correctly rounded (-ffp-contract=off)
double factor(double c, double cos_inner, double cos_outer) {
  if (c >= cos_inner) return 1.0;
  if (c <= cos_outer) return 0.0;
  const double s = (c - cos_outer) / (cos_inner - cos_outer);
  return (s * s) * (3.0 - 2.0 * s);
}

double coneFactor(const Cone& K, orc::Tuple point_to_light) {
  if (!K.on) return 1.0;
  const double c = -((point_to_light.x * K.axis.x + point_to_light.y * K.axis.y) + point_to_light.z * K.axis.z);
  if (K.cos_inner == K.cos_outer && std::fabs(c - K.cos_outer) < 1e-9) t_hard_edge = true;
  return factor(c, K.cos_inner, K.cos_outer);
}

std::vector<Cone> make(const area::Scene& S, const uint8_t* cone, const double* axis, const double* cos_inner, const double* cos_outer,
                       uint32_t n_lights) {
  if (n_lights != S.lights.size()) throw std::runtime_error("InvalidArgument: n_lights");
  std::vector<Cone> cones(n_lights);
  for (uint32_t i = 0; i < n_lights && cone; ++i) {
    if (cone[i] > 1) throw std::runtime_error("InvalidArgument: cone flag");
    if (cone[i] == 0) continue;
    if (S.lights[i].is_area) throw std::runtime_error("InvalidArgument: a cone on an area light");
    Cone& K = cones[i];
    K.on = true;
    K.axis = orc::normalized(orc::vec3(axis[3 * i], axis[3 * i + 1], axis[3 * i + 2]));
    K.cos_inner = cos_inner[i];
    K.cos_outer = cos_outer[i];
  }
  return cones;
}

// Material.lighting (material.zig:40-74) of a point light, diffuse and specular scaled by f once formed
orc::Color spotLighting(const orc::Material& m, orc::Color color, const area::Light& L, orc::Tuple point_to_light, orc::Tuple eyev,
                        orc::Tuple normal, bool in_shadow, double f) {
  const orc::Color effective_color = orc::cemul(color, L.intensity);
  const orc::Color ambient_ = orc::cmul(effective_color, m.ambient);
  if (in_shadow) return ambient_;
  orc::Color diffuse_{0.0, 0.0, 0.0}, specular_{0.0, 0.0, 0.0};
  const double light_dot_normal = orc::dot(point_to_light, normal);
  if (light_dot_normal >= 0.0) {
    diffuse_ = orc::cmul(orc::cmul(effective_color, m.diffuse * light_dot_normal), f);
    const double reflect_dot_eye = orc::dot(orc::negate(orc::reflect(point_to_light, normal)), eyev);
    if (reflect_dot_eye > 0.0) specular_ = orc::cmul(orc::cmul(L.intensity, m.specular * orc::zig_pow(reflect_dot_eye, m.shininess)), f);
  }
  return orc::cadd(orc::cadd(ambient_, diffuse_), specular_);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<Cone>& K, const orc::Ray& ray, size_t remaining,
                   const area::Jitter& J);

orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<Cone>& K, const orc::PreComputations& comps,
                    size_t remaining, const area::Jitter& J) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  for (uint32_t l = 0; l < S.lights.size(); ++l) {
    const area::Light& L = S.lights[l];
    const orc::Color color = motion::colorAtPoint(M, obj, comps.over_point);
    if (!L.is_area) {
      const orc::Tuple point_to_light = orc::normalized(orc::sub(L.corner, comps.over_point));
      const double f = coneFactor(K[l], point_to_light);
      if (f == 0.0) {  // outside the cone: `ambient` alone, and no isShadowed call
        surface = orc::cadd(surface, orc::cmul(orc::cemul(color, L.intensity), m.ambient));
        continue;
      }
      const bool shadowed = motion::isShadowed(S, M, comps.over_point, L.corner);
      surface = orc::cadd(surface, spotLighting(m, color, L, point_to_light, comps.eyev, comps.normal, shadowed, f));
    } else {
      surface = orc::cadd(surface, motion::areaLighting(S, M, m, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    reflected = orc::cmul(colorAt(S, M, K, orc::Ray{comps.over_point, comps.reflectv}, remaining - 1, J), m.reflective);
  }
  {  // world.zig:171-189
    const double n_ratio = comps.n1 / comps.n2;
    const double cos_i = orc::dot(comps.eyev, comps.normal);
    const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
    if (!(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0) {
      const double cos_t = std::sqrt(1.0 - sin2_t);
      const orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
      orc::counters().secondary++;
      refracted = orc::cmul(colorAt(S, M, K, orc::Ray{comps.under_point, direction}, remaining - 1, J), m.transparency);
    }
  }
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<Cone>& K, const orc::Ray& ray, size_t remaining,
                   const area::Jitter& J) {
  const orc::Intersections xs = motion::intersect(S, M, ray);
  const long h = orc::hit(xs);
  if (h >= 0) return shadeHit(S, M, K, motion::precompute(M, xs[h], ray, xs), remaining, J);
  return {0.0, 0.0, 0.0};
}

// motion::render's pixel loop with spot::colorAt, and the hard-edge flag of every pixel
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<Cone>& cones, uint32_t x0, uint32_t y0, uint32_t w,
           uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out, uint8_t* edge_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const motion::Motion base = motion::make(S, disp, n_roots);
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
      motion::Motion M = base;
      try {
        for (;;) {
          const uint32_t r = next_row.fetch_add(1);
          if (r >= h || failed.load()) break;
          const uint32_t y = y0 + r;
          for (uint32_t i = 0; i < w; ++i) {
            const uint32_t x = x0 + i;
            const uint64_t p = static_cast<uint64_t>(y) * cam->hsize + x;
            orc::Color sum{0.0, 0.0, 0.0};
            t_hard_edge = false;
            for (uint32_t k = 0; k < n_samples; ++k) {
              const uint64_t g = static_cast<uint64_t>(pass) * n_samples + k;
              orc::counters().primary++;
              area::Jitter J;
              J.seed = light_seed;
              J.pixel = (pass * n_pixels + p) * n_samples + k;  // (u64, wraps)
              J.n_lights = S.lights.size();
              M.t = motion::time(smp.seed, p, g);
              sum = orc::cadd(sum, colorAt(S, M, cones, motion::passRay(camera, smp, x, y, k, g), max_depth, J));
              orc::Arena::mine().reset();
            }
            const double n = static_cast<double>(n_samples);
            double* px = rgb_out + 3 * (static_cast<size_t>(r) * w + i);
            px[0] = sum.r / n;
            px[1] = sum.g / n;
            px[2] = sum.b / n;
            if (edge_out) edge_out[static_cast<size_t>(r) * w + i] = t_hard_edge ? 1 : 0;
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

}  // namespace spot

extern "C" {

// The scene: area_scene_create / area_scene_destroy of the included checkers; disp [n_roots][3] in World.objects order
// (the motion checker's); cone / axis [n][3] / cos_inner / cos_outer in World.lights order (rtc_spot; cone NULL: none).
// rgb_out [h][w][3] of the rectangle [x0, x0 + w) x [y0, y0 + h); counters_out [primary, secondary, shadow calls];
// edge_out [h][w] (may be NULL): 1 where an evaluation met a hard-edged cone within 1e-9 of its cosine.
int spot_render(void* scene, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling, uint32_t pass,
                const double* disp, uint32_t n_roots, const uint8_t* cone, const double* axis, const double* cos_inner,
                const double* cos_outer, uint32_t n_lights, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads,
                double* rgb_out, uint64_t* counters_out, uint8_t* edge_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  std::vector<spot::Cone> cones;
  try {
    cones = spot::make(S, cone, axis, cos_inner, cos_outer, n_lights);
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
  return spot::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, x0, y0, w, h, n_threads, rgb_out, counters_out,
                      edge_out);
}

// ---- KAT hook: the cone's factor
double spot_kat_factor(double c, double cos_inner, double cos_outer) { return spot::factor(c, cos_inner, cos_outer); }

}  // extern "C"
