// occlusion_oracle.cpp — CPU checker of ambient occlusion (liboccl_oracle.so).  TEST INFRASTRUCTURE.
//
// Hemisphere rays that dim a material's ambient term (include/rtc.h rtc_scene_set_occlusion) on top
// of the gloss checker: gloss_oracle.cpp is included, read-only, and with it the mesh-texture, torus, bump, spot, motion,
// camera-sampling and area-light checkers and the oracle's sources.  What is restated here is what the feature changes:
//   - shadeHit: the occlusion step of rtc.h before the lights, and its ka in material.ambient's place for every light;
//   - the direction of one sample, from the gloss checker's sampler and hash with this feature's key and word;
//   - colorAt and the pass loop, as gloss_oracle.cpp has them, because they name shadeHit.
// Four counters beside the ray counts: occluded samples, unoccluded samples, hits with a radius skipped for ambient == 0,
// occlusion hits of a ray whose path code is above 1.
// Nothing of the product is included or linked.
#include "gloss_oracle.cpp"

namespace occl {

constexpr uint64_t kSalt = 0xA4093822299F31D0ull;
constexpr uint32_t kMaxSamples = 64;
constexpr uint32_t kSampleShift = 17;

struct Table {
  std::vector<double> radius;  // per material row (mat_* order); a leaf's row: bump::Table::mat_of
  uint32_t samples = 1;
  uint64_t seed = 0;
};

std::atomic<uint64_t> g_occluded{0}, g_clear{0}, g_skipped{0}, g_deep{0};

uint64_t keyOf(uint64_t seed) { return gloss::mix64(seed ^ kSalt); }

// The direction of one sample: J(axis) -> a draw in [0, 1).  The first of the 32 triples with q <= 1; none, or q == 0: ng.
template <class F>
orc::Tuple direction(F&& J, orc::Tuple ng) {
  for (uint32_t t = 0; t < gloss::kDraws; ++t) {
    const double a = 2.0 * J(3 * t + 0) - 1.0;
    const double b = 2.0 * J(3 * t + 1) - 1.0;
    const double c = 2.0 * J(3 * t + 2) - 1.0;
    const double q = ((a * a) + (b * b)) + (c * c);
    if (q <= 1.0) {
      if (q == 0.0) return ng;
      const double r = std::sqrt(q);
      const double ex = ng.x + a / r, ey = ng.y + b / r, ez = ng.z + c / r;
      const double m = std::sqrt((ex * ex + ey * ey) + ez * ez);
      if (m == 0.0) return ng;
      return orc::vec3(ex / m, ey / m, ez / m);
    }
  }
  return ng;
}

// torus::isShadowed for a ray given by its direction and its length
bool occluded(const area::Scene& S, const motion::Motion& M, const torus::Table& Q, orc::Tuple pt, orc::Tuple d, double distance) {
  orc::counters().shadow++;
  const orc::Ray shadow_ray{pt, d};
  const orc::Intersections xs = torus::intersect(S, M, Q, shadow_ray);
  long i = orc::hit(xs);
  while (i >= 0) {
    if (xs[i].t < distance && xs[i].object->casts_shadow) return true;
    i = orc::hit(xs, static_cast<size_t>(i) + 1);
  }
  return false;
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const Table& O, const gloss::Ctx& X,
                   const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J);

// gloss::shadeHit with the occlusion step; X: the gloss draws' hash of the camera sample, XO: the occlusion draws'
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const Table& O, const gloss::Ctx& X,
                    const gloss::Ctx& XO, const meshuv::Hit& H, const orc::PreComputations& comps, orc::Tuple ng, uint64_t code,
                    size_t remaining, const area::Jitter& J) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  // ---- the occlusion step (rtc.h): once per hit, before the lights
  double ka = m.ambient;
  if (!O.radius.empty()) {
    const auto it = T.mat_of.find(obj->id);
    if (it == T.mat_of.end()) throw std::runtime_error("occlusion checker: a hit on a shape that is no leaf of the description");
    const double radius = O.radius[it->second];
    if (radius > 0.0 && m.ambient == 0.0) g_skipped.fetch_add(1, std::memory_order_relaxed);
    if (radius > 0.0 && m.ambient != 0.0) {
      if (code > 1) g_deep.fetch_add(1, std::memory_order_relaxed);
      uint32_t n_occluded = 0;
      for (uint32_t k = 0; k < O.samples; ++k) {
        const uint64_t word = (static_cast<uint64_t>(k) << kSampleShift) | code;
        const orc::Tuple d = direction([&](uint32_t axis) { return gloss::jitter(XO.h, word, axis); }, ng);
        if (occluded(S, M, Q, comps.over_point, d, radius)) ++n_occluded;
      }
      g_occluded.fetch_add(n_occluded, std::memory_order_relaxed);
      g_clear.fetch_add(O.samples - n_occluded, std::memory_order_relaxed);
      const double vis = static_cast<double>(O.samples - n_occluded) / static_cast<double>(O.samples);
      ka = m.ambient * vis;
    }
  }
  orc::Material mk;  // (the material with ka as its ambient, made only when ka differs)
  const orc::Material* ml = &m;
  if (ka != m.ambient) {
    mk = m;
    mk.ambient = ka;
    ml = &mk;
  }
  for (uint32_t l = 0; l < S.lights.size(); ++l) {
    const area::Light& L = S.lights[l];
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    if (!L.is_area) {
      const orc::Tuple point_to_light = orc::normalized(orc::sub(L.corner, comps.over_point));
      const double f = spot::coneFactor(K[l], point_to_light);
      if (f == 0.0) {
        surface = orc::cadd(surface, orc::cmul(orc::cemul(color, L.intensity), ka));
        continue;
      }
      const bool shadowed = torus::isShadowed(S, M, Q, comps.over_point, L.corner);
      surface = orc::cadd(surface, spot::spotLighting(*ml, color, L, point_to_light, comps.eyev, comps.normal, shadowed, f));
    } else {
      surface = orc::cadd(surface, torus::areaLighting(S, M, Q, *ml, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  double rough_r = 0.0, rough_t = 0.0;
  if (!G.reflection.empty()) {
    const auto it = T.mat_of.find(obj->id);
    if (it == T.mat_of.end()) throw std::runtime_error("occlusion checker: a hit on a shape that is no leaf of the description");
    rough_r = G.reflection[it->second];
    rough_t = G.transmission[it->second];
  }
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    orc::Tuple d = comps.reflectv;
    if (rough_r > 0.0) d = gloss::scatter(X, 2 * code, rough_r, d, ng, false);
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, X, XO, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J), m.reflective);
  }
  {  // world.zig:171-189
    const double n_ratio = comps.n1 / comps.n2;
    const double cos_i = orc::dot(comps.eyev, comps.normal);
    const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
    if (!(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0) {
      const double cos_t = std::sqrt(1.0 - sin2_t);
      orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
      orc::counters().secondary++;
      if (rough_t > 0.0) direction = gloss::scatter(X, 2 * code + 1, rough_t, direction, ng, true);
      refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, X, XO, orc::Ray{comps.under_point, direction}, 2 * code + 1, remaining - 1, J),
                            m.transparency);
    }
  }
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const Table& O, const gloss::Ctx& X,
                   const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  if (h < 0) return {0.0, 0.0, 0.0};
  const meshuv::Hit H = meshuv::hitOf(M, U, xs[h], ray);
  const orc::PreComputations comps = torus::precompute(M, T, Q, xs[h], ray, xs);
  // the geometric normal (torus::precompute's first step), negated by the same `inside`
  orc::Tuple ng = torus::normalAt(Q, xs[h].object, motion::shift(comps.point, M.t, motion::dispOf(M, xs[h].object)), xs[h]);
  if (comps.inside) ng = orc::negate(ng);
  return shadeHit(S, M, K, T, Q, U, G, O, X, XO, H, comps, ng, code, remaining, J);
}

// gloss::render's pixel loop with occl::colorAt; counters_out [primary, secondary, shadow calls, occluded, unoccluded,
// skipped for ambient == 0, occlusion hits at a code above 1]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const Table& O, uint32_t x0, uint32_t y0, uint32_t w,
           uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const motion::Motion base = motion::make(S, disp, n_roots);
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if ((static_cast<uint64_t>(pass) + 1) * n_samples > (1ull << 24)) throw std::runtime_error("InvalidArgument: pass");
    const uint64_t n_pixels = static_cast<uint64_t>(cam->hsize) * cam->vsize;
    const uint64_t key = gloss::keyOf(G.seed), okey = keyOf(O.seed);
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    gloss::g_used = 0;
    gloss::g_fell = 0;
    g_occluded = 0;
    g_clear = 0;
    g_skipped = 0;
    g_deep = 0;
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
            for (uint32_t k = 0; k < n_samples; ++k) {
              const uint64_t g = static_cast<uint64_t>(pass) * n_samples + k;
              orc::counters().primary++;
              area::Jitter J;
              J.seed = light_seed;
              J.pixel = (pass * n_pixels + p) * n_samples + k;  // (u64, wraps)
              J.n_lights = S.lights.size();
              M.t = motion::time(smp.seed, p, g);
              gloss::Ctx X, XO;
              X.h = gloss::sampleKey(key, p, g);
              XO.h = gloss::sampleKey(okey, p, g);
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, O, X, XO, motion::passRay(camera, smp, x, y, k, g), 1, max_depth, J));
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
      counters_out[3] = g_occluded.load();
      counters_out[4] = g_clear.load();
      counters_out[5] = g_skipped.load();
      counters_out[6] = g_deep.load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace occl

extern "C" {

// The radius rows (NULL: all zeros; n_materials 0: no table at all), the samples and the seed.  Refuses what
// rtc_scene_set_occlusion refuses of the table's own values.
int occl_table_create(uint32_t n_materials, const double* radius, uint32_t samples, uint64_t seed, void** out) {
  try {
    auto t = std::make_unique<occl::Table>();
    t->radius.assign(n_materials, 0.0);
    for (uint32_t i = 0; i < n_materials; ++i) {
      if (radius) t->radius[i] = radius[i];
      if (!std::isfinite(t->radius[i]) || t->radius[i] < 0.0) throw std::runtime_error("InvalidArgument: a radius that is not finite or below 0");
    }
    if (samples < 1 || samples > occl::kMaxSamples) throw std::runtime_error("InvalidArgument: samples outside 1 .. 64");
    t->samples = samples;
    t->seed = seed;
    *out = t.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void occl_table_destroy(void* t) { delete static_cast<occl::Table*>(t); }

// The scene and the bump, torus, texture and gloss tables: as gloss_render's; and the occlusion table.  counters_out: 7 entries.
int occl_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, const rtc_camera* cam, uint32_t max_depth,
                uint64_t light_seed, const rtc_sampling* sampling, uint32_t pass, const double* disp, uint32_t n_roots, const uint8_t* cone,
                const double* axis, const double* cos_inner, const double* cos_outer, uint32_t n_lights, uint32_t x0, uint32_t y0,
                uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  std::vector<spot::Cone> cones;
  try {
    cones = spot::make(S, cone, axis, cos_inner, cos_outer, n_lights);
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
  return occl::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                      *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                      *static_cast<occl::Table*>(oc), x0, y0, w, h, n_threads, rgb_out, counters_out);
}

// ---- KAT hook
// the direction of one sample of (ng, draws[96]), each draw in [0, 1) -> out[3]
void occl_kat_direction(const double* ng, const double* draws, double* out) {
  const orc::Tuple d = occl::direction([&](uint32_t axis) { return draws[axis]; }, orc::vec3(ng[0], ng[1], ng[2]));
  out[0] = d.x;
  out[1] = d.y;
  out[2] = d.z;
}

}  // extern "C"
