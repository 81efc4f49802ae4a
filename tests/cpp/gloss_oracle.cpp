// gloss_oracle.cpp — CPU checker of glossy reflection and refraction (libgloss_oracle.so).  TEST INFRASTRUCTURE.
//
// Rough materials (include/rtc.h rtc_scene_set_gloss) on top of the mesh-texture checker:
// meshuv_oracle.cpp is included, read-only, and with it the torus, bump, spot, motion, camera-sampling and area-light
// checkers and the oracle's sources.  What is restated here is what the feature changes:
//   - reflectedColor / refractedColor (world.zig:157-189) with every ray's path code - the primary ray 1, the reflected
//     child of c 2 c, the refracted child 2 c + 1 - and the child direction of a rough material scattered as rtc.h writes it;
//   - the draws: the hash of rtc.h, restated (splitmix64's finaliser), and the rejection sampler over 32 triples;
//   - through them shadeHit, colorAt and the pass loop, as meshuv_oracle.cpp has them.
// Two counters beside the ray counts: children whose d' was used, children that fell back to d.
// Nothing of the product is included or linked.
#include "meshuv_oracle.cpp"

namespace gloss {

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kSalt = 0x13198A2E03707344ull;
constexpr uint32_t kDraws = 32;

struct Table {
  std::vector<double> reflection, transmission;  // per material row (mat_* order); a leaf's row: bump::Table::mat_of
  uint64_t seed = 0;
};

std::atomic<uint64_t> g_used{0}, g_fell{0};

uint64_t mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint64_t keyOf(uint64_t seed) { return mix64(seed ^ kSalt); }
uint64_t sampleKey(uint64_t key, uint64_t p, uint64_t g) { return mix64(key + kGold * (((p << 32) | (g << 8)) + 1ull)); }
double jitter(uint64_t h, uint64_t code, uint64_t axis) {
  return static_cast<double>(mix64(h + kGold * (((code << 8) | axis) + 1ull)) >> 11) * 0x1.0p-53;
}

// The sampler: the first of the 32 triples inside the unit ball; none: (0, 0, 0).  J(axis) -> a draw in [0, 1).
template <class F>
void sampleBall(F&& J, double s[3]) {
  s[0] = s[1] = s[2] = 0.0;
  for (uint32_t t = 0; t < kDraws; ++t) {
    const double a = 2.0 * J(3 * t + 0) - 1.0;
    const double b = 2.0 * J(3 * t + 1) - 1.0;
    const double c = 2.0 * J(3 * t + 2) - 1.0;
    if (((a * a) + (b * b)) + (c * c) <= 1.0) {
      s[0] = a;
      s[1] = b;
      s[2] = c;
      return;
    }
  }
}

// The child direction of (d, ng, roughness, s): d' when it lies on the child's side of ng, else d.  *used: which.
orc::Tuple childDirection(orc::Tuple d, orc::Tuple ng, double roughness, const double s[3], bool below, bool* used) {
  const double ex = d.x + s[0] * roughness, ey = d.y + s[1] * roughness, ez = d.z + s[2] * roughness;
  const double m = std::sqrt((ex * ex + ey * ey) + ez * ez);
  *used = false;
  if (m == 0.0) return d;
  const double ux = ex / m, uy = ey / m, uz = ez / m;
  const double side = (ux * ng.x + uy * ng.y) + uz * ng.z;
  if (below ? side < 0.0 : side > 0.0) {
    *used = true;
    return orc::vec3(ux, uy, uz);
  }
  return d;
}

struct Ctx {
  uint64_t h = 0;  // the camera sample's hash
};

orc::Tuple scatter(const Ctx& X, uint64_t code, double roughness, orc::Tuple d, orc::Tuple ng, bool below) {
  double s[3];
  sampleBall([&](uint32_t axis) { return jitter(X.h, code, axis); }, s);
  bool used;
  const orc::Tuple r = childDirection(d, ng, roughness, s, below, &used);
  (used ? g_used : g_fell).fetch_add(1, std::memory_order_relaxed);
  return r;
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const Table& G, const Ctx& X, const orc::Ray& ray, uint64_t code,
                   size_t remaining, const area::Jitter& J);

// meshuv::shadeHit with the path code and the scattered children; ng: the geometric normal after its `inside` flip
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const Table& G, const Ctx& X, const meshuv::Hit& H,
                    const orc::PreComputations& comps, orc::Tuple ng, uint64_t code, size_t remaining, const area::Jitter& J) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  for (uint32_t l = 0; l < S.lights.size(); ++l) {
    const area::Light& L = S.lights[l];
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    if (!L.is_area) {
      const orc::Tuple point_to_light = orc::normalized(orc::sub(L.corner, comps.over_point));
      const double f = spot::coneFactor(K[l], point_to_light);
      if (f == 0.0) {
        surface = orc::cadd(surface, orc::cmul(orc::cemul(color, L.intensity), m.ambient));
        continue;
      }
      const bool shadowed = torus::isShadowed(S, M, Q, comps.over_point, L.corner);
      surface = orc::cadd(surface, spot::spotLighting(m, color, L, point_to_light, comps.eyev, comps.normal, shadowed, f));
    } else {
      surface = orc::cadd(surface, torus::areaLighting(S, M, Q, m, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  double rough_r = 0.0, rough_t = 0.0;
  if (!G.reflection.empty()) {
    const auto it = T.mat_of.find(obj->id);
    if (it == T.mat_of.end()) throw std::runtime_error("gloss checker: a hit on a shape that is no leaf of the description");
    rough_r = G.reflection[it->second];
    rough_t = G.transmission[it->second];
  }
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    orc::Tuple d = comps.reflectv;
    if (rough_r > 0.0) d = scatter(X, 2 * code, rough_r, d, ng, false);
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, X, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J), m.reflective);
  }
  {  // world.zig:171-189
    const double n_ratio = comps.n1 / comps.n2;
    const double cos_i = orc::dot(comps.eyev, comps.normal);
    const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
    if (!(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0) {
      const double cos_t = std::sqrt(1.0 - sin2_t);
      orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
      orc::counters().secondary++;
      if (rough_t > 0.0) direction = scatter(X, 2 * code + 1, rough_t, direction, ng, true);
      refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, X, orc::Ray{comps.under_point, direction}, 2 * code + 1, remaining - 1, J),
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
                   const torus::Table& Q, const meshuv::Table& U, const Table& G, const Ctx& X, const orc::Ray& ray, uint64_t code,
                   size_t remaining, const area::Jitter& J) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  if (h < 0) return {0.0, 0.0, 0.0};
  const meshuv::Hit H = meshuv::hitOf(M, U, xs[h], ray);
  const orc::PreComputations comps = torus::precompute(M, T, Q, xs[h], ray, xs);
  // the geometric normal (torus::precompute's first step), negated by the same `inside`
  orc::Tuple ng = torus::normalAt(Q, xs[h].object, motion::shift(comps.point, M.t, motion::dispOf(M, xs[h].object)), xs[h]);
  if (comps.inside) ng = orc::negate(ng);
  return shadeHit(S, M, K, T, Q, U, G, X, H, comps, ng, code, remaining, J);
}

// meshuv::render's pixel loop with gloss::colorAt; counters_out [primary, secondary, shadow calls, d' used, fell back to d]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const Table& G, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
           uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const motion::Motion base = motion::make(S, disp, n_roots);
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if ((static_cast<uint64_t>(pass) + 1) * n_samples > (1ull << 24)) throw std::runtime_error("InvalidArgument: pass");
    const uint64_t n_pixels = static_cast<uint64_t>(cam->hsize) * cam->vsize;
    const uint64_t key = keyOf(G.seed);
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    g_used = 0;
    g_fell = 0;
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
              Ctx X;
              X.h = sampleKey(key, p, g);
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, X, motion::passRay(camera, smp, x, y, k, g), 1, max_depth, J));
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
      counters_out[3] = g_used.load();
      counters_out[4] = g_fell.load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace gloss

extern "C" {

// The roughness rows (NULL: all zeros; n_materials 0: no table at all) and the seed.  Refuses what rtc_scene_set_gloss refuses.
int gloss_table_create(uint32_t n_materials, const double* reflection, const double* transmission, uint64_t seed, void** out) {
  try {
    auto t = std::make_unique<gloss::Table>();
    t->reflection.assign(n_materials, 0.0);
    t->transmission.assign(n_materials, 0.0);
    for (uint32_t i = 0; i < n_materials; ++i) {
      if (reflection) t->reflection[i] = reflection[i];
      if (transmission) t->transmission[i] = transmission[i];
      for (const double v : {t->reflection[i], t->transmission[i]})
        if (!std::isfinite(v) || v < 0.0 || v > 1.0) throw std::runtime_error("InvalidArgument: a roughness outside [0, 1]");
    }
    t->seed = seed;
    *out = t.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void gloss_table_destroy(void* t) { delete static_cast<gloss::Table*>(t); }

// The scene, the bump, torus and texture tables: as meshuv_render's; and the gloss table.  counters_out: 5 entries.
int gloss_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed,
                 const rtc_sampling* sampling, uint32_t pass, const double* disp, uint32_t n_roots, const uint8_t* cone, const double* axis,
                 const double* cos_inner, const double* cos_outer, uint32_t n_lights, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                 uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  std::vector<spot::Cone> cones;
  try {
    cones = spot::make(S, cone, axis, cos_inner, cos_outer, n_lights);
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
  return gloss::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                       *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl), x0, y0, w,
                       h, n_threads, rgb_out, counters_out);
}

// ---- KAT hooks
// the sampler given its 96 draws (each in [0, 1)): n sets, draws [n][96] -> s [n][3]
void gloss_kat_sampler_many(const double* draws, uint32_t n, double* s_out) {
  for (uint32_t i = 0; i < n; ++i) {
    const double* D = draws + 96ull * i;
    gloss::sampleBall([&](uint32_t axis) { return D[axis]; }, s_out + 3ull * i);
  }
}
// J(axis) of (seed, p, g, code): n entries each
void gloss_kat_jitter_many(uint64_t seed, const uint64_t* p, const uint64_t* g, const uint64_t* code, const uint64_t* axis, uint32_t n,
                           double* out) {
  const uint64_t key = gloss::keyOf(seed);
  for (uint32_t i = 0; i < n; ++i) out[i] = gloss::jitter(gloss::sampleKey(key, p[i], g[i]), code[i], axis[i]);
}
// the child direction of (d, ng, roughness, draws[96]); below: the refracted child's side rule.  -> out[3], *used
void gloss_kat_child(const double* d, const double* ng, double roughness, const double* draws, uint32_t below, double* out, uint32_t* used) {
  double s[3];
  gloss::sampleBall([&](uint32_t axis) { return draws[axis]; }, s);
  bool u;
  const orc::Tuple r = gloss::childDirection(orc::vec3(d[0], d[1], d[2]), orc::vec3(ng[0], ng[1], ng[2]), roughness, s, below != 0, &u);
  out[0] = r.x;
  out[1] = r.y;
  out[2] = r.z;
  *used = u ? 1u : 0u;
}

}  // extern "C"
