// media_oracle.cpp — CPU checker of participating media (libmedia_oracle.so).  TEST INFRASTRUCTURE.
//
// Absorbing materials and a uniform fog (include/rtc.h rtc_scene_set_media) on top of the
// shadow-filter checker: sfilter_oracle.cpp is included, read-only, and with it the occlusion, gloss, mesh-texture, torus,
// bump, spot, motion, camera-sampling and area-light checkers and the oracle's sources.  What is restated here is what the
// feature changes:
//   - a medium carried down the colorAt recursion: the atmosphere for a camera ray, the parent's for a reflected child, and
//     for a refracted child the shape the containers walk of PreComputations.new leaves last when it sets n2 - walked here
//     again over the same sorted list, and held to comps.n2;
//   - the step of rtc.h after every closest-hit search: the segment's transmittance per channel (std::exp), the fog's
//     in-scatter in the atmosphere, and the returned colour times the transmittance - the recursion's form of W.c * T.c;
//   - shadeHit, colorAt and the pass loop, as sfilter_oracle.cpp has them, because they name the recursion.
// With no table the step is skipped whole: the render is sfilt::render's bit for bit.  The lights' transmittances, the
// occlusion rays and every draw are the shadow-filter checker's own functions.
// Eight counters beside the shadow-filter checker's: segments in the atmosphere and in a material; segments with some
// T.c != 1; misses with a non-zero sigma; reflected children spawned with a material medium; refracted children whose medium
// is not the hit shape's material (a container's); refracted children whose medium is the atmosphere; and refracted children
// that wait for a reflected sibling with two or more such waiting on their path already (`deep`: the third level of a
// lane's stack of pending rays, or a deeper one).
// Nothing of the product is included or linked.
#include "sfilter_oracle.cpp"

namespace media {

constexpr uint32_t kNoMedium = RTC_NO_MEDIUM;

struct Table {
  std::vector<double> absorption;  // three per material row (mat_* order); empty with no fog: no table
  double fog_density = 0.0;
  double fog_color[3] = {0.0, 0.0, 0.0};
  bool any() const { return !absorption.empty() || fog_density != 0.0; }
};

std::atomic<uint64_t> g_seg_atmosphere{0}, g_seg_medium{0}, g_seg_tinted{0}, g_miss_in_medium{0}, g_reflect_in_medium{0}, g_nested{0},
    g_exit{0}, g_deep{0};

uint32_t materialOf(const bump::Table& T, const orc::Shape* s) {
  const auto it = T.mat_of.find(s->id);
  if (it == T.mat_of.end()) throw std::runtime_error("media checker: a shape that is no leaf of the description");
  return it->second;
}

// The shape whose refractive index PreComputations.new takes for n2 (world.zig:229-255), or null where n2 stays 1.0: the
// walk again, over the same list.
const orc::Shape* n2Shape(const orc::Intersection& hit, const orc::Intersections& xs) {
  std::vector<const orc::Shape*> containers;
  const orc::Shape* last = nullptr;
  for (const orc::Intersection& item : xs) {
    const bool is_hit = item.t == hit.t && item.object->id == hit.object->id;
    bool removed = false;
    for (size_t i = 0; i < containers.size(); ++i)
      if (containers[i]->id == item.object->id) {
        containers.erase(containers.begin() + static_cast<long>(i));
        removed = true;
        break;
      }
    if (!removed) containers.push_back(item.object);
    if (is_hit && !containers.empty()) {
      last = containers.back();
      break;
    }
  }
  return last;
}

struct Step {
  double t[3] = {1.0, 1.0, 1.0};
  double in[3] = {0.0, 0.0, 0.0};  // the fog's in-scatter, formed only in the atmosphere with a density above zero
  bool fog = false;
};

// rtc.h's step for one segment: `hit` with its t, or a miss
Step segment(const Table& A, uint32_t medium, const orc::Ray& ray, bool hit, double t) {
  Step s;
  double sigma[3] = {A.fog_density, A.fog_density, A.fog_density};
  if (medium != kNoMedium) {
    g_seg_medium.fetch_add(1, std::memory_order_relaxed);
    for (int c = 0; c < 3; ++c) sigma[c] = A.absorption.empty() ? 0.0 : A.absorption[3 * static_cast<size_t>(medium) + c];
  } else {
    g_seg_atmosphere.fetch_add(1, std::memory_order_relaxed);
  }
  if (hit) {
    const orc::Tuple d = ray.direction;
    const double dist = t * std::sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
    for (int c = 0; c < 3; ++c) s.t[c] = sigma[c] == 0.0 ? 1.0 : std::exp(-(sigma[c] * dist));
  } else {
    for (int c = 0; c < 3; ++c) s.t[c] = sigma[c] == 0.0 ? 1.0 : 0.0;
    if (sigma[0] != 0.0 || sigma[1] != 0.0 || sigma[2] != 0.0) g_miss_in_medium.fetch_add(1, std::memory_order_relaxed);
  }
  if (s.t[0] != 1.0 || s.t[1] != 1.0 || s.t[2] != 1.0) g_seg_tinted.fetch_add(1, std::memory_order_relaxed);
  if (medium == kNoMedium && A.fog_density > 0.0) {
    s.fog = true;
    for (int c = 0; c < 3; ++c) s.in[c] = (1.0 - s.t[c]) * A.fog_color[c];
  }
  return s;
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const Table& A, const gloss::Ctx& X, const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code, size_t remaining,
                   const area::Jitter& J, uint32_t medium, uint32_t level);

// sfilt::shadeHit with the children's media
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                    const Table& A, const gloss::Ctx& X, const gloss::Ctx& XO, const meshuv::Hit& H, const orc::PreComputations& comps,
                    orc::Tuple ng, uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t kid_medium,
                    bool kid_nested, uint32_t level) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  // ---- the occlusion step (rtc.h): once per hit, before the lights; its rays stay binary and are not attenuated
  double ka = m.ambient;
  if (!O.radius.empty()) {
    const double radius = O.radius[materialOf(T, obj)];
    if (radius > 0.0 && m.ambient == 0.0) occl::g_skipped.fetch_add(1, std::memory_order_relaxed);
    if (radius > 0.0 && m.ambient != 0.0) {
      if (code > 1) occl::g_deep.fetch_add(1, std::memory_order_relaxed);
      uint32_t n_occluded = 0;
      for (uint32_t k = 0; k < O.samples; ++k) {
        const uint64_t word = (static_cast<uint64_t>(k) << occl::kSampleShift) | code;
        const orc::Tuple d = occl::direction([&](uint32_t axis) { return gloss::jitter(XO.h, word, axis); }, ng);
        if (occl::occluded(S, M, Q, comps.over_point, d, radius)) ++n_occluded;
      }
      occl::g_occluded.fetch_add(n_occluded, std::memory_order_relaxed);
      occl::g_clear.fetch_add(O.samples - n_occluded, std::memory_order_relaxed);
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
  for (uint32_t l = 0; l < S.lights.size(); ++l) {  // (the lights' shadow rays are not attenuated by media)
    const area::Light& L = S.lights[l];
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    if (!L.is_area) {
      const orc::Tuple point_to_light = orc::normalized(orc::sub(L.corner, comps.over_point));
      const double f = spot::coneFactor(K[l], point_to_light);
      if (f == 0.0) {
        surface = orc::cadd(surface, orc::cmul(orc::cemul(color, L.intensity), ka));
        continue;
      }
      const bool traced = !(m.diffuse == 0.0 && m.specular == 0.0) && orc::dot(point_to_light, comps.normal) >= 0.0;
      const sfilt::Trans t = sfilt::transmittance(S, M, T, Q, F, comps.over_point, L.corner, traced);
      surface = orc::cadd(surface, sfilt::pointLighting(*ml, color, L, point_to_light, comps.eyev, comps.normal, t, f));
    } else {
      surface = orc::cadd(surface, sfilt::areaLighting(S, M, T, Q, F, *ml, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  double rough_r = 0.0, rough_t = 0.0;
  if (!G.reflection.empty()) {
    const uint32_t mi = materialOf(T, obj);
    rough_r = G.reflection[mi];
    rough_t = G.transmission[mi];
  }
  const bool do_reflect = remaining != 0 && m.reflective != 0.0;
  const double n_ratio = comps.n1 / comps.n2;
  const double cos_i = orc::dot(comps.eyev, comps.normal);
  const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
  const bool do_refract = !(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0;
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (do_reflect) {  // world.zig:157-167: in its parent's medium
    orc::counters().secondary++;
    if (A.any() && medium != kNoMedium) g_reflect_in_medium.fetch_add(1, std::memory_order_relaxed);
    orc::Tuple d = comps.reflectv;
    if (rough_r > 0.0) d = gloss::scatter(X, 2 * code, rough_r, d, ng, false);
    // (where both children are spawned the refracted one waits on the lane's stack while the reflected sub-tree runs)
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, X, XO, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                  level + (do_refract ? 1u : 0u)),
                          m.reflective);
  }
  if (do_refract) {  // world.zig:171-189: in the medium that supplied n2
    const double cos_t = std::sqrt(1.0 - sin2_t);
    orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
    orc::counters().secondary++;
    if (A.any()) {
      if (kid_nested) g_nested.fetch_add(1, std::memory_order_relaxed);
      if (kid_medium == kNoMedium) g_exit.fetch_add(1, std::memory_order_relaxed);
    }
    if (do_reflect && level >= 2u) g_deep.fetch_add(1, std::memory_order_relaxed);
    if (rough_t > 0.0) direction = gloss::scatter(X, 2 * code + 1, rough_t, direction, ng, true);
    refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, X, XO, orc::Ray{comps.under_point, direction}, 2 * code + 1, remaining - 1,
                                  J, kid_medium, level),
                          m.transparency);
  }
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const Table& A, const gloss::Ctx& X, const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code, size_t remaining,
                   const area::Jitter& J, uint32_t medium, uint32_t level) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  // ---- the step (rtc.h): after the closest-hit search, whatever `remaining`; without a table it is not there at all
  Step st;
  if (A.any()) st = segment(A, medium, ray, h >= 0, h >= 0 ? xs[h].t : 0.0);
  if (h < 0) return st.fog ? orc::Color{st.in[0], st.in[1], st.in[2]} : orc::Color{0.0, 0.0, 0.0};
  const meshuv::Hit H = meshuv::hitOf(M, U, xs[h], ray);
  const orc::PreComputations comps = torus::precompute(M, T, Q, xs[h], ray, xs);
  orc::Tuple ng = torus::normalAt(Q, xs[h].object, motion::shift(comps.point, M.t, motion::dispOf(M, xs[h].object)), xs[h]);
  if (comps.inside) ng = orc::negate(ng);
  // the refracted child's medium: the shape that supplied n2
  uint32_t kid_medium = kNoMedium;
  bool kid_nested = false;
  const orc::Shape* s2 = n2Shape(xs[h], xs);
  if ((s2 ? s2->material.refractive_index : 1.0) != comps.n2) throw std::runtime_error("media checker: the containers walk disagrees with n2");
  if (s2) {
    kid_medium = materialOf(T, s2);
    kid_nested = s2->id != xs[h].object->id;
  }
  const orc::Color c = shadeHit(S, M, K, T, Q, U, G, O, F, A, X, XO, H, comps, ng, code, remaining, J, medium, kid_medium, kid_nested, level);
  if (!A.any()) return c;
  orc::Color out{c.r * st.t[0], c.g * st.t[1], c.b * st.t[2]};
  if (st.fog) out = {st.in[0] + out.r, st.in[1] + out.g, st.in[2] + out.b};
  return out;
}

// sfilt::render's pixel loop with media::colorAt; counters_out: sfilt::render's 14, then [segments in the atmosphere, in a
// material, tinted segments, misses in a medium, reflected children in a material, nested refracted children, refracted
// children into the atmosphere, deep]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
           const Table& A, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out,
           uint64_t* counters_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const motion::Motion base = motion::make(S, disp, n_roots);
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if ((static_cast<uint64_t>(pass) + 1) * n_samples > (1ull << 24)) throw std::runtime_error("InvalidArgument: pass");
    const uint64_t n_pixels = static_cast<uint64_t>(cam->hsize) * cam->vsize;
    const uint64_t key = gloss::keyOf(G.seed), okey = occl::keyOf(O.seed);
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    gloss::g_used = 0;
    gloss::g_fell = 0;
    occl::g_occluded = 0;
    occl::g_clear = 0;
    occl::g_skipped = 0;
    occl::g_deep = 0;
    sfilt::g_clear = 0;
    sfilt::g_partial = 0;
    sfilt::g_blocked = 0;
    sfilt::g_three = 0;
    sfilt::g_three_partial = 0;
    sfilt::g_factors = 0;
    sfilt::g_at_light = 0;
    g_seg_atmosphere = 0;
    g_seg_medium = 0;
    g_seg_tinted = 0;
    g_miss_in_medium = 0;
    g_reflect_in_medium = 0;
    g_nested = 0;
    g_exit = 0;
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
              // (a camera ray is in the atmosphere: the camera stands outside every solid)
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, O, F, A, X, XO, motion::passRay(camera, smp, x, y, k, g), 1, max_depth,
                                           J, kNoMedium, 0u));
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
      counters_out[3] = occl::g_occluded.load();
      counters_out[4] = occl::g_clear.load();
      counters_out[5] = occl::g_skipped.load();
      counters_out[6] = occl::g_deep.load();
      counters_out[7] = sfilt::g_clear.load();
      counters_out[8] = sfilt::g_partial.load();
      counters_out[9] = sfilt::g_blocked.load();
      counters_out[10] = sfilt::g_three.load();
      counters_out[11] = sfilt::g_three_partial.load();
      counters_out[12] = sfilt::g_factors.load();
      counters_out[13] = sfilt::g_at_light.load();
      counters_out[14] = g_seg_atmosphere.load();
      counters_out[15] = g_seg_medium.load();
      counters_out[16] = g_seg_tinted.load();
      counters_out[17] = g_miss_in_medium.load();
      counters_out[18] = g_reflect_in_medium.load();
      counters_out[19] = g_nested.load();
      counters_out[20] = g_exit.load();
      counters_out[21] = g_deep.load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace media

extern "C" {

// The media (absorption NULL: all zeros; n_materials 0, no rows and a density of 0: no table at all).  Refuses what
// rtc_scene_set_media refuses of the table's own values.
int media_table_create(uint32_t n_materials, const double* absorption, double fog_density, const double* fog_color, void** out) {
  try {
    auto t = std::make_unique<media::Table>();
    t->absorption.assign(3 * static_cast<size_t>(n_materials), 0.0);
    for (size_t i = 0; i < t->absorption.size(); ++i) {
      if (absorption) t->absorption[i] = absorption[i];
      if (!std::isfinite(t->absorption[i]) || t->absorption[i] < 0.0)
        throw std::runtime_error("InvalidArgument: an absorption that is not finite or is negative");
    }
    t->fog_density = fog_density;
    for (int c = 0; c < 3; ++c) t->fog_color[c] = fog_color ? fog_color[c] : 0.0;
    if (!std::isfinite(fog_density) || fog_density < 0.0) throw std::runtime_error("InvalidArgument: a fog density that is not finite or is negative");
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(t->fog_color[c]) || t->fog_color[c] < 0.0) throw std::runtime_error("InvalidArgument: a fog colour that is not finite or is negative");
    *out = t.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void media_table_destroy(void* t) { delete static_cast<media::Table*>(t); }

// The scene and the bump, torus, texture, gloss, occlusion and filter tables: as sfilt_render's; and the media table.
// counters_out: 22 entries.
int media_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, void* sf, void* me, const rtc_camera* cam,
                 uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling, uint32_t pass, const double* disp, uint32_t n_roots,
                 const uint8_t* cone, const double* axis, const double* cos_inner, const double* cos_outer, uint32_t n_lights, uint32_t x0,
                 uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  std::vector<spot::Cone> cones;
  try {
    cones = spot::make(S, cone, axis, cos_inner, cos_outer, n_lights);
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
  return media::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                       *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                       *static_cast<occl::Table*>(oc), *static_cast<sfilt::Table*>(sf), *static_cast<media::Table*>(me), x0, y0, w, h,
                       n_threads, rgb_out, counters_out);
}

}  // extern "C"
