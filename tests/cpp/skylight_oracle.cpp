// skylight_oracle.cpp — CPU checker of the sky light (libskylight_oracle.so).  TEST INFRASTRUCTURE.
//
// Hemisphere rays that reach the sky light diffuse surfaces (include/rtc.h rtc_scene_set_sky_light) on
// top of the environment checker: environment_oracle.cpp is included, read-only, and with it every checker below it and the
// oracle's sources.  What is restated here is what names the recursion:
//   - shadeHit, as environment_oracle.cpp has it, with the sky-light step after the suns' loop: `samples` directions by
//     occl::direction from this table's key, each walked by env::sunTransmittance - a sun's shadow ray: every entry with
//     t >= 0 on a casts_shadow shape multiplies its filter row -, and where that is not zero env::sky at the direction;
//     the mean times the gain times colour * diffuse is added to the surface term;
//   - colorAt and the pass loop, which name it.
// With no table, a gain of zero or an environment without a sky the step is skipped whole: the render is env::render's bit
// for bit.  Five counters beside the environment checker's: samples whose transmittance is one, is filtered, is zero; hits
// the step skips because the material has no diffuse term; hits of the step at a path code above 1 (a secondary ray's).
// Nothing of the product is included or linked.
#include "environment_oracle.cpp"

namespace skyl {

constexpr uint64_t kSalt = 0x082EFA98EC4E6C89ull;
constexpr uint32_t kMaxSamples = RTC_SKY_LIGHT_MAX_SAMPLES;

struct Table {
  double gain = 0.0;
  uint32_t samples = 1;
  uint64_t seed = 0;
};

std::atomic<uint64_t> g_clear{0}, g_partial{0}, g_blocked{0}, g_skipped{0}, g_deep{0};

uint64_t keyOf(uint64_t seed) { return gloss::mix64(seed ^ kSalt); }

bool hasSky(const env::Table& E) {
  return E.present && (E.pattern != env::kNoPattern || E.rgb[0] != 0.0 || E.rgb[1] != 0.0 || E.rgb[2] != 0.0);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const env::Table& E, const Table& Y, const gloss::Ctx& X, const gloss::Ctx& XO, const gloss::Ctx& XY,
                   const orc::Ray& ray, uint64_t code,
                   size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t level, uint32_t kind, bool rough_parent);

// env::shadeHit with the sky-light step after the suns' loop, and skyl::colorAt
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                    const media::Table& A, const env::Table& E, const Table& Y, const gloss::Ctx& X, const gloss::Ctx& XO, const gloss::Ctx& XY,
                    const meshuv::Hit& H,
                    const orc::PreComputations& comps, orc::Tuple ng, uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium,
                    uint32_t kid_medium, bool kid_nested, uint32_t level) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  // ---- the occlusion step (rtc.h): once per hit, before the lights; its rays stay binary, are not attenuated, see no sky
  double ka = m.ambient;
  if (!O.radius.empty()) {
    const double radius = O.radius[media::materialOf(T, obj)];
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
  const bool shadow_matters = !(m.diffuse == 0.0 && m.specular == 0.0);
  bool lit_by_light = false;  // a light of World.lights reaches the hit: in front of the surface and not blocked
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
      const bool traced = shadow_matters && orc::dot(point_to_light, comps.normal) >= 0.0;
      const sfilt::Trans t = sfilt::transmittance(S, M, T, Q, F, comps.over_point, L.corner, traced);
      lit_by_light = lit_by_light || (traced && !t.blocked());
      surface = orc::cadd(surface, sfilt::pointLighting(*ml, color, L, point_to_light, comps.eyev, comps.normal, t, f));
    } else {
      lit_by_light = true;  // (an area light: not looked into)
      surface = orc::cadd(surface, sfilt::areaLighting(S, M, T, Q, F, *ml, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  // ---- the suns (rtc.h): after World.lights, in table order; no cone, no far end
  bool lit_by_sun = false;
  for (const env::Sun& sun : E.suns) {
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    const double light_dot_normal = orc::dot(sun.lv, comps.normal);
    const bool traced = shadow_matters && light_dot_normal >= 0.0;
    if (shadow_matters && !(light_dot_normal >= 0.0)) env::g_sun_behind.fetch_add(1, std::memory_order_relaxed);
    const sfilt::Trans t = env::sunTransmittance(S, M, T, Q, F, comps.over_point, sun.lv, traced);
    lit_by_sun = lit_by_sun || (traced && !t.blocked());
    area::Light L{};
    L.intensity = sun.rgb;
    surface = orc::cadd(surface, sfilt::pointLighting(*ml, color, L, sun.lv, comps.eyev, comps.normal, t, 1.0));
  }
  if (lit_by_sun && !lit_by_light) env::g_sun_only.fetch_add(1, std::memory_order_relaxed);
  // ---- the sky light (rtc.h): once per hit, after the last sun's term; its rays are a sun's shadow rays - no far end, the
  // filter rows multiply, no medium dims them - along the occlusion step's directions, drawn from this table's key
  if (Y.gain > 0.0 && hasSky(E)) {
    if (m.diffuse == 0.0) {
      g_skipped.fetch_add(1, std::memory_order_relaxed);
    } else {
      if (code > 1) g_deep.fetch_add(1, std::memory_order_relaxed);
      const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
      double L[3] = {0.0, 0.0, 0.0};
      for (uint32_t k = 0; k < Y.samples; ++k) {
        const uint64_t word = (static_cast<uint64_t>(k) << occl::kSampleShift) | code;
        const orc::Tuple d = occl::direction([&](uint32_t axis) { return gloss::jitter(XY.h, word, axis); }, ng);
        const sfilt::Trans t = env::sunTransmittance(S, M, T, Q, F, comps.over_point, d, false);
        if (t.blocked()) {
          g_blocked.fetch_add(1, std::memory_order_relaxed);
          continue;
        }
        (t.r == 1.0 && t.g == 1.0 && t.b == 1.0 ? g_clear : g_partial).fetch_add(1, std::memory_order_relaxed);
        const orc::Color e = env::sky(S, U, E, orc::Ray{comps.over_point, d});
        L[0] = L[0] + t.r * e.r;
        L[1] = L[1] + t.g * e.g;
        L[2] = L[2] + t.b * e.b;
      }
      const double n = static_cast<double>(Y.samples);
      const orc::Color gathered{Y.gain * (L[0] / n), Y.gain * (L[1] / n), Y.gain * (L[2] / n)};
      surface = orc::cadd(surface, orc::Color{(color.r * m.diffuse) * gathered.r, (color.g * m.diffuse) * gathered.g, (color.b * m.diffuse) * gathered.b});
    }
  }
  double rough_r = 0.0, rough_t = 0.0;
  if (!G.reflection.empty()) {
    const uint32_t mi = media::materialOf(T, obj);
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
    if (A.any() && medium != media::kNoMedium) media::g_reflect_in_medium.fetch_add(1, std::memory_order_relaxed);
    orc::Tuple d = comps.reflectv;
    if (rough_r > 0.0) d = gloss::scatter(X, 2 * code, rough_r, d, ng, false);
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, X, XO, XY, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                  level + (do_refract ? 1u : 0u), env::kReflected, rough_r > 0.0),
                          m.reflective);
  }
  if (do_refract) {  // world.zig:171-189: in the medium that supplied n2
    const double cos_t = std::sqrt(1.0 - sin2_t);
    orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
    orc::counters().secondary++;
    if (A.any()) {
      if (kid_nested) media::g_nested.fetch_add(1, std::memory_order_relaxed);
      if (kid_medium == media::kNoMedium) media::g_exit.fetch_add(1, std::memory_order_relaxed);
    }
    if (do_reflect && level >= 2u) media::g_deep.fetch_add(1, std::memory_order_relaxed);
    if (rough_t > 0.0) direction = gloss::scatter(X, 2 * code + 1, rough_t, direction, ng, true);
    refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, X, XO, XY, orc::Ray{comps.under_point, direction}, 2 * code + 1,
                                  remaining - 1, J, kid_medium, level, env::kRefracted, rough_t > 0.0),
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
                   const media::Table& A, const env::Table& E, const Table& Y, const gloss::Ctx& X, const gloss::Ctx& XO, const gloss::Ctx& XY,
                   const orc::Ray& ray, uint64_t code,
                   size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t level, uint32_t kind, bool rough_parent) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  // ---- the media step (rtc.h): after the closest-hit search, whatever `remaining`; without a table it is not there at all
  media::Step st;
  if (A.any()) st = media::segment(A, medium, ray, h >= 0, h >= 0 ? xs[h].t : 0.0);
  if (h < 0) {
    const orc::Color in = st.fog ? orc::Color{st.in[0], st.in[1], st.in[2]} : orc::Color{0.0, 0.0, 0.0};
    const bool has_sky = E.present && (E.pattern != env::kNoPattern || E.rgb[0] != 0.0 || E.rgb[1] != 0.0 || E.rgb[2] != 0.0);
    if (!has_sky) return in;
    // ---- the miss step (rtc.h): after the media step, the sky's colour times the miss transmittance
    orc::Color e = env::sky(S, U, E, ray);
    if (A.any()) e = {e.r * st.t[0], e.g * st.t[1], e.b * st.t[2]};
    if (st.t[0] == 0.0 && st.t[1] == 0.0 && st.t[2] == 0.0) {
      env::g_miss_dark.fetch_add(1, std::memory_order_relaxed);
    } else {
      (kind == env::kCamera ? env::g_miss_camera : (kind == env::kReflected ? env::g_miss_reflected : env::g_miss_refracted)).fetch_add(1, std::memory_order_relaxed);
      if (rough_parent) env::g_miss_rough.fetch_add(1, std::memory_order_relaxed);
    }
    return st.fog ? orc::Color{in.r + e.r, in.g + e.g, in.b + e.b} : e;
  }
  const meshuv::Hit H = meshuv::hitOf(M, U, xs[h], ray);
  const orc::PreComputations comps = torus::precompute(M, T, Q, xs[h], ray, xs);
  orc::Tuple ng = torus::normalAt(Q, xs[h].object, motion::shift(comps.point, M.t, motion::dispOf(M, xs[h].object)), xs[h]);
  if (comps.inside) ng = orc::negate(ng);
  // the refracted child's medium: the shape that supplied n2
  uint32_t kid_medium = media::kNoMedium;
  bool kid_nested = false;
  const orc::Shape* s2 = media::n2Shape(xs[h], xs);
  if ((s2 ? s2->material.refractive_index : 1.0) != comps.n2) throw std::runtime_error("sky-light checker: the containers walk disagrees with n2");
  if (s2) {
    kid_medium = media::materialOf(T, s2);
    kid_nested = s2->id != xs[h].object->id;
  }
  const orc::Color c = shadeHit(S, M, K, T, Q, U, G, O, F, A, E, Y, X, XO, XY, H, comps, ng, code, remaining, J, medium, kid_medium, kid_nested, level);
  if (!A.any()) return c;
  orc::Color out{c.r * st.t[0], c.g * st.t[1], c.b * st.t[2]};
  if (st.fog) out = {st.in[0] + out.r, st.in[1] + out.g, st.in[2] + out.b};
  return out;
}

// env::render's pixel loop with skyl::colorAt; counters_out: env::render's 32, then [sky-light samples with T == 1, with a
// filtered T, with T == 0, hits the step skips for diffuse == 0, hits of the step at a path code above 1]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
           const media::Table& A, const env::Table& E, const Table& Y, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out,
           uint64_t* counters_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const motion::Motion base = motion::make(S, disp, n_roots);
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if ((static_cast<uint64_t>(pass) + 1) * n_samples > (1ull << 24)) throw std::runtime_error("InvalidArgument: pass");
    const uint64_t n_pixels = static_cast<uint64_t>(cam->hsize) * cam->vsize;
    const uint64_t key = gloss::keyOf(G.seed), okey = occl::keyOf(O.seed), ykey = keyOf(Y.seed);
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
    media::g_seg_atmosphere = 0;
    media::g_seg_medium = 0;
    media::g_seg_tinted = 0;
    media::g_miss_in_medium = 0;
    media::g_reflect_in_medium = 0;
    media::g_nested = 0;
    media::g_exit = 0;
    media::g_deep = 0;
    env::g_miss_camera = 0;
    env::g_miss_reflected = 0;
    env::g_miss_refracted = 0;
    env::g_miss_rough = 0;
    env::g_miss_dark = 0;
    env::g_sun_clear = 0;
    env::g_sun_blocked = 0;
    env::g_sun_partial = 0;
    env::g_sun_behind = 0;
    env::g_sun_only = 0;
    g_clear = 0;
    g_partial = 0;
    g_blocked = 0;
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
              gloss::Ctx X, XO, XY;
              X.h = gloss::sampleKey(key, p, g);
              XO.h = gloss::sampleKey(okey, p, g);
              XY.h = gloss::sampleKey(ykey, p, g);
              // (a camera ray is in the atmosphere: the camera stands outside every solid)
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, O, F, A, E, Y, X, XO, XY, motion::passRay(camera, smp, x, y, k, g), 1, max_depth,
                                           J, media::kNoMedium, 0u, env::kCamera, false));
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
      counters_out[14] = media::g_seg_atmosphere.load();
      counters_out[15] = media::g_seg_medium.load();
      counters_out[16] = media::g_seg_tinted.load();
      counters_out[17] = media::g_miss_in_medium.load();
      counters_out[18] = media::g_reflect_in_medium.load();
      counters_out[19] = media::g_nested.load();
      counters_out[20] = media::g_exit.load();
      counters_out[21] = media::g_deep.load();
      counters_out[22] = env::g_miss_camera.load();
      counters_out[23] = env::g_miss_reflected.load();
      counters_out[24] = env::g_miss_refracted.load();
      counters_out[25] = env::g_miss_rough.load();
      counters_out[26] = env::g_miss_dark.load();
      counters_out[27] = env::g_sun_clear.load();
      counters_out[28] = env::g_sun_blocked.load();
      counters_out[29] = env::g_sun_partial.load();
      counters_out[30] = env::g_sun_behind.load();
      counters_out[31] = env::g_sun_only.load();
      counters_out[32] = g_clear.load();
      counters_out[33] = g_partial.load();
      counters_out[34] = g_blocked.load();
      counters_out[35] = g_skipped.load();
      counters_out[36] = g_deep.load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace skyl

extern "C" {

// The sky light (y NULL: no table).  Refuses what rtc_scene_set_sky_light refuses.
int skyl_table_create(const rtc_sky_light* y, void** out) {
  try {
    auto t = std::make_unique<skyl::Table>();
    if (y) {
      if (!std::isfinite(y->gain) || y->gain < 0.0) throw std::runtime_error("InvalidArgument: a gain that is not finite or is negative");
      if (y->samples < 1 || y->samples > skyl::kMaxSamples) throw std::runtime_error("InvalidArgument: samples");
      t->gain = y->gain;
      t->samples = y->samples;
      t->seed = y->seed;
    }
    *out = t.release();
    return 0;
  } catch (const std::exception& ex) {
    g_error = ex.what();
    return 1;
  }
}
void skyl_table_destroy(void* t) { delete static_cast<skyl::Table*>(t); }

// The scene and the tables: as env_render's; and the sky-light table.  counters_out: 37 entries.
int skyl_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, void* sf, void* me, void* ev, void* sl,
                const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling, uint32_t pass,
                const double* disp, uint32_t n_roots, const uint8_t* cone, const double* axis, const double* cos_inner,
                const double* cos_outer, uint32_t n_lights, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads,
                double* rgb_out, uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  std::vector<spot::Cone> cones;
  try {
    cones = spot::make(S, cone, axis, cos_inner, cos_outer, n_lights);
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
  return skyl::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                      *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                      *static_cast<occl::Table*>(oc), *static_cast<sfilt::Table*>(sf), *static_cast<media::Table*>(me),
                      *static_cast<env::Table*>(ev), *static_cast<skyl::Table*>(sl), x0, y0, w, h, n_threads, rgb_out, counters_out);
}

}  // extern "C"
