// environment_oracle.cpp — CPU checker of the environment (libenvironment_oracle.so).  TEST INFRASTRUCTURE.
//
// A sky behind the world and suns that light it (include/rtc.h rtc_scene_set_environment) on top of
// the participating-media checker: media_oracle.cpp is included, read-only, and with it every checker below it and the
// oracle's sources.  What is restated here is what names the recursion:
//   - shadeHit, as media_oracle.cpp has it, with the suns' loop after World.lights: point_to_light is the sun's unit vector,
//     the shadow walk has no far end - every entry with t >= 0 on a casts_shadow shape counts - and the lighting is
//     sfilt::pointLighting with the sun's intensity, the cone's factor 1;
//   - colorAt with the miss step: the sky's colour at the ray's direction, times the miss transmittance - the recursion's
//     form of W.c * E.c after the media step - and after the fog's in-scatter.
// The sky's pattern is the scene's own pattern row, built by the oracle from the description as a material's pattern is,
// and evaluated by meshuv::patternAt at the point where the direction meets the unit sphere or cube, with no hit triangle.
// With no table both steps are skipped whole: the render is media::render's bit for bit.
// Ten counters beside the media checker's: misses that add a sky term, by the ray's kind - a camera ray, a reflected child,
// a refracted child - and those among the children whose parent's material is rough; misses whose transmittance is zero in
// every channel (in fog or in an absorbing material); the suns' shadow rays by result - clear, blocked, partly filtered -
// and those not traced because the sun is behind the surface; and hits that only a sun lights (every light of World.lights
// blocked or behind the surface, or none there, and a sun's ray traced and not blocked).
// Nothing of the product is included or linked.
#include "media_oracle.cpp"

namespace env {

constexpr uint32_t kNoPattern = RTC_ENV_NO_PATTERN;

struct Sun {
  orc::Tuple lv;  // the unit vector TOWARDS the sun
  orc::Color rgb;
};

struct Table {
  bool present = false;
  double rgb[3] = {0.0, 0.0, 0.0};
  uint32_t pattern = kNoPattern, projection = RTC_ENV_SPHERE;
  std::vector<Sun> suns;
};

enum Kind : uint32_t { kCamera = 0, kReflected = 1, kRefracted = 2 };

std::atomic<uint64_t> g_miss_camera{0}, g_miss_reflected{0}, g_miss_refracted{0}, g_miss_rough{0}, g_miss_dark{0}, g_sun_clear{0},
    g_sun_blocked{0}, g_sun_partial{0}, g_sun_behind{0}, g_sun_only{0};

// rtc.h's sky: E at the direction of a ray that found nothing
orc::Color sky(const area::Scene& S, const meshuv::Table& U, const Table& E, const orc::Ray& ray) {
  if (E.pattern == kNoPattern) return {E.rgb[0], E.rgb[1], E.rgb[2]};
  const orc::Tuple d = ray.direction;
  const double len = E.projection == RTC_ENV_CUBE ? std::max(std::fabs(d.x), std::max(std::fabs(d.y), std::fabs(d.z)))
                                                  : std::sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
  if (E.pattern >= S.os->patterns.size()) throw std::runtime_error("environment checker: a pattern that is no row of the description");
  const meshuv::Hit none;  // (no hit triangle: the row of zeros)
  const orc::Color c = meshuv::patternAt(S, U, none, S.os->patterns[E.pattern], orc::point(d.x / len, d.y / len, d.z / len));
  return {c.r * E.rgb[0], c.g * E.rgb[1], c.b * E.rgb[2]};
}

// sfilt::transmittance of a ray that never ends: the product of the filter rows of every entry with t >= 0 on a
// casts_shadow shape; `traced`: the product traces this ray - it is counted by result
sfilt::Trans sunTransmittance(const area::Scene& S, const motion::Motion& M, const bump::Table& T, const torus::Table& Q, const sfilt::Table& F,
                              orc::Tuple pt, orc::Tuple lv, bool traced) {
  orc::counters().shadow++;
  const orc::Ray shadow_ray{pt, lv};
  const orc::Intersections xs = torus::intersect(S, M, Q, shadow_ray);
  sfilt::Trans t;
  long i = orc::hit(xs);
  while (i >= 0) {
    if (xs[i].object->casts_shadow) {
      double f[3] = {0.0, 0.0, 0.0};
      if (!F.rgb.empty()) {
        const auto it = T.mat_of.find(xs[i].object->id);
        if (it == T.mat_of.end()) throw std::runtime_error("environment checker: an entry of a shape that is no leaf of the description");
        for (int c = 0; c < 3; ++c) f[c] = F.rgb[3 * static_cast<size_t>(it->second) + c];
      }
      t.r = t.r * f[0];
      t.g = t.g * f[1];
      t.b = t.b * f[2];
    }
    i = orc::hit(xs, static_cast<size_t>(i) + 1);
  }
  if (traced) {
    if (t.blocked()) g_sun_blocked.fetch_add(1, std::memory_order_relaxed);
    else if (t.r == 1.0 && t.g == 1.0 && t.b == 1.0) g_sun_clear.fetch_add(1, std::memory_order_relaxed);
    else g_sun_partial.fetch_add(1, std::memory_order_relaxed);
  }
  return t;
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const Table& E, const gloss::Ctx& X, const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code,
                   size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t level, uint32_t kind, bool rough_parent);

// media::shadeHit with the suns' loop and env::colorAt
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                    const media::Table& A, const Table& E, const gloss::Ctx& X, const gloss::Ctx& XO, const meshuv::Hit& H,
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
  for (const Sun& sun : E.suns) {
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    const double light_dot_normal = orc::dot(sun.lv, comps.normal);
    const bool traced = shadow_matters && light_dot_normal >= 0.0;
    if (shadow_matters && !(light_dot_normal >= 0.0)) g_sun_behind.fetch_add(1, std::memory_order_relaxed);
    const sfilt::Trans t = sunTransmittance(S, M, T, Q, F, comps.over_point, sun.lv, traced);
    lit_by_sun = lit_by_sun || (traced && !t.blocked());
    area::Light L{};
    L.intensity = sun.rgb;
    surface = orc::cadd(surface, sfilt::pointLighting(*ml, color, L, sun.lv, comps.eyev, comps.normal, t, 1.0));
  }
  if (lit_by_sun && !lit_by_light) g_sun_only.fetch_add(1, std::memory_order_relaxed);
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
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, X, XO, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                  level + (do_refract ? 1u : 0u), kReflected, rough_r > 0.0),
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
    refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, X, XO, orc::Ray{comps.under_point, direction}, 2 * code + 1,
                                  remaining - 1, J, kid_medium, level, kRefracted, rough_t > 0.0),
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
                   const media::Table& A, const Table& E, const gloss::Ctx& X, const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code,
                   size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t level, uint32_t kind, bool rough_parent) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  // ---- the media step (rtc.h): after the closest-hit search, whatever `remaining`; without a table it is not there at all
  media::Step st;
  if (A.any()) st = media::segment(A, medium, ray, h >= 0, h >= 0 ? xs[h].t : 0.0);
  if (h < 0) {
    const orc::Color in = st.fog ? orc::Color{st.in[0], st.in[1], st.in[2]} : orc::Color{0.0, 0.0, 0.0};
    const bool has_sky = E.present && (E.pattern != kNoPattern || E.rgb[0] != 0.0 || E.rgb[1] != 0.0 || E.rgb[2] != 0.0);
    if (!has_sky) return in;
    // ---- the miss step (rtc.h): after the media step, the sky's colour times the miss transmittance
    orc::Color e = sky(S, U, E, ray);
    if (A.any()) e = {e.r * st.t[0], e.g * st.t[1], e.b * st.t[2]};
    if (st.t[0] == 0.0 && st.t[1] == 0.0 && st.t[2] == 0.0) {
      g_miss_dark.fetch_add(1, std::memory_order_relaxed);
    } else {
      (kind == kCamera ? g_miss_camera : (kind == kReflected ? g_miss_reflected : g_miss_refracted)).fetch_add(1, std::memory_order_relaxed);
      if (rough_parent) g_miss_rough.fetch_add(1, std::memory_order_relaxed);
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
  if ((s2 ? s2->material.refractive_index : 1.0) != comps.n2) throw std::runtime_error("environment checker: the containers walk disagrees with n2");
  if (s2) {
    kid_medium = media::materialOf(T, s2);
    kid_nested = s2->id != xs[h].object->id;
  }
  const orc::Color c = shadeHit(S, M, K, T, Q, U, G, O, F, A, E, X, XO, H, comps, ng, code, remaining, J, medium, kid_medium, kid_nested, level);
  if (!A.any()) return c;
  orc::Color out{c.r * st.t[0], c.g * st.t[1], c.b * st.t[2]};
  if (st.fog) out = {st.in[0] + out.r, st.in[1] + out.g, st.in[2] + out.b};
  return out;
}

// media::render's pixel loop with env::colorAt; counters_out: media::render's 22, then [misses of camera rays, of reflected
// children, of refracted children, of children of a rough material, misses with a zero transmittance, sun rays clear,
// blocked, partly filtered, suns behind the surface, hits that only a sun lights]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
           const media::Table& A, const Table& E, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out,
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
    media::g_seg_atmosphere = 0;
    media::g_seg_medium = 0;
    media::g_seg_tinted = 0;
    media::g_miss_in_medium = 0;
    media::g_reflect_in_medium = 0;
    media::g_nested = 0;
    media::g_exit = 0;
    media::g_deep = 0;
    g_miss_camera = 0;
    g_miss_reflected = 0;
    g_miss_refracted = 0;
    g_miss_rough = 0;
    g_miss_dark = 0;
    g_sun_clear = 0;
    g_sun_blocked = 0;
    g_sun_partial = 0;
    g_sun_behind = 0;
    g_sun_only = 0;
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
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, O, F, A, E, X, XO, motion::passRay(camera, smp, x, y, k, g), 1, max_depth,
                                           J, media::kNoMedium, 0u, kCamera, false));
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
      counters_out[22] = g_miss_camera.load();
      counters_out[23] = g_miss_reflected.load();
      counters_out[24] = g_miss_refracted.load();
      counters_out[25] = g_miss_rough.load();
      counters_out[26] = g_miss_dark.load();
      counters_out[27] = g_sun_clear.load();
      counters_out[28] = g_sun_blocked.load();
      counters_out[29] = g_sun_partial.load();
      counters_out[30] = g_sun_behind.load();
      counters_out[31] = g_sun_only.load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace env

extern "C" {

// The environment (e NULL: no table at all).  Refuses what rtc_scene_set_environment refuses of the table's own values; the
// pattern index is held to the scene's rows when the sky is evaluated.  The suns are normalised as the product's host does.
int env_table_create(const rtc_environment* e, void** out) {
  try {
    auto t = std::make_unique<env::Table>();
    if (e) {
      t->present = true;
      for (int c = 0; c < 3; ++c) {
        t->rgb[c] = e->rgb[c];
        if (!std::isfinite(e->rgb[c]) || e->rgb[c] < 0.0) throw std::runtime_error("InvalidArgument: a colour that is not finite or is negative");
      }
      t->pattern = e->pattern;
      t->projection = e->projection;
      if (e->projection != RTC_ENV_SPHERE && e->projection != RTC_ENV_CUBE) throw std::runtime_error("InvalidArgument: a projection");
      if (e->n_suns > RTC_ENV_MAX_SUNS) throw std::runtime_error("InvalidArgument: too many suns");
      if (e->n_suns != 0 && (!e->sun_direction || !e->sun_rgb)) throw std::runtime_error("InvalidArgument: suns without a table");
      for (uint32_t i = 0; i < e->n_suns; ++i) {
        const double* d = e->sun_direction + 3 * static_cast<size_t>(i);
        const double* c = e->sun_rgb + 3 * static_cast<size_t>(i);
        for (int k = 0; k < 3; ++k)
          if (!std::isfinite(d[k]) || !std::isfinite(c[k]) || c[k] < 0.0) throw std::runtime_error("InvalidArgument: a sun that is not finite or is negative");
        const double len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (!(std::isfinite(len) && len > 0.0)) throw std::runtime_error("InvalidArgument: a sun's direction of zero or non-finite magnitude");
        const double a[3] = {d[0] / len, d[1] / len, d[2] / len};
        t->suns.push_back({orc::vec3(-a[0], -a[1], -a[2]), {c[0], c[1], c[2]}});
      }
    }
    *out = t.release();
    return 0;
  } catch (const std::exception& ex) {
    g_error = ex.what();
    return 1;
  }
}
void env_table_destroy(void* t) { delete static_cast<env::Table*>(t); }

// The scene and the bump, torus, texture, gloss, occlusion, filter and media tables: as media_render's; and the environment
// table.  counters_out: 32 entries.
int env_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, void* sf, void* me, void* ev, const rtc_camera* cam,
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
  return env::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                     *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                     *static_cast<occl::Table*>(oc), *static_cast<sfilt::Table*>(sf), *static_cast<media::Table*>(me),
                     *static_cast<env::Table*>(ev), x0, y0, w, h, n_threads, rgb_out, counters_out);
}

}  // extern "C"
