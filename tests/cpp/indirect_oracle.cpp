// indirect_oracle.cpp — CPU checker of indirect light (libindirect_oracle.so).  TEST INFRASTRUCTURE.
//
// Diffuse bounce rays and emissive materials (include/rtc.h rtc_scene_set_indirect) on top of the
// sky-light checker: skylight_oracle.cpp is included, read-only, and with it every checker below it and the oracle's sources.
// What is restated here is what names the recursion, as plain recursion:
//   - shadeHit, as skylight_oracle.cpp has it, with the material's emission row added after the sky-light step, and the third
//     child: where gain > 0, diffuse != 0, remaining > 0 and d < bounces, a ray from over_point along occl::direction about
//     ng, drawn from this table's key at word (d << 17) | code, with the reflected child's code, its parent's medium and
//     d + 1; what it returns, times (colour * diffuse) * gain per channel, is added to the hit's colour;
//   - colorAt, with the miss rule - the ray formed as a diffuse child adds no sky where the sky-light step runs - and the
//     keys of a ray with d > 0: key ^ (d * RTC_INDIRECT_DECORR) for the gloss, occlusion, sky-light and indirect draws;
//   - the pass loop, which names them.
// With no table, or one that forms no child and emits nothing, the render is skyl::render's bit for bit.  Seven counters
// beside the sky-light checker's: hits that formed a diffuse child; children withheld by `remaining`; by `bounces`; misses of
// diffuse children that were suppressed; that added the sky; the largest number of children pending at once in any pixel -
// what a depth-first walk that continues with the reflected child, then the refracted, then the diffuse one holds on its
// stack -; hits that added a non-zero emission.  Nothing of the product is included or linked.
#include "skylight_oracle.cpp"

namespace indir {

constexpr uint64_t kSalt = 0x452821E638D01377ull;
constexpr uint64_t kDecorr = RTC_INDIRECT_DECORR;
constexpr uint32_t kDiffuse = 3u;  // a ray's kind beside env::kCamera, kReflected, kRefracted
static_assert(kDiffuse != env::kCamera && kDiffuse != env::kReflected && kDiffuse != env::kRefracted, "a kind of its own");

struct Table {
  double gain = 0.0;
  uint32_t bounces = 0;
  uint64_t seed = 0;
  std::vector<double> emission;  // [materials][3]; empty: none
};

std::atomic<uint64_t> g_formed{0}, g_no_remaining{0}, g_no_bounces{0}, g_suppressed{0}, g_miss_diffuse{0}, g_max_pending{0}, g_emitted{0};

uint64_t keyOf(uint64_t seed) { return gloss::mix64(seed ^ kSalt); }

// The per-handle keys and the camera sample they are hashed with: a ray with d diffuse bounces draws from key ^ (d * C).
struct Keys {
  uint64_t gloss = 0, occl = 0, skyl = 0, indir = 0, p = 0, g = 0;
  gloss::Ctx of(uint64_t key, uint32_t d) const {
    gloss::Ctx c;
    c.h = gloss::sampleKey(key ^ (static_cast<uint64_t>(d) * kDecorr), p, g);
    return c;
  }
};

void notePending(uint64_t n) {
  uint64_t seen = g_max_pending.load(std::memory_order_relaxed);
  while (n > seen && !g_max_pending.compare_exchange_weak(seen, n, std::memory_order_relaxed)) {
  }
}

struct Walk {  // what a ray carries beside skyl::colorAt's arguments
  uint32_t d = 0;           // diffuse bounces on its lineage
  bool diffuse_child = false;
  uint64_t pending = 0;     // rays waiting on the depth-first walk's stack while this one is traced
};

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const env::Table& E, const skyl::Table& Y, const Table& I, const Keys& X, const orc::Ray& ray,
                   uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t level, uint32_t kind, bool rough_parent,
                   const Walk& W);

// skyl::shadeHit with the emission row after the sky-light step, the third child, the keys of d, and indir::colorAt
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                    const media::Table& A, const env::Table& E, const skyl::Table& Y, const Table& I, const Keys& X, const meshuv::Hit& H,
                    const orc::PreComputations& comps, orc::Tuple ng, uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium,
                    uint32_t kid_medium, bool kid_nested, uint32_t level, const Walk& W) {
  const gloss::Ctx XG = X.of(X.gloss, W.d), XO = X.of(X.occl, W.d), XY = X.of(X.skyl, W.d), XI = X.of(X.indir, W.d);
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
  // ---- the sky light (rtc.h): once per hit, after the last sun's term
  if (Y.gain > 0.0 && skyl::hasSky(E)) {
    if (m.diffuse == 0.0) {
      skyl::g_skipped.fetch_add(1, std::memory_order_relaxed);
    } else {
      if (code > 1) skyl::g_deep.fetch_add(1, std::memory_order_relaxed);
      const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
      double L[3] = {0.0, 0.0, 0.0};
      for (uint32_t k = 0; k < Y.samples; ++k) {
        const uint64_t word = (static_cast<uint64_t>(k) << occl::kSampleShift) | code;
        const orc::Tuple d = occl::direction([&](uint32_t axis) { return gloss::jitter(XY.h, word, axis); }, ng);
        const sfilt::Trans t = env::sunTransmittance(S, M, T, Q, F, comps.over_point, d, false);
        if (t.blocked()) {
          skyl::g_blocked.fetch_add(1, std::memory_order_relaxed);
          continue;
        }
        (t.r == 1.0 && t.g == 1.0 && t.b == 1.0 ? skyl::g_clear : skyl::g_partial).fetch_add(1, std::memory_order_relaxed);
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
  // ---- emission (rtc.h): after the last light's, sun's and sky-light term
  if (!I.emission.empty()) {
    const double* e = I.emission.data() + 3ull * media::materialOf(T, obj);
    if (e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0) g_emitted.fetch_add(1, std::memory_order_relaxed);
    surface = orc::cadd(surface, orc::Color{e[0], e[1], e[2]});
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
  // ---- the diffuse child's conditions (rtc.h)
  bool do_diffuse = false;
  if (I.gain > 0.0 && m.diffuse != 0.0) {
    if (remaining == 0) {
      g_no_remaining.fetch_add(1, std::memory_order_relaxed);
    } else if (!(W.d < I.bounces)) {
      g_no_bounces.fetch_add(1, std::memory_order_relaxed);
    } else {
      do_diffuse = true;
      g_formed.fetch_add(1, std::memory_order_relaxed);
    }
  }
  // (the depth-first walk: the reflected child continues, the refracted waits above the diffuse one; each is traced with
  // the siblings that still wait beneath it)
  const uint64_t kids = (do_reflect ? 1u : 0u) + (do_refract ? 1u : 0u) + (do_diffuse ? 1u : 0u);
  if (kids != 0) notePending(W.pending + kids - 1);
  uint64_t waiting = kids;
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0}, indirect{0.0, 0.0, 0.0};
  if (do_reflect) {  // world.zig:157-167: in its parent's medium
    orc::counters().secondary++;
    if (A.any() && medium != media::kNoMedium) media::g_reflect_in_medium.fetch_add(1, std::memory_order_relaxed);
    orc::Tuple d = comps.reflectv;
    if (rough_r > 0.0) d = gloss::scatter(XG, 2 * code, rough_r, d, ng, false);
    const Walk w{W.d, false, W.pending + --waiting};
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, I, X, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                  level + (do_refract ? 1u : 0u), env::kReflected, rough_r > 0.0, w),
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
    if (rough_t > 0.0) direction = gloss::scatter(XG, 2 * code + 1, rough_t, direction, ng, true);
    const Walk w{W.d, false, W.pending + --waiting};
    refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, I, X, orc::Ray{comps.under_point, direction}, 2 * code + 1,
                                  remaining - 1, J, kid_medium, level, env::kRefracted, rough_t > 0.0, w),
                          m.transparency);
  }
  if (do_diffuse) {  // (rtc.h) in its parent's medium, with the reflected child's code
    orc::counters().secondary++;
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    const uint64_t word = (static_cast<uint64_t>(W.d) << occl::kSampleShift) | code;
    const orc::Tuple d = occl::direction([&](uint32_t axis) { return gloss::jitter(XI.h, word, axis); }, ng);
    const Walk w{W.d + 1, true, W.pending + --waiting};
    const orc::Color c = colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, I, X, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                 level, kDiffuse, false, w);
    indirect = {c.r * ((color.r * m.diffuse) * I.gain), c.g * ((color.g * m.diffuse) * I.gain), c.b * ((color.b * m.diffuse) * I.gain)};
  }
  orc::Color out;
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    out = orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  } else {
    out = orc::cadd(orc::cadd(surface, reflected), refracted);
  }
  return do_diffuse ? orc::cadd(out, indirect) : out;
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const env::Table& E, const skyl::Table& Y, const Table& I, const Keys& X, const orc::Ray& ray,
                   uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t level, uint32_t kind, bool rough_parent,
                   const Walk& W) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  // ---- the media step (rtc.h): after the closest-hit search, whatever `remaining`; without a table it is not there at all
  media::Step st;
  if (A.any()) st = media::segment(A, medium, ray, h >= 0, h >= 0 ? xs[h].t : 0.0);
  if (h < 0) {
    const orc::Color in = st.fog ? orc::Color{st.in[0], st.in[1], st.in[2]} : orc::Color{0.0, 0.0, 0.0};
    if (!skyl::hasSky(E)) return in;
    // ---- no sky counted twice (rtc.h): the sky-light step at the parent's hit gathered it
    if (W.diffuse_child && Y.gain > 0.0) {
      g_suppressed.fetch_add(1, std::memory_order_relaxed);
      return in;
    }
    // ---- the miss step (rtc.h): after the media step, the sky's colour times the miss transmittance
    orc::Color e = env::sky(S, U, E, ray);
    if (A.any()) e = {e.r * st.t[0], e.g * st.t[1], e.b * st.t[2]};
    if (st.t[0] == 0.0 && st.t[1] == 0.0 && st.t[2] == 0.0) {
      env::g_miss_dark.fetch_add(1, std::memory_order_relaxed);
    } else {
      (kind == env::kCamera ? env::g_miss_camera
                            : (kind == env::kReflected ? env::g_miss_reflected : (kind == env::kRefracted ? env::g_miss_refracted : g_miss_diffuse)))
          .fetch_add(1, std::memory_order_relaxed);
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
  if ((s2 ? s2->material.refractive_index : 1.0) != comps.n2) throw std::runtime_error("indirect checker: the containers walk disagrees with n2");
  if (s2) {
    kid_medium = media::materialOf(T, s2);
    kid_nested = s2->id != xs[h].object->id;
  }
  const orc::Color c = shadeHit(S, M, K, T, Q, U, G, O, F, A, E, Y, I, X, H, comps, ng, code, remaining, J, medium, kid_medium, kid_nested, level, W);
  if (!A.any()) return c;
  orc::Color out{c.r * st.t[0], c.g * st.t[1], c.b * st.t[2]};
  if (st.fog) out = {st.in[0] + out.r, st.in[1] + out.g, st.in[2] + out.b};
  return out;
}

constexpr uint32_t kSkylCounters = 37;
constexpr uint32_t kCounters = kSkylCounters + 7;

// skyl::render's pixel loop with indir::colorAt; counters_out: skyl::render's 37, then [hits that formed a diffuse child,
// children withheld by remaining, by bounces, diffuse-child misses suppressed, diffuse-child misses that added the sky, the
// largest number of children pending at once in any pixel, hits that added a non-zero emission]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
           const media::Table& A, const env::Table& E, const skyl::Table& Y, const Table& I, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
           uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const motion::Motion base = motion::make(S, disp, n_roots);
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if ((static_cast<uint64_t>(pass) + 1) * n_samples > (1ull << 24)) throw std::runtime_error("InvalidArgument: pass");
    const uint64_t n_pixels = static_cast<uint64_t>(cam->hsize) * cam->vsize;
    Keys keys;
    keys.gloss = gloss::keyOf(G.seed);
    keys.occl = occl::keyOf(O.seed);
    keys.skyl = skyl::keyOf(Y.seed);
    keys.indir = keyOf(I.seed);
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    std::atomic<uint64_t>* const zeroed[] = {
        &gloss::g_used, &gloss::g_fell, &occl::g_occluded, &occl::g_clear, &occl::g_skipped, &occl::g_deep, &sfilt::g_clear, &sfilt::g_partial,
        &sfilt::g_blocked, &sfilt::g_three, &sfilt::g_three_partial, &sfilt::g_factors, &sfilt::g_at_light, &media::g_seg_atmosphere,
        &media::g_seg_medium, &media::g_seg_tinted, &media::g_miss_in_medium, &media::g_reflect_in_medium, &media::g_nested, &media::g_exit,
        &media::g_deep, &env::g_miss_camera, &env::g_miss_reflected, &env::g_miss_refracted, &env::g_miss_rough, &env::g_miss_dark,
        &env::g_sun_clear, &env::g_sun_blocked, &env::g_sun_partial, &env::g_sun_behind, &env::g_sun_only, &skyl::g_clear, &skyl::g_partial,
        &skyl::g_blocked, &skyl::g_skipped, &skyl::g_deep, &g_formed, &g_no_remaining, &g_no_bounces, &g_suppressed, &g_miss_diffuse,
        &g_max_pending, &g_emitted};
    for (std::atomic<uint64_t>* c : zeroed) *c = 0;
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
              Keys X = keys;
              X.p = p;
              X.g = g;
              // (a camera ray is in the atmosphere: the camera stands outside every solid)
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, O, F, A, E, Y, I, X, motion::passRay(camera, smp, x, y, k, g), 1, max_depth, J,
                                           media::kNoMedium, 0u, env::kCamera, false, Walk{}));
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
      const std::atomic<uint64_t>* const reported[] = {
          &occl::g_occluded, &occl::g_clear, &occl::g_skipped, &occl::g_deep, &sfilt::g_clear, &sfilt::g_partial, &sfilt::g_blocked, &sfilt::g_three,
          &sfilt::g_three_partial, &sfilt::g_factors, &sfilt::g_at_light, &media::g_seg_atmosphere, &media::g_seg_medium, &media::g_seg_tinted,
          &media::g_miss_in_medium, &media::g_reflect_in_medium, &media::g_nested, &media::g_exit, &media::g_deep, &env::g_miss_camera,
          &env::g_miss_reflected, &env::g_miss_refracted, &env::g_miss_rough, &env::g_miss_dark, &env::g_sun_clear, &env::g_sun_blocked,
          &env::g_sun_partial, &env::g_sun_behind, &env::g_sun_only, &skyl::g_clear, &skyl::g_partial, &skyl::g_blocked, &skyl::g_skipped,
          &skyl::g_deep, &g_formed, &g_no_remaining, &g_no_bounces, &g_suppressed, &g_miss_diffuse, &g_max_pending, &g_emitted};
      static_assert(3 + sizeof(reported) / sizeof(reported[0]) == kCounters, "skyl::render's 37 counters, then this checker's seven");
      uint32_t at = 3;
      for (const std::atomic<uint64_t>* c : reported) counters_out[at++] = c->load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace indir

extern "C" {

// The indirect table (d NULL: no table).  Refuses what rtc_scene_set_indirect refuses but the material count, which the
// checker's scene does not flatten: the rows are taken as given.
int indir_table_create(const rtc_indirect* d, void** out) {
  try {
    auto t = std::make_unique<indir::Table>();
    if (d) {
      if (!std::isfinite(d->gain) || d->gain < 0.0) throw std::runtime_error("InvalidArgument: a gain that is not finite or is negative");
      if (d->bounces > 16u) throw std::runtime_error("InvalidArgument: bounces");
      if (d->emission) {
        for (size_t i = 0; i < 3ull * d->n_materials; ++i)
          if (!std::isfinite(d->emission[i]) || d->emission[i] < 0.0) throw std::runtime_error("InvalidArgument: an emission that is not finite or is negative");
        t->emission.assign(d->emission, d->emission + 3ull * d->n_materials);
      }
      t->gain = d->gain;
      t->bounces = d->bounces;
      t->seed = d->seed;
    }
    *out = t.release();
    return 0;
  } catch (const std::exception& ex) {
    g_error = ex.what();
    return 1;
  }
}
void indir_table_destroy(void* t) { delete static_cast<indir::Table*>(t); }
uint32_t indir_counters(void) { return indir::kCounters; }

// The scene and the tables: as skyl_render's; and the indirect table.  counters_out: indir_counters() entries.
int indir_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, void* sf, void* me, void* ev, void* sl, void* in,
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
  return indir::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                       *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                       *static_cast<occl::Table*>(oc), *static_cast<sfilt::Table*>(sf), *static_cast<media::Table*>(me),
                       *static_cast<env::Table*>(ev), *static_cast<skyl::Table*>(sl), *static_cast<indir::Table*>(in), x0, y0, w, h, n_threads,
                       rgb_out, counters_out);
}

}  // extern "C"
