// sfilter_oracle.cpp — CPU checker of shadow filters (libsfilter_oracle.so).  TEST INFRASTRUCTURE.
//
// Light that comes through a filtering material dimmed and tinted (include/rtc.h rtc_scene_set_shadow_filters, DESIGN.md
// section 22) on top of the occlusion checker: occlusion_oracle.cpp is included, read-only, and with it the gloss,
// mesh-texture, torus, bump, spot, motion, camera-sampling and area-light checkers and the oracle's sources.  What is
// restated here is what the feature changes:
//   - isShadowed of a LIGHT as a transmittance: the product of the filter rows of every entry with 0 <= t < distance on a
//     casts_shadow leaf, in the sorted list's order (the occlusion rays keep occl::occluded, a bool);
//   - Material.lighting of a point or spot light with the diffuse and specular terms times the transmittance, and of an
//     area light with the per-channel mean of its samples' transmittances in intensity_at's place;
//   - shadeHit, colorAt and the pass loop, as occlusion_oracle.cpp has them, because they name the lighting.
// Seven counters beside the ray counts, over the light shadow rays the product traces (a point or spot light's only where the
// material has a diffuse or specular term and the light is not behind the surface; an area light's when its sum is not
// zero): rays that end with T all one, with a partial T, blocked; rays that saw three or more counting entries; rays that
// saw three or more PARTIAL factors (neither 0 nor 1 in some channel); the factors multiplied; and the entries of
// casts_shadow leaves that fell at t == distance to the bit, which do not count.
// Nothing of the product is included or linked.
#include "occlusion_oracle.cpp"

namespace sfilt {

struct Table {
  std::vector<double> rgb;  // three per material row (mat_* order); empty: no table, every material blocks
};

std::atomic<uint64_t> g_clear{0}, g_partial{0}, g_blocked{0}, g_three{0}, g_three_partial{0}, g_factors{0}, g_at_light{0};

struct Trans {
  double r = 1.0, g = 1.0, b = 1.0;
  bool blocked() const { return r == 0.0 && g == 0.0 && b == 0.0; }
};

// torus::isShadowed as a transmittance (rtc.h); `traced`: the product traces this ray - it is counted by result
Trans transmittance(const area::Scene& S, const motion::Motion& M, const bump::Table& T, const torus::Table& Q, const Table& F,
                    orc::Tuple pt, orc::Tuple light_pos, bool traced) {
  orc::counters().shadow++;
  const orc::Tuple direction = orc::sub(light_pos, pt);
  const double distance = orc::magnitude(direction);
  const orc::Ray shadow_ray{pt, orc::normalized(direction)};
  const orc::Intersections xs = torus::intersect(S, M, Q, shadow_ray);
  Trans t;
  uint32_t entries = 0, partial = 0;
  long i = orc::hit(xs);
  while (i >= 0) {
    if (xs[i].t < distance && xs[i].object->casts_shadow) {
      double f[3] = {0.0, 0.0, 0.0};
      if (!F.rgb.empty()) {
        const auto it = T.mat_of.find(xs[i].object->id);
        if (it == T.mat_of.end()) throw std::runtime_error("shadow-filter checker: an entry of a shape that is no leaf of the description");
        for (int c = 0; c < 3; ++c) f[c] = F.rgb[3 * static_cast<size_t>(it->second) + c];
      }
      t.r = t.r * f[0];
      t.g = t.g * f[1];
      t.b = t.b * f[2];
      ++entries;
      bool part = false;
      for (int c = 0; c < 3; ++c) part = part || (f[c] != 0.0 && f[c] != 1.0);
      if (part) ++partial;
    } else if (traced && xs[i].t == distance && xs[i].object->casts_shadow) {
      g_at_light.fetch_add(1, std::memory_order_relaxed);
    }
    i = orc::hit(xs, static_cast<size_t>(i) + 1);
  }
  if (traced) {
    if (t.blocked()) g_blocked.fetch_add(1, std::memory_order_relaxed);
    else if (t.r == 1.0 && t.g == 1.0 && t.b == 1.0) g_clear.fetch_add(1, std::memory_order_relaxed);
    else g_partial.fetch_add(1, std::memory_order_relaxed);
    if (entries >= 3) g_three.fetch_add(1, std::memory_order_relaxed);
    if (partial >= 3) g_three_partial.fetch_add(1, std::memory_order_relaxed);
    g_factors.fetch_add(entries, std::memory_order_relaxed);
  }
  return t;
}

// spot::spotLighting with the transmittance: blocked - the shadowed branch; else both terms times T, after the cone's factor
orc::Color pointLighting(const orc::Material& m, orc::Color color, const area::Light& L, orc::Tuple point_to_light, orc::Tuple eyev,
                         orc::Tuple normal, const Trans& t, double f) {
  const orc::Color effective_color = orc::cemul(color, L.intensity);
  const orc::Color ambient_ = orc::cmul(effective_color, m.ambient);
  if (t.blocked()) return ambient_;
  orc::Color diffuse_{0.0, 0.0, 0.0}, specular_{0.0, 0.0, 0.0};
  const double light_dot_normal = orc::dot(point_to_light, normal);
  if (light_dot_normal >= 0.0) {
    diffuse_ = orc::cmul(orc::cmul(effective_color, m.diffuse * light_dot_normal), f);
    const double reflect_dot_eye = orc::dot(orc::negate(orc::reflect(point_to_light, normal)), eyev);
    if (reflect_dot_eye > 0.0) specular_ = orc::cmul(orc::cmul(L.intensity, m.specular * orc::zig_pow(reflect_dot_eye, m.shininess)), f);
  }
  diffuse_ = {diffuse_.r * t.r, diffuse_.g * t.g, diffuse_.b * t.b};
  specular_ = {specular_.r * t.r, specular_.g * t.g, specular_.b * t.b};
  return orc::cadd(orc::cadd(ambient_, diffuse_), specular_);
}

// torus::areaLighting with intensity_at per channel: the samples' transmittances summed from 0.0, v outer, u inner
orc::Color areaLighting(const area::Scene& S, const motion::Motion& M, const bump::Table& T, const torus::Table& Q, const Table& F,
                        const orc::Material& m, orc::Color color, const area::Light& L, uint32_t l, orc::Tuple pt, orc::Tuple eyev,
                        orc::Tuple normal, const area::Jitter& J) {
  const orc::Color effective = orc::cemul(color, L.intensity);
  const orc::Color ambient = orc::cmul(effective, m.ambient);
  const orc::Color sum = area::areaSum(m, effective, L, l, pt, eyev, normal, J);
  if (sum.r == 0.0 && sum.g == 0.0 && sum.b == 0.0) {
    orc::counters().shadow += L.samples();
    return ambient;
  }
  const double n = static_cast<double>(L.samples());
  double lit_r = 0.0, lit_g = 0.0, lit_b = 0.0;
  for (uint32_t v = 0; v < L.vsteps; ++v)
    for (uint32_t u = 0; u < L.usteps; ++u) {
      const uint32_t k = v * L.usteps + u;
      const double ju = J.at(L, l, k, 0), jv = J.at(L, l, k, 1);
      const Trans t = transmittance(S, M, T, Q, F, pt, area::pointOnLight(L, u, v, ju, jv), true);
      lit_r = lit_r + t.r;
      lit_g = lit_g + t.g;
      lit_b = lit_b + t.b;
    }
  return {ambient.r + (sum.r / n) * (lit_r / n), ambient.g + (sum.g / n) * (lit_g / n), ambient.b + (sum.b / n) * (lit_b / n)};
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const Table& F,
                   const gloss::Ctx& X, const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J);

// occl::shadeHit with the lights' transmittances
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const Table& F,
                    const gloss::Ctx& X, const gloss::Ctx& XO, const meshuv::Hit& H, const orc::PreComputations& comps, orc::Tuple ng,
                    uint64_t code, size_t remaining, const area::Jitter& J) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  // ---- the occlusion step (rtc.h): once per hit, before the lights; its rays stay binary
  double ka = m.ambient;
  if (!O.radius.empty()) {
    const auto it = T.mat_of.find(obj->id);
    if (it == T.mat_of.end()) throw std::runtime_error("shadow-filter checker: a hit on a shape that is no leaf of the description");
    const double radius = O.radius[it->second];
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
      const bool traced = !(m.diffuse == 0.0 && m.specular == 0.0) && orc::dot(point_to_light, comps.normal) >= 0.0;
      const Trans t = transmittance(S, M, T, Q, F, comps.over_point, L.corner, traced);
      surface = orc::cadd(surface, pointLighting(*ml, color, L, point_to_light, comps.eyev, comps.normal, t, f));
    } else {
      surface = orc::cadd(surface, areaLighting(S, M, T, Q, F, *ml, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  double rough_r = 0.0, rough_t = 0.0;
  if (!G.reflection.empty()) {
    const auto it = T.mat_of.find(obj->id);
    if (it == T.mat_of.end()) throw std::runtime_error("shadow-filter checker: a hit on a shape that is no leaf of the description");
    rough_r = G.reflection[it->second];
    rough_t = G.transmission[it->second];
  }
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    orc::Tuple d = comps.reflectv;
    if (rough_r > 0.0) d = gloss::scatter(X, 2 * code, rough_r, d, ng, false);
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, X, XO, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J), m.reflective);
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
      refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, X, XO, orc::Ray{comps.under_point, direction}, 2 * code + 1, remaining - 1, J),
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
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const Table& F,
                   const gloss::Ctx& X, const gloss::Ctx& XO, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  if (h < 0) return {0.0, 0.0, 0.0};
  const meshuv::Hit H = meshuv::hitOf(M, U, xs[h], ray);
  const orc::PreComputations comps = torus::precompute(M, T, Q, xs[h], ray, xs);
  orc::Tuple ng = torus::normalAt(Q, xs[h].object, motion::shift(comps.point, M.t, motion::dispOf(M, xs[h].object)), xs[h]);
  if (comps.inside) ng = orc::negate(ng);
  return shadeHit(S, M, K, T, Q, U, G, O, F, X, XO, H, comps, ng, code, remaining, J);
}

// occl::render's pixel loop with sfilt::colorAt; counters_out [primary, secondary, shadow calls, occluded, unoccluded,
// skipped for ambient == 0, occlusion hits at a code above 1, T all one, partial, blocked, three or more entries, three or
// more partial factors, factors, entries at t == distance]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const Table& F, uint32_t x0,
           uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
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
    g_clear = 0;
    g_partial = 0;
    g_blocked = 0;
    g_three = 0;
    g_three_partial = 0;
    g_factors = 0;
    g_at_light = 0;
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
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, O, F, X, XO, motion::passRay(camera, smp, x, y, k, g), 1, max_depth, J));
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
      counters_out[7] = g_clear.load();
      counters_out[8] = g_partial.load();
      counters_out[9] = g_blocked.load();
      counters_out[10] = g_three.load();
      counters_out[11] = g_three_partial.load();
      counters_out[12] = g_factors.load();
      counters_out[13] = g_at_light.load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace sfilt

extern "C" {

// The filter rows (NULL: all zeros; n_materials 0: no table at all).  Refuses what rtc_scene_set_shadow_filters refuses of
// the table's own values.
int sfilt_table_create(uint32_t n_materials, const double* rgb, void** out) {
  try {
    auto t = std::make_unique<sfilt::Table>();
    t->rgb.assign(3 * static_cast<size_t>(n_materials), 0.0);
    for (size_t i = 0; i < t->rgb.size(); ++i) {
      if (rgb) t->rgb[i] = rgb[i];
      if (!std::isfinite(t->rgb[i]) || t->rgb[i] < 0.0 || t->rgb[i] > 1.0)
        throw std::runtime_error("InvalidArgument: a filter value that is not finite or outside [0, 1]");
    }
    *out = t.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void sfilt_table_destroy(void* t) { delete static_cast<sfilt::Table*>(t); }

// The scene and the bump, torus, texture, gloss and occlusion tables: as occl_render's; and the filter table.
// counters_out: 14 entries.
int sfilt_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, void* sf, const rtc_camera* cam, uint32_t max_depth,
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
  return sfilt::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                       *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                       *static_cast<occl::Table*>(oc), *static_cast<sfilt::Table*>(sf), x0, y0, w, h, n_threads, rgb_out, counters_out);
}

}  // extern "C"
