// emitters_oracle.cpp — CPU checker of emitter sampling (libemitters_oracle.so).  TEST INFRASTRUCTURE.
//
// Emissive surfaces sampled directly at diffuse hits (include/rtc.h rtc_scene_set_emitters) on top of the
// indirect-light checker: indirect_oracle.cpp is included, read-only, and with it every checker below it and the oracle's
// sources.  What is restated here, as plain recursion:
//   - the emitter list, from the oracle's own scene build - the shapes' inverse matrices, triangles and materials as
//     oracle_capi.cpp made them, walked depth first -, not from any table of the product;
//   - shadeHit, as indirect_oracle.cpp has it, with the sample step after the sky-light step and the suppressed emission of a
//     ray formed as a diffuse child at a listed leaf;
//   - colorAt and the pass loop, which name them.
// With no table or an empty list the render is indir::render's bit for bit.  Seven counters beside the indirect checker's:
// samples drawn; skipped by cos_x; by cos_e; by r; walks made; walks blocked; emissions suppressed.  Three variants of the
// sample step (kNoPi, kNoCosE, kHalfArea) and one of the suppression rule (kNoSuppress) exist for the tests that show each of
// those mistakes missing its bound; a table made without flags has none.  Nothing of the product is included or linked.
#include "indirect_oracle.cpp"

#include <unordered_set>

namespace emit {

constexpr uint64_t kSalt = 0xC0AC29B7C97C50DDull;
constexpr uint32_t kRow = 18;
constexpr uint32_t kMaxEntries = RTC_MAX_EMITTERS;
constexpr uint32_t kNoPi = 1u, kNoCosE = 2u, kHalfArea = 4u, kNoSuppress = 8u;  // the variants (tests only)

struct Table {
  bool on = false;
  uint32_t samples = 1;
  uint64_t seed = 0;
  uint32_t flags = 0;
};

struct List {
  std::vector<double> row, cdf;  // rtc_diag_emitters' layout
  std::unordered_set<size_t> ids;  // Shape.id of every listed leaf
  double total = 0.0;
  size_t size() const { return cdf.size(); }
};

std::atomic<uint64_t> g_drawn{0}, g_skip_cos_x{0}, g_skip_cos_e{0}, g_skip_r{0}, g_walks{0}, g_blocked{0}, g_suppressed{0};

uint64_t keyOf(uint64_t seed) { return gloss::mix64(seed ^ kSalt); }

// rtc.h's list: depth first over World.objects; a csg's leaves are counted, not listed
void listShape(const orc::Shape& s, const bump::Table& T, const sfilt::Table& F, const indir::Table& I, uint32_t flags, bool under_csg,
               uint32_t& next_leaf, List& out) {
  if (s.kind == orc::GROUP || s.kind == orc::CSG) {
    for (const orc::Shape& c : s.children) listShape(c, T, F, I, flags, under_csg || s.kind == orc::CSG, next_leaf, out);
    return;
  }
  const uint32_t leaf = next_leaf++;
  if (s.kind != orc::CUBE && s.kind != orc::TRIANGLE && s.kind != orc::SMOOTH_TRIANGLE) return;
  if (!s.casts_shadow || under_csg || I.emission.empty()) return;
  const uint32_t mi = media::materialOf(T, &s);
  const double* E = I.emission.data() + 3ull * mi;
  if (E[0] == 0.0 && E[1] == 0.0 && E[2] == 0.0) return;
  if (!F.rgb.empty()) {
    const double* f = F.rgb.data() + 3ull * mi;
    if (f[0] != 0.0 || f[1] != 0.0 || f[2] != 0.0) return;
  }
  const auto& a = s.inverse.d;
  const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  const double c10 = a[0][2] * a[2][1] - a[0][1] * a[2][2], c11 = a[0][0] * a[2][2] - a[0][2] * a[2][0], c12 = a[0][1] * a[2][0] - a[0][0] * a[2][1];
  const double c20 = a[0][1] * a[1][2] - a[0][2] * a[1][1], c21 = a[0][2] * a[1][0] - a[0][0] * a[1][2], c22 = a[0][0] * a[1][1] - a[0][1] * a[1][0];
  const double det = (a[0][0] * c00 + a[0][1] * c01) + a[0][2] * c02;
  const double L[3][3] = {{c00 / det, c10 / det, c20 / det}, {c01 / det, c11 / det, c21 / det}, {c02 / det, c12 / det, c22 / det}};
  double t[3];
  for (int i = 0; i < 3; ++i) t[i] = -((L[i][0] * a[0][3] + L[i][1] * a[1][3]) + L[i][2] * a[2][3]);
  const double sum_e = (E[0] + E[1]) + E[2];
  auto add = [&](const double* o, const double* eu, const double* ev, bool half) {
    double R[kRow] = {};
    for (int i = 0; i < 3; ++i) {
      R[0 + i] = ((L[i][0] * o[0] + L[i][1] * o[1]) + L[i][2] * o[2]) + t[i];
      R[3 + i] = (L[i][0] * eu[0] + L[i][1] * eu[1]) + L[i][2] * eu[2];
      R[6 + i] = (L[i][0] * ev[0] + L[i][1] * ev[1]) + L[i][2] * ev[2];
    }
    const double mx = R[4] * R[8] - R[5] * R[7], my = R[5] * R[6] - R[3] * R[8], mz = R[3] * R[7] - R[4] * R[6];
    const double len = std::sqrt((mx * mx + my * my) + mz * mz);
    R[9] = mx / len;
    R[10] = my / len;
    R[11] = mz / len;
    double area = half ? len / 2.0 : len;
    if (flags & kHalfArea) area = area / 2.0;  // (variant: every area halved once more)
    const double w = area * sum_e;
    if (!(std::isfinite(w) && w > 0.0)) return;
    R[12] = E[0];
    R[13] = E[1];
    R[14] = E[2];
    R[16] = half ? 1.0 : 0.0;
    R[17] = static_cast<double>(leaf);
    out.total = out.total + w;
    out.row.insert(out.row.end(), R, R + kRow);
    out.cdf.push_back(out.total);
    out.ids.insert(s.id);
  };
  if (s.kind == orc::CUBE) {
    for (int ax = 0; ax < 3; ++ax)
      for (int sgn = 0; sgn < 2; ++sgn) {
        const int b = (ax + 1) % 3, c = (ax + 2) % 3;
        double o[3] = {-1.0, -1.0, -1.0}, eu[3] = {0.0, 0.0, 0.0}, ev[3] = {0.0, 0.0, 0.0};
        o[ax] = sgn == 0 ? 1.0 : -1.0;
        eu[b] = 2.0;
        ev[c] = 2.0;
        add(o, eu, ev, false);
      }
  } else {
    const double o[3] = {s.p1.x, s.p1.y, s.p1.z}, eu[3] = {s.e1.x, s.e1.y, s.e1.z}, ev[3] = {s.e2.x, s.e2.y, s.e2.z};
    add(o, eu, ev, true);
  }
}

List makeList(const area::Scene& S, const bump::Table& T, const sfilt::Table& F, const indir::Table& I, uint32_t flags) {
  List out;
  uint32_t next_leaf = 0;
  for (const orc::Shape& s : S.os->world.objects) listShape(s, T, F, I, flags, false, next_leaf, out);
  if (out.size() > kMaxEntries) throw std::runtime_error("Unsupported: more than RTC_MAX_EMITTERS entries");
  for (size_t k = 0; k < out.size(); ++k) {
    double* R = out.row.data() + static_cast<size_t>(kRow) * k;
    R[15] = out.total / ((R[12] + R[13]) + R[14]);
  }
  return out;
}

// rtc.h's pick: the first entry with cdf[k] > u0 * W, the last entry where there is none
uint32_t pick(const double* cdf, uint32_t n, double total, double u0) {
  const double x = u0 * total;
  for (uint32_t k = 0; k < n; ++k)
    if (cdf[k] > x) return k;
  return n - 1;
}

struct Ctx {  // what the sample step needs beside indir's arguments
  const Table* table;
  const List* list;
  uint64_t key = 0;
};

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const Ctx& C,
                   const indir::Keys& X, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium,
                   uint32_t level, uint32_t kind, bool rough_parent, const indir::Walk& W);

// rtc.h's walk of one sample: the filter rows of every entry with 0 <= t < far on a casts_shadow leaf, from pt along w
sfilt::Trans sampleWalk(const area::Scene& S, const motion::Motion& M, const bump::Table& T, const torus::Table& Q, const sfilt::Table& F,
                        orc::Tuple pt, orc::Tuple w, double far) {
  orc::counters().shadow++;
  const orc::Intersections xs = torus::intersect(S, M, Q, orc::Ray{pt, w});
  sfilt::Trans t;
  long i = orc::hit(xs);
  while (i >= 0) {
    if (xs[i].t < far && xs[i].object->casts_shadow) {
      double f[3] = {0.0, 0.0, 0.0};
      if (!F.rgb.empty()) {
        const uint32_t mi = media::materialOf(T, xs[i].object);
        for (int c = 0; c < 3; ++c) f[c] = F.rgb[3 * static_cast<size_t>(mi) + c];
      }
      t.r = t.r * f[0];
      t.g = t.g * f[1];
      t.b = t.b * f[2];
    }
    i = orc::hit(xs, static_cast<size_t>(i) + 1);
  }
  return t;
}

// indir::shadeHit with the sample step after the sky-light step, the suppressed emission, and emit::colorAt
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                    const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const Ctx& C,
                    const indir::Keys& X, const meshuv::Hit& H, const orc::PreComputations& comps, orc::Tuple ng, uint64_t code,
                    size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t kid_medium, bool kid_nested, uint32_t level,
                    const indir::Walk& W) {
  const gloss::Ctx XG = X.of(X.gloss, W.d), XO = X.of(X.occl, W.d), XY = X.of(X.skyl, W.d), XI = X.of(X.indir, W.d);
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  // ---- the occlusion step (rtc.h)
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
  orc::Material mk;
  const orc::Material* ml = &m;
  if (ka != m.ambient) {
    mk = m;
    mk.ambient = ka;
    ml = &mk;
  }
  const bool shadow_matters = !(m.diffuse == 0.0 && m.specular == 0.0);
  bool lit_by_light = false;
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
      const bool traced = shadow_matters && orc::dot(point_to_light, comps.normal) >= 0.0;
      const sfilt::Trans t = sfilt::transmittance(S, M, T, Q, F, comps.over_point, L.corner, traced);
      lit_by_light = lit_by_light || (traced && !t.blocked());
      surface = orc::cadd(surface, sfilt::pointLighting(*ml, color, L, point_to_light, comps.eyev, comps.normal, t, f));
    } else {
      lit_by_light = true;
      surface = orc::cadd(surface, sfilt::areaLighting(S, M, T, Q, F, *ml, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  // ---- the suns (rtc.h)
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
  // ---- the sky light (rtc.h)
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
  // ---- the emitter samples (rtc.h's rtc_scene_set_emitters): where the diffuse child is formed, after the sky-light step
  const bool forms_child = I.gain > 0.0 && m.diffuse != 0.0 && remaining != 0 && W.d < I.bounces;
  if (forms_child && C.list->size() != 0) {
    const List& EL = *C.list;
    const uint32_t flags = C.table->flags;
    const gloss::Ctx XE = X.of(C.key, W.d);
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < C.table->samples; ++j) {
      const uint64_t word = (static_cast<uint64_t>(j) << occl::kSampleShift) | code;
      const double u0 = gloss::jitter(XE.h, word, 0);
      double u = gloss::jitter(XE.h, word, 1), v = gloss::jitter(XE.h, word, 2);
      g_drawn.fetch_add(1, std::memory_order_relaxed);
      const uint32_t k = pick(EL.cdf.data(), static_cast<uint32_t>(EL.size()), EL.total, u0);
      const double* R = EL.row.data() + static_cast<size_t>(kRow) * k;
      if (R[16] != 0.0 && u + v > 1.0) {
        u = 1.0 - u;
        v = 1.0 - v;
      }
      const double yx = (R[0] + u * R[3]) + v * R[6], yy = (R[1] + u * R[4]) + v * R[7], yz = (R[2] + u * R[5]) + v * R[8];
      const double vx = yx - comps.over_point.x, vy = yy - comps.over_point.y, vz = yz - comps.over_point.z;
      const double r2 = (vx * vx + vy * vy) + vz * vz;
      const double r = std::sqrt(r2);
      const orc::Tuple w = orc::vec3(vx / r, vy / r, vz / r);
      const double cos_x = (ng.x * w.x + ng.y * w.y) + ng.z * w.z;
      const double cos_e = (flags & kNoCosE) ? 1.0 : std::fabs((R[9] * w.x + R[10] * w.y) + R[11] * w.z);
      if (cos_x <= 0.0) {
        g_skip_cos_x.fetch_add(1, std::memory_order_relaxed);
        continue;
      }
      if (cos_e == 0.0) {
        g_skip_cos_e.fetch_add(1, std::memory_order_relaxed);
        continue;
      }
      if (r <= 2e-4) {
        g_skip_r.fetch_add(1, std::memory_order_relaxed);
        continue;
      }
      g_walks.fetch_add(1, std::memory_order_relaxed);
      const sfilt::Trans t = sampleWalk(S, M, T, Q, F, comps.over_point, w, r - 1e-4);
      if (t.blocked()) {
        g_blocked.fetch_add(1, std::memory_order_relaxed);
        continue;
      }
      const double geo = (cos_x * cos_e) / ((flags & kNoPi) ? r2 : RTC_PI * r2);
      double term[3] = {((R[12] * R[15]) * geo) * t.r, ((R[13] * R[15]) * geo) * t.g, ((R[14] * R[15]) * geo) * t.b};
      for (int c = 0; c < 3; ++c) {
        double sigma = A.fog_density;
        if (medium != media::kNoMedium) sigma = A.absorption.empty() ? 0.0 : A.absorption[3 * static_cast<size_t>(medium) + c];
        if (sigma != 0.0) term[c] = term[c] * std::exp(-(sigma * r));
        sum[c] = sum[c] + term[c];
      }
    }
    const double n = static_cast<double>(C.table->samples);
    surface = orc::cadd(surface, orc::Color{(color.r * m.diffuse) * (I.gain * (sum[0] / n)), (color.g * m.diffuse) * (I.gain * (sum[1] / n)),
                                            (color.b * m.diffuse) * (I.gain * (sum[2] / n))});
  }
  // ---- emission (rtc.h): after the last light's, sun's, sky-light and emitter term; nothing counted twice - the ray formed as
  // a diffuse child adds none at a listed leaf
  if (!I.emission.empty()) {
    const double* e = I.emission.data() + 3ull * media::materialOf(T, obj);
    const bool counted = W.diffuse_child && C.list->ids.count(obj->id) != 0;
    if (counted) g_suppressed.fetch_add(1, std::memory_order_relaxed);
    if (!counted || (C.table->flags & kNoSuppress)) {
      if (e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0) indir::g_emitted.fetch_add(1, std::memory_order_relaxed);
      surface = orc::cadd(surface, orc::Color{e[0], e[1], e[2]});
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
  // ---- the diffuse child's conditions (rtc.h)
  bool do_diffuse = false;
  if (I.gain > 0.0 && m.diffuse != 0.0) {
    if (remaining == 0) {
      indir::g_no_remaining.fetch_add(1, std::memory_order_relaxed);
    } else if (!(W.d < I.bounces)) {
      indir::g_no_bounces.fetch_add(1, std::memory_order_relaxed);
    } else {
      do_diffuse = true;
      indir::g_formed.fetch_add(1, std::memory_order_relaxed);
    }
  }
  const uint64_t kids = (do_reflect ? 1u : 0u) + (do_refract ? 1u : 0u) + (do_diffuse ? 1u : 0u);
  if (kids != 0) indir::notePending(W.pending + kids - 1);
  uint64_t waiting = kids;
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0}, indirect{0.0, 0.0, 0.0};
  if (do_reflect) {
    orc::counters().secondary++;
    if (A.any() && medium != media::kNoMedium) media::g_reflect_in_medium.fetch_add(1, std::memory_order_relaxed);
    orc::Tuple d = comps.reflectv;
    if (rough_r > 0.0) d = gloss::scatter(XG, 2 * code, rough_r, d, ng, false);
    const indir::Walk w{W.d, false, W.pending + --waiting};
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, I, C, X, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                  level + (do_refract ? 1u : 0u), env::kReflected, rough_r > 0.0, w),
                          m.reflective);
  }
  if (do_refract) {
    const double cos_t = std::sqrt(1.0 - sin2_t);
    orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
    orc::counters().secondary++;
    if (A.any()) {
      if (kid_nested) media::g_nested.fetch_add(1, std::memory_order_relaxed);
      if (kid_medium == media::kNoMedium) media::g_exit.fetch_add(1, std::memory_order_relaxed);
    }
    if (do_reflect && level >= 2u) media::g_deep.fetch_add(1, std::memory_order_relaxed);
    if (rough_t > 0.0) direction = gloss::scatter(XG, 2 * code + 1, rough_t, direction, ng, true);
    const indir::Walk w{W.d, false, W.pending + --waiting};
    refracted = orc::cmul(colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, I, C, X, orc::Ray{comps.under_point, direction}, 2 * code + 1,
                                  remaining - 1, J, kid_medium, level, env::kRefracted, rough_t > 0.0, w),
                          m.transparency);
  }
  if (do_diffuse) {
    orc::counters().secondary++;
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    const uint64_t word = (static_cast<uint64_t>(W.d) << occl::kSampleShift) | code;
    const orc::Tuple d = occl::direction([&](uint32_t axis) { return gloss::jitter(XI.h, word, axis); }, ng);
    const indir::Walk w{W.d + 1, true, W.pending + --waiting};
    const orc::Color c = colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, I, C, X, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                 level, indir::kDiffuse, false, w);
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

// indir::colorAt with emit::shadeHit
orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const Ctx& C,
                   const indir::Keys& X, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium,
                   uint32_t level, uint32_t kind, bool rough_parent, const indir::Walk& W) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  media::Step st;
  if (A.any()) st = media::segment(A, medium, ray, h >= 0, h >= 0 ? xs[h].t : 0.0);
  if (h < 0) {
    const orc::Color in = st.fog ? orc::Color{st.in[0], st.in[1], st.in[2]} : orc::Color{0.0, 0.0, 0.0};
    if (!skyl::hasSky(E)) return in;
    if (W.diffuse_child && Y.gain > 0.0) {
      indir::g_suppressed.fetch_add(1, std::memory_order_relaxed);
      return in;
    }
    orc::Color e = env::sky(S, U, E, ray);
    if (A.any()) e = {e.r * st.t[0], e.g * st.t[1], e.b * st.t[2]};
    if (st.t[0] == 0.0 && st.t[1] == 0.0 && st.t[2] == 0.0) {
      env::g_miss_dark.fetch_add(1, std::memory_order_relaxed);
    } else {
      (kind == env::kCamera ? env::g_miss_camera
                            : (kind == env::kReflected ? env::g_miss_reflected : (kind == env::kRefracted ? env::g_miss_refracted : indir::g_miss_diffuse)))
          .fetch_add(1, std::memory_order_relaxed);
      if (rough_parent) env::g_miss_rough.fetch_add(1, std::memory_order_relaxed);
    }
    return st.fog ? orc::Color{in.r + e.r, in.g + e.g, in.b + e.b} : e;
  }
  const meshuv::Hit H = meshuv::hitOf(M, U, xs[h], ray);
  const orc::PreComputations comps = torus::precompute(M, T, Q, xs[h], ray, xs);
  orc::Tuple ng = torus::normalAt(Q, xs[h].object, motion::shift(comps.point, M.t, motion::dispOf(M, xs[h].object)), xs[h]);
  if (comps.inside) ng = orc::negate(ng);
  uint32_t kid_medium = media::kNoMedium;
  bool kid_nested = false;
  const orc::Shape* s2 = media::n2Shape(xs[h], xs);
  if ((s2 ? s2->material.refractive_index : 1.0) != comps.n2) throw std::runtime_error("emitter checker: the containers walk disagrees with n2");
  if (s2) {
    kid_medium = media::materialOf(T, s2);
    kid_nested = s2->id != xs[h].object->id;
  }
  const orc::Color c = shadeHit(S, M, K, T, Q, U, G, O, F, A, E, Y, I, C, X, H, comps, ng, code, remaining, J, medium, kid_medium, kid_nested, level, W);
  if (!A.any()) return c;
  orc::Color out{c.r * st.t[0], c.g * st.t[1], c.b * st.t[2]};
  if (st.fog) out = {st.in[0] + out.r, st.in[1] + out.g, st.in[2] + out.b};
  return out;
}

constexpr uint32_t kCounters = indir::kCounters + 7;

// indir::render's pixel loop with emit::colorAt; counters_out: indir::render's 44, then [samples drawn, skipped by cos_x, by
// cos_e, by r, walks made, walks blocked, emissions suppressed]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
           const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const Table& EM, uint32_t x0, uint32_t y0,
           uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const motion::Motion base = motion::make(S, disp, n_roots);
    const camsmp::Sampling smp = camsmp::from(sampling);
    const uint32_t n_samples = smp.grid * smp.grid;
    if ((static_cast<uint64_t>(pass) + 1) * n_samples > (1ull << 24)) throw std::runtime_error("InvalidArgument: pass");
    const uint64_t n_pixels = static_cast<uint64_t>(cam->hsize) * cam->vsize;
    indir::Keys keys;
    keys.gloss = gloss::keyOf(G.seed);
    keys.occl = occl::keyOf(O.seed);
    keys.skyl = skyl::keyOf(Y.seed);
    keys.indir = indir::keyOf(I.seed);
    const List list = EM.on ? makeList(S, T, F, I, EM.flags) : List{};
    Ctx ctx;
    ctx.table = &EM;
    ctx.list = &list;
    ctx.key = keyOf(EM.seed);
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    std::atomic<uint64_t>* const zeroed[] = {
        &gloss::g_used, &gloss::g_fell, &occl::g_occluded, &occl::g_clear, &occl::g_skipped, &occl::g_deep, &sfilt::g_clear, &sfilt::g_partial,
        &sfilt::g_blocked, &sfilt::g_three, &sfilt::g_three_partial, &sfilt::g_factors, &sfilt::g_at_light, &media::g_seg_atmosphere,
        &media::g_seg_medium, &media::g_seg_tinted, &media::g_miss_in_medium, &media::g_reflect_in_medium, &media::g_nested, &media::g_exit,
        &media::g_deep, &env::g_miss_camera, &env::g_miss_reflected, &env::g_miss_refracted, &env::g_miss_rough, &env::g_miss_dark,
        &env::g_sun_clear, &env::g_sun_blocked, &env::g_sun_partial, &env::g_sun_behind, &env::g_sun_only, &skyl::g_clear, &skyl::g_partial,
        &skyl::g_blocked, &skyl::g_skipped, &skyl::g_deep, &indir::g_formed, &indir::g_no_remaining, &indir::g_no_bounces, &indir::g_suppressed,
        &indir::g_miss_diffuse, &indir::g_max_pending, &indir::g_emitted, &g_drawn, &g_skip_cos_x, &g_skip_cos_e, &g_skip_r, &g_walks, &g_blocked,
        &g_suppressed};
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
              indir::Keys X = keys;
              X.p = p;
              X.g = g;
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, G, O, F, A, E, Y, I, ctx, X, motion::passRay(camera, smp, x, y, k, g), 1, max_depth,
                                           J, media::kNoMedium, 0u, env::kCamera, false, indir::Walk{}));
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
          &skyl::g_deep, &indir::g_formed, &indir::g_no_remaining, &indir::g_no_bounces, &indir::g_suppressed, &indir::g_miss_diffuse,
          &indir::g_max_pending, &indir::g_emitted, &g_drawn, &g_skip_cos_x, &g_skip_cos_e, &g_skip_r, &g_walks, &g_blocked, &g_suppressed};
      static_assert(3 + sizeof(reported) / sizeof(reported[0]) == kCounters, "indir::render's 44 counters, then this checker's seven");
      uint32_t at = 3;
      for (const std::atomic<uint64_t>* c : reported) counters_out[at++] = c->load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace emit

extern "C" {

// The emitter table (e NULL: no table).  `flags`: the variants of the sample step and of the suppression rule (0: rtc.h's).
// Refuses what rtc_scene_set_emitters refuses of the table's own values.
int emit_table_create(const rtc_emitters* e, uint32_t flags, void** out) {
  try {
    auto t = std::make_unique<emit::Table>();
    if (e) {
      if (e->samples < 1u || e->samples > RTC_EMITTER_MAX_SAMPLES) throw std::runtime_error("InvalidArgument: samples");
      t->on = true;
      t->samples = e->samples;
      t->seed = e->seed;
      t->flags = flags;
    }
    *out = t.release();
    return 0;
  } catch (const std::exception& ex) {
    g_error = ex.what();
    return 1;
  }
}
void emit_table_destroy(void* t) { delete static_cast<emit::Table*>(t); }
uint32_t emit_counters(void) { return emit::kCounters; }

// The checker's own emitter list for a scene, its material map (the bump table), a filter table and an indirect table:
// rows[18 k ...] and cdf[k] in rtc_diag_emitters' layout; *count the entries (capacity too small: only *count).
int emit_list(void* scene, void* bumps, void* sf, void* in, uint32_t capacity, double* rows, double* cdf, uint32_t* count) {
  try {
    const emit::List l = emit::makeList(*static_cast<area::Scene*>(scene), *static_cast<bump::Table*>(bumps), *static_cast<sfilt::Table*>(sf),
                                        *static_cast<indir::Table*>(in), 0u);
    *count = static_cast<uint32_t>(l.size());
    if (capacity >= l.size()) {
      if (rows) std::copy(l.row.begin(), l.row.end(), rows);
      if (cdf) std::copy(l.cdf.begin(), l.cdf.end(), cdf);
    }
    return 0;
  } catch (const std::exception& ex) {
    g_error = ex.what();
    return 1;
  }
}

// rtc.h's pick, by a linear scan
uint32_t emit_pick(const double* cdf, uint32_t n, double total, double u0) { return emit::pick(cdf, n, total, u0); }

// The scene and the tables: as indir_render's; and the emitter table.  counters_out: emit_counters() entries.
int emit_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, void* sf, void* me, void* ev, void* sl, void* in, void* em,
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
  return emit::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                      *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                      *static_cast<occl::Table*>(oc), *static_cast<sfilt::Table*>(sf), *static_cast<media::Table*>(me),
                      *static_cast<env::Table*>(ev), *static_cast<skyl::Table*>(sl), *static_cast<indir::Table*>(in),
                      *static_cast<emit::Table*>(em), x0, y0, w, h, n_threads, rgb_out, counters_out);
}

}  // extern "C"
