// mis_oracle.cpp — CPU checker of multiple importance sampling (libmis_oracle.so).  TEST INFRASTRUCTURE.
//
// Emitter samples and diffuse children combined by the balance heuristic (include/rtc.h rtc_scene_set_emitter_mis, DESIGN.md
// section 32) on top of the emitter-sampling checker: emitters_oracle.cpp is included, read-only, and with it every checker
// below it and the oracle's sources.  What is restated here, as plain recursion:
//   - which entry of the emitter list belongs to which face of which leaf: the list's derivation walked once more over the
//     oracle's own scene build, with the face of every entry that emit::makeList kept;
//   - the two weights, rtc.h's a = q * (cos_s * cos_e), b = n * (pi * r2), w_e = b / (b + a), w_b = a / (b + a);
//   - shadeHit, as emitters_oracle.cpp has it, with w_e on every sample's term and, at the hit of a ray formed as a diffuse
//     child on a listed leaf, the emission row times w_b - the face by the reference's rule for cube normals on the
//     object-space hit point, the normal and q from that face's row, cos_b carried from where the child was formed;
//   - colorAt and the pass loop, which name them.
// With mode 0 the render is emit::render's bit for bit.  Three counters beside the emitter checker's: child hits weighted;
// child hits with w_b = 1 by a skip rule (cos_b <= 0, cos_e' == 0, t <= 2e-4, or a face the list leaves out); and the largest
// |w_e + w_b - 1| over every sample that made a walk, where both weights are evaluated for the sampled direction (reported
// as the bits of a double).  Two variants exist for the tests that show each mistake missing its bound: kChildSuppressed
// weights the samples and keeps the child's emission suppressed, kChildFull weights the samples and adds the child's whole
// row.  Nothing of the product is included or linked.
#include "emitters_oracle.cpp"

#include <array>
#include <unordered_map>

namespace mis {

constexpr uint32_t kChildSuppressed = 1u, kChildFull = 2u;  // the variants (tests only)

struct Table {
  uint32_t mode = 0;   // rtc_scene_set_emitter_mis' mode
  uint32_t flags = 0;  // a variant (0: rtc.h's rules)
};

using emit::kRow;
using emit::pick;
using emit::List;
using emit::sampleWalk;
using emit::g_blocked;
using emit::g_drawn;
using emit::g_skip_cos_e;
using emit::g_skip_cos_x;
using emit::g_skip_r;
using emit::g_suppressed;
using emit::g_walks;

std::atomic<uint64_t> g_weighted{0}, g_whole{0}, g_partition{0};  // (g_partition: the bits of a non-negative double, whose order is the integers')

// rtc.h's weights
void weights(double n, double q, double cos_s, double cos_e, double r2, double& w_e, double& w_b) {
  const double a = q * (cos_s * cos_e);
  const double b = n * (RTC_PI * r2);
  const double s = b + a;
  w_e = b / s;
  w_b = a / s;
}

void notePartition(double w_e, double w_b) {
  const double e = std::fabs((w_e + w_b) - 1.0);
  uint64_t bits;
  std::memcpy(&bits, &e, sizeof bits);
  uint64_t seen = g_partition.load(std::memory_order_relaxed);
  while (bits > seen && !g_partition.compare_exchange_weak(seen, bits, std::memory_order_relaxed)) {
  }
}

// The entries of every listed leaf, by face: a cube's +x, -x, +y, -y, +z, -z, a triangle's at 0; -1: the list has none.
// The list's own derivation walked again (emit::listShape's conditions and its weight rule, on the rows it made): a leaf's
// entries are consecutive and in face order, and a face is left out exactly where its w is not finite or not above zero.
using Faces = std::unordered_map<size_t, std::array<int, 6>>;  // by Shape.id

void facesOfShape(const orc::Shape& s, const List& L, uint32_t& next_leaf, size_t& next_entry, Faces& out) {
  if (s.kind == orc::GROUP || s.kind == orc::CSG) {
    for (const orc::Shape& c : s.children) facesOfShape(c, L, next_leaf, next_entry, out);
    return;
  }
  const uint32_t leaf = next_leaf++;
  if (L.ids.count(s.id) == 0) return;
  std::array<int, 6> f{-1, -1, -1, -1, -1, -1};
  // (the leaf's entries: those that name it; which face each is follows from the order and from the face's own geometry -
  // the entry of axis a has its eu along axis (a + 1) mod 3 in object space and its origin at +1 or -1 on a)
  while (next_entry < L.size() && static_cast<uint32_t>(L.row[kRow * next_entry + 17]) == leaf) {
    const double* R = L.row.data() + kRow * next_entry;
    int face = 0;
    if (s.kind == orc::CUBE) {
      const orc::Tuple eu = s.inverse.tupleMul(orc::vec3(R[3], R[4], R[5]));
      const orc::Tuple o = s.inverse.tupleMul(orc::point(R[0], R[1], R[2]));
      const double e[3] = {std::fabs(eu.x), std::fabs(eu.y), std::fabs(eu.z)};
      const int b = e[0] >= e[1] && e[0] >= e[2] ? 0 : (e[1] >= e[2] ? 1 : 2);
      const int a = (b + 2) % 3;
      const double oa = a == 0 ? o.x : (a == 1 ? o.y : o.z);
      face = 2 * a + (oa > 0.0 ? 0 : 1);
    }
    if (f[face] != -1) throw std::runtime_error("mis checker: two entries for one face");
    f[face] = static_cast<int>(next_entry);
    ++next_entry;
  }
  out.emplace(s.id, f);
}

Faces makeFaces(const area::Scene& S, const List& L) {
  Faces out;
  uint32_t next_leaf = 0;
  size_t next_entry = 0;
  for (const orc::Shape& s : S.os->world.objects) facesOfShape(s, L, next_leaf, next_entry, out);
  if (next_entry != L.size()) throw std::runtime_error("mis checker: the list's entries are not in leaf order");
  return out;
}

struct Ctx {  // what the steps need beside indir's arguments
  const emit::Table* table;
  const List* list;
  const Faces* faces;
  const Table* mis;
  uint64_t key = 0;
};

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const Ctx& C,
                   const indir::Keys& X, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium,
                   uint32_t level, uint32_t kind, bool rough_parent, const indir::Walk& W, double cos_b);

// emit::shadeHit with w_e on the samples' terms, w_b on the emission row a diffuse child meets at a listed leaf, cos_b formed
// with the child, and mis::colorAt
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                    const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const Ctx& C,
                    const indir::Keys& X, const meshuv::Hit& H, const orc::PreComputations& comps, orc::Tuple ng, uint64_t code,
                    size_t remaining, const area::Jitter& J, uint32_t medium, uint32_t kid_medium, bool kid_nested, uint32_t level,
                    const indir::Walk& W, double cos_b) {
  const bool mis_on = C.mis->mode != 0u;
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
      const double cos_e = (flags & emit::kNoCosE) ? 1.0 : std::fabs((R[9] * w.x + R[10] * w.y) + R[11] * w.z);
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
      const double geo = (cos_x * cos_e) / ((flags & emit::kNoPi) ? r2 : RTC_PI * r2);
      double base[3] = {(R[12] * R[15]) * geo, (R[13] * R[15]) * geo, (R[14] * R[15]) * geo};
      if (mis_on) {  // rtc.h: the term but for the filter, times w_e
        double w_e, w_b;
        weights(static_cast<double>(C.table->samples), R[15], cos_x, cos_e, r2, w_e, w_b);
        notePartition(w_e, w_b);
        for (int c = 0; c < 3; ++c) base[c] = base[c] * w_e;
      }
      double term[3] = {base[0] * t.r, base[1] * t.g, base[2] * t.b};
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
    if (counted && mis_on && (C.mis->flags & (kChildSuppressed | kChildFull)) == 0u) {
      // rtc.h: the row times w_b; the face, its normal and its q from the list; r = t of the hit; the skip rules keep the row
      double w_b = 1.0;
      const std::array<int, 6>& faces = C.faces->at(obj->id);
      int face = 0;
      if (obj->kind == orc::CUBE) {
        const orc::Tuple lp = obj->inverse.tupleMul(comps.point);
        const double ax = std::fabs(lp.x), ay = std::fabs(lp.y), az = std::fabs(lp.z);
        const double maxc = std::fmax(ax, std::fmax(ay, az));
        if (maxc == ax) face = lp.x < 0.0 ? 1 : 0;
        else if (maxc == ay) face = lp.y < 0.0 ? 3 : 2;
        else face = lp.z < 0.0 ? 5 : 4;
      }
      bool weighted = false;
      if (faces[face] >= 0) {
        const double* R = C.list->row.data() + static_cast<size_t>(kRow) * static_cast<size_t>(faces[face]);
        const orc::Tuple dir = orc::negate(comps.eyev);
        const double t = comps.intersection.t;
        const double cos_e = std::fabs((R[9] * dir.x + R[10] * dir.y) + R[11] * dir.z);
        if (!(cos_b <= 0.0) && !(cos_e == 0.0) && !(t <= 2e-4)) {
          double w_e;
          weights(static_cast<double>(C.table->samples), R[15], cos_b, cos_e, t * t, w_e, w_b);
          weighted = true;
        }
      }
      (weighted ? g_weighted : g_whole).fetch_add(1, std::memory_order_relaxed);
      if (e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0) indir::g_emitted.fetch_add(1, std::memory_order_relaxed);
      surface = orc::cadd(surface, orc::Color{e[0] * w_b, e[1] * w_b, e[2] * w_b});
    } else {
      if (counted) g_suppressed.fetch_add(1, std::memory_order_relaxed);
      const bool whole = (C.table->flags & emit::kNoSuppress) != 0u || (mis_on && (C.mis->flags & kChildFull) != 0u);
      if (!counted || whole) {
        if (e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0) indir::g_emitted.fetch_add(1, std::memory_order_relaxed);
        surface = orc::cadd(surface, orc::Color{e[0], e[1], e[2]});
      }
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
                                  level + (do_refract ? 1u : 0u), env::kReflected, rough_r > 0.0, w, 0.0),
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
                                  remaining - 1, J, kid_medium, level, env::kRefracted, rough_t > 0.0, w, 0.0),
                          m.transparency);
  }
  if (do_diffuse) {
    orc::counters().secondary++;
    const orc::Color color = meshuv::colorAtPoint(S, M, U, H, obj, comps.over_point);
    const uint64_t word = (static_cast<uint64_t>(W.d) << occl::kSampleShift) | code;
    const orc::Tuple d = occl::direction([&](uint32_t axis) { return gloss::jitter(XI.h, word, axis); }, ng);
    const indir::Walk w{W.d + 1, true, W.pending + --waiting};
    const orc::Color c = colorAt(S, M, K, T, Q, U, G, O, F, A, E, Y, I, C, X, orc::Ray{comps.over_point, d}, 2 * code, remaining - 1, J, medium,
                                 level, indir::kDiffuse, false, w, (d.x * ng.x + d.y * ng.y) + d.z * ng.z);  // (cos_b, rtc.h)
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

// emit::colorAt with mis::shadeHit; cos_b: of a ray formed as a diffuse child, else 0
orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
                   const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const Ctx& C,
                   const indir::Keys& X, const orc::Ray& ray, uint64_t code, size_t remaining, const area::Jitter& J, uint32_t medium,
                   uint32_t level, uint32_t kind, bool rough_parent, const indir::Walk& W, double cos_b) {
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
  if ((s2 ? s2->material.refractive_index : 1.0) != comps.n2) throw std::runtime_error("mis checker: the containers walk disagrees with n2");
  if (s2) {
    kid_medium = media::materialOf(T, s2);
    kid_nested = s2->id != xs[h].object->id;
  }
  const orc::Color c = shadeHit(S, M, K, T, Q, U, G, O, F, A, E, Y, I, C, X, H, comps, ng, code, remaining, J, medium, kid_medium, kid_nested, level, W, cos_b);
  if (!A.any()) return c;
  orc::Color out{c.r * st.t[0], c.g * st.t[1], c.b * st.t[2]};
  if (st.fog) out = {st.in[0] + out.r, st.in[1] + out.g, st.in[2] + out.b};
  return out;
}

constexpr uint32_t kCounters = emit::kCounters + 3;

// emit::render's pixel loop with mis::colorAt; counters_out: emit::render's 51, then [child hits weighted, child hits that kept
// the whole row by a skip rule, the bits of the largest |w_e + w_b - 1|]
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const meshuv::Table& U, const gloss::Table& G, const occl::Table& O, const sfilt::Table& F,
           const media::Table& A, const env::Table& E, const skyl::Table& Y, const indir::Table& I, const emit::Table& EM, const Table& MI, uint32_t x0, uint32_t y0,
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
    const List list = EM.on ? emit::makeList(S, T, F, I, EM.flags) : List{};
    const Faces faces = makeFaces(S, list);
    Ctx ctx;
    ctx.table = &EM;
    ctx.list = &list;
    ctx.faces = &faces;
    ctx.mis = &MI;
    ctx.key = emit::keyOf(EM.seed);
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    std::atomic<uint64_t>* const zeroed[] = {
        &gloss::g_used, &gloss::g_fell, &occl::g_occluded, &occl::g_clear, &occl::g_skipped, &occl::g_deep, &sfilt::g_clear, &sfilt::g_partial,
        &sfilt::g_blocked, &sfilt::g_three, &sfilt::g_three_partial, &sfilt::g_factors, &sfilt::g_at_light, &media::g_seg_atmosphere,
        &media::g_seg_medium, &media::g_seg_tinted, &media::g_miss_in_medium, &media::g_reflect_in_medium, &media::g_nested, &media::g_exit,
        &media::g_deep, &env::g_miss_camera, &env::g_miss_reflected, &env::g_miss_refracted, &env::g_miss_rough, &env::g_miss_dark,
        &env::g_sun_clear, &env::g_sun_blocked, &env::g_sun_partial, &env::g_sun_behind, &env::g_sun_only, &skyl::g_clear, &skyl::g_partial,
        &skyl::g_blocked, &skyl::g_skipped, &skyl::g_deep, &indir::g_formed, &indir::g_no_remaining, &indir::g_no_bounces, &indir::g_suppressed,
        &indir::g_miss_diffuse, &indir::g_max_pending, &indir::g_emitted, &g_drawn, &g_skip_cos_x, &g_skip_cos_e, &g_skip_r, &g_walks, &g_blocked,
        &g_suppressed, &g_weighted, &g_whole, &g_partition};
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
                                           J, media::kNoMedium, 0u, env::kCamera, false, indir::Walk{}, 0.0));
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
          &indir::g_max_pending, &indir::g_emitted, &g_drawn, &g_skip_cos_x, &g_skip_cos_e, &g_skip_r, &g_walks, &g_blocked, &g_suppressed,
          &g_weighted, &g_whole, &g_partition};
      static_assert(3 + sizeof(reported) / sizeof(reported[0]) == kCounters, "emit::render's 51 counters, then this checker's three");
      uint32_t at = 3;
      for (const std::atomic<uint64_t>* c : reported) counters_out[at++] = c->load();
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace mis

extern "C" {

uint32_t mis_counters(void) { return mis::kCounters; }

// rtc.h's weights for one direction, the skip rules applied as rtc_diag_mis_weights applies them
void mis_weights(uint32_t samples, double q, double cos_s, double cos_e, double r, double* w_e, double* w_b) {
  *w_e = 0.0;
  *w_b = 1.0;
  if (!(cos_s <= 0.0) && !(cos_e == 0.0) && !(r <= 2e-4)) mis::weights(static_cast<double>(samples), q, cos_s, cos_e, r * r, *w_e, *w_b);
}

// The scene and the tables: as emit_render's; `mode`: rtc_scene_set_emitter_mis' (anything but 0 and 1 is refused); `variant`:
// 0, or a variant of the checker.  counters_out: mis_counters() entries.
int mis_render(void* scene, void* bumps, void* tori, void* uvs, void* gl, void* oc, void* sf, void* me, void* ev, void* sl, void* in, void* em,
               uint32_t mode, uint32_t variant, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
               uint32_t pass, const double* disp, uint32_t n_roots, const uint8_t* cone, const double* axis, const double* cos_inner,
               const double* cos_outer, uint32_t n_lights, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads,
               double* rgb_out, uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  std::vector<spot::Cone> cones;
  try {
    if (mode > 1u) throw std::runtime_error("InvalidArgument: mis mode");
    cones = spot::make(S, cone, axis, cos_inner, cos_outer, n_lights);
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
  mis::Table MI;
  MI.mode = mode;
  MI.flags = variant;
  return mis::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                     *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), *static_cast<gloss::Table*>(gl),
                     *static_cast<occl::Table*>(oc), *static_cast<sfilt::Table*>(sf), *static_cast<media::Table*>(me),
                     *static_cast<env::Table*>(ev), *static_cast<skyl::Table*>(sl), *static_cast<indir::Table*>(in),
                     *static_cast<emit::Table*>(em), MI, x0, y0, w, h, n_threads, rgb_out, counters_out);
}

}  // extern "C"
