// meshuv_oracle.cpp — CPU checker of UV-mapped mesh textures (libmeshuv_oracle.so).  TEST INFRASTRUCTURE.
//
// The mesh mapping (include/rtc.h RTC_TEX_MESH) on top of the torus checker: torus_oracle.cpp is
// included, read-only, and with it the bump, spot, motion, camera-sampling and area-light checkers and the oracle's sources.
// The oracle's TextureMap is a closed switch without a mesh mapping, so the checker receives its scene with every mesh map
// replaced by a placeholder planar map - same uv pattern, same place in the pattern tree - and a side table: which tex_*
// entries are mesh maps, and Shape.id -> the triangle's texture row.  What is restated here is what the mapping changes:
//   - Pattern.patternAt for a tree in which a mesh map can be reached (the placeholder's planar (u, v) never is computed);
//   - the hit's barycentrics, by the checker's own Moller-Trumbore on the winning intersection's triangle (the oracle keeps
//     (u, v) for smooth triangles only), and (tu, tv) of rtc.h from them and the row;
//   - through them shadeHit, colorAt and the pass loop, as torus_oracle.cpp has them.
// Everything after (tu, tv) - align check, uv checkers, uv image, uv test - is the oracle's UvPattern.uvPatternAt.
// Nothing of the product is included or linked.
#include <array>

#include "torus_oracle.cpp"

namespace meshuv {

struct Table {
  std::vector<uint8_t> is_mesh;                               // [n_texmaps]; empty: no mesh map
  std::unordered_map<size_t, std::array<double, 6>> row_of;  // a triangle's Shape.id -> (a1, b1, a2, b2, a3, b3)
};

// What the whole pattern evaluation of one hit holds constant
struct Hit {
  double row[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double u = 0.0, v = 0.0;
};

// rtc.h, RTC_TEX_MESH: (tu, tv) of a row at the barycentrics (u, v)
void texcoord(const double row[6], double u, double v, double* tu, double* tv) {
  const double a1 = row[0], b1 = row[1], a2 = row[2], b2 = row[3], a3 = row[4], b3 = row[5];
  const double w = (1.0 - u) - v;
  double x = (a2 * u + a3 * v) + a1 * w;
  double y = (b2 * u + b3 * v) + b1 * w;
  if (x < 0.0 || x > 1.0) x = x - std::floor(x);
  if (y < 0.0 || y > 1.0) y = y - std::floor(y);
  *tu = x;
  *tv = y;
}

// Moller-Trumbore (triangle.zig:29-63, 225-259) of the ray `lr`, in the triangle's object space: the barycentrics of its
// entry.  false: the ray has none.
bool barycentrics(const orc::Shape& s, const orc::Ray& lr, double* u_out, double* v_out) {
  const orc::Tuple dir_cross_e2 = orc::cross(lr.direction, s.e2);
  const double det = orc::dot(s.e1, dir_cross_e2);
  if (std::fabs(det) < 1e-5) return false;
  const double f = 1.0 / det;
  const orc::Tuple p1_to_origin = orc::sub(lr.origin, s.p1);
  const double u = f * orc::dot(p1_to_origin, dir_cross_e2);
  if (u < 0.0 || u > 1.0) return false;
  const orc::Tuple p1_to_origin_cross_e1 = orc::cross(p1_to_origin, s.e1);
  const double v = f * orc::dot(lr.direction, p1_to_origin_cross_e1);
  if (v < 0.0 || (u + v) > 1.0) return false;
  *u_out = u;
  *v_out = v;
  return true;
}

// The hit's constants: a triangle with a row gets it and its entry's barycentrics, anything else six zeros and (0, 0).
// The entry is the one the root's own ray - shifted by the root's displacement, as motion::intersect tests it - produced.
Hit hitOf(const motion::Motion& M, const Table& U, const orc::Intersection& h, const orc::Ray& ray) {
  Hit H;
  const orc::Shape* s = h.object;
  if (s->kind != orc::TRIANGLE && s->kind != orc::SMOOTH_TRIANGLE) return H;
  const auto it = U.row_of.find(s->id);
  if (it == U.row_of.end()) return H;
  const orc::Ray rr{motion::shift(ray.origin, M.t, motion::dispOf(M, s)), ray.direction};
  if (!barycentrics(*s, rr.transform(s->inverse), &H.u, &H.v)) throw std::runtime_error("meshuv checker: the hit triangle has no entry");
  for (int k = 0; k < 6; ++k) H.row[k] = it->second[k];
  return H;
}

bool isMeshMap(const area::Scene& S, const Table& U, const orc::TextureMap* tm) {
  if (U.is_mesh.empty()) return false;
  const size_t i = static_cast<size_t>(tm - S.os->texmaps.data());
  return i < U.is_mesh.size() && U.is_mesh[i] != 0;
}

// Pattern.patternAt (pattern.zig:112-124, rtc_oracle.hpp) with the mesh mapping: sub-patterns at the OBJECT point with
// their own inverse; a mesh map at (tu, tv), its own inverse not applied to them.
orc::Color patternAt(const area::Scene& S, const Table& U, const Hit& H, const orc::Pattern& p, orc::Tuple object_point) {
  const orc::Tuple pp = p.inverse.tupleMul(object_point);
  auto sub = [&](const orc::Pattern* q, orc::Tuple at) { return patternAt(S, U, H, *q, at); };
  switch (p.kind) {
    case orc::PAT_SOLID: return p.rgb;
    case orc::PAT_TEST: return {pp.x, pp.y, pp.z};
    case orc::PAT_STRIPES: return (orc::zigMod(pp.x, 2.0) < 1.0) ? sub(p.a, object_point) : sub(p.b, object_point);
    case orc::PAT_CHECKERS:
      return (orc::zigMod(std::floor(pp.x) + std::floor(pp.y) + std::floor(pp.z), 2.0) < 1.0) ? sub(p.a, object_point) : sub(p.b, object_point);
    case orc::PAT_RINGS:
      return (orc::zigMod(std::floor(std::sqrt(pp.x * pp.x + pp.z * pp.z)), 2.0) < 1.0) ? sub(p.a, object_point) : sub(p.b, object_point);
    case orc::PAT_GRADIENT: {
      const orc::Color ca = sub(p.a, object_point), cb = sub(p.b, object_point);
      const orc::Color distance{cb.r - ca.r, cb.g - ca.g, cb.b - ca.b};
      const double fraction = pp.x - std::floor(pp.x);
      return orc::cadd(ca, orc::cmul(distance, fraction));
    }
    case orc::PAT_RADIAL_GRADIENT: {
      const orc::Color ca = sub(p.a, object_point), cb = sub(p.b, object_point);
      const orc::Color distance{cb.r - ca.r, cb.g - ca.g, cb.b - ca.b};
      const double mag = std::sqrt(pp.x * pp.x + pp.z * pp.z);
      const double fraction = mag - std::floor(mag);
      return orc::cadd(ca, orc::cmul(distance, fraction));
    }
    case orc::PAT_BLEND: {
      const orc::Color ca = sub(p.a, object_point), cb = sub(p.b, object_point);
      return orc::cmul(orc::cadd(ca, cb), 0.5);
    }
    case orc::PAT_TEXTURE_MAP: {
      if (!isMeshMap(S, U, p.texture_map)) return p.texture_map->patternAt(pp, object_point);
      double tu, tv;
      texcoord(H.row, H.u, H.v, &tu, &tv);
      return p.texture_map->faces[0].uvPatternAt(tu, tv, object_point);
    }
    case orc::PAT_PERTURB: {
      const unsigned octaves = static_cast<unsigned>(p.rgb.g);
      const orc::Tuple offset = orc::vec3(orc::octaveNoise(object_point.x, object_point.y, object_point.z, octaves, p.rgb.b),
                                          orc::octaveNoise(object_point.x, object_point.y, object_point.z + 1.0, octaves, p.rgb.b),
                                          orc::octaveNoise(object_point.x, object_point.y, object_point.z + 2.0, octaves, p.rgb.b));
      return sub(p.a, orc::add(object_point, orc::mul(offset, p.rgb.r)));
    }
    default: throw std::runtime_error("meshuv checker: unsupported pattern kind");
  }
}

// motion::colorAtPoint with meshuv::patternAt
orc::Color colorAtPoint(const area::Scene& S, const motion::Motion& M, const Table& U, const Hit& H, const orc::Shape* obj, orc::Tuple pt) {
  return patternAt(S, U, H, obj->material.pattern, obj->worldToObject(motion::shift(pt, M.t, motion::dispOf(M, obj))));
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const Table& U, const orc::Ray& ray, size_t remaining, const area::Jitter& J);

// torus::shadeHit with meshuv::colorAtPoint and colorAt
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                    const torus::Table& Q, const Table& U, const Hit& H, const orc::PreComputations& comps, size_t remaining,
                    const area::Jitter& J) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  for (uint32_t l = 0; l < S.lights.size(); ++l) {
    const area::Light& L = S.lights[l];
    const orc::Color color = colorAtPoint(S, M, U, H, obj, comps.over_point);
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
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    reflected = orc::cmul(colorAt(S, M, K, T, Q, U, orc::Ray{comps.over_point, comps.reflectv}, remaining - 1, J), m.reflective);
  }
  {  // world.zig:171-189
    const double n_ratio = comps.n1 / comps.n2;
    const double cos_i = orc::dot(comps.eyev, comps.normal);
    const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
    if (!(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0) {
      const double cos_t = std::sqrt(1.0 - sin2_t);
      const orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
      orc::counters().secondary++;
      refracted = orc::cmul(colorAt(S, M, K, T, Q, U, orc::Ray{comps.under_point, direction}, remaining - 1, J), m.transparency);
    }
  }
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T,
                   const torus::Table& Q, const Table& U, const orc::Ray& ray, size_t remaining, const area::Jitter& J) {
  const orc::Intersections xs = torus::intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  if (h < 0) return {0.0, 0.0, 0.0};
  const Hit H = hitOf(M, U, xs[h], ray);
  return shadeHit(S, M, K, T, Q, U, H, torus::precompute(M, T, Q, xs[h], ray, xs), remaining, J);
}

// torus::render's pixel loop with meshuv::colorAt
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T,
           const torus::Table& Q, const Table& U, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out,
           uint64_t* counters_out) {
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
            for (uint32_t k = 0; k < n_samples; ++k) {
              const uint64_t g = static_cast<uint64_t>(pass) * n_samples + k;
              orc::counters().primary++;
              area::Jitter J;
              J.seed = light_seed;
              J.pixel = (pass * n_pixels + p) * n_samples + k;  // (u64, wraps)
              J.n_lights = S.lights.size();
              M.t = motion::time(smp.seed, p, g);
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, U, motion::passRay(camera, smp, x, y, k, g), max_depth, J));
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
    }
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // namespace meshuv

extern "C" {

// The side table: is_mesh[i] != 0 for every tex_* entry that is a mesh map in the product's description (n_texmaps == 0:
// none), and n_rows texture rows, rows[6 i ..] belonging to the triangle whose Shape.id (leaf_id) is ids[i].
int meshuv_table_create(const uint8_t* is_mesh, uint32_t n_texmaps, const size_t* ids, const double* rows, uint32_t n_rows, void** out) {
  try {
    auto t = std::make_unique<meshuv::Table>();
    t->is_mesh.assign(is_mesh, is_mesh + n_texmaps);
    for (uint32_t i = 0; i < n_rows; ++i) {
      std::array<double, 6> r;
      for (int k = 0; k < 6; ++k) {
        r[k] = rows[6ull * i + k];
        if (!std::isfinite(r[k])) throw std::runtime_error("InvalidArgument: a texture coordinate that is not finite");
      }
      t->row_of[ids[i]] = r;
    }
    *out = t.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void meshuv_table_destroy(void* t) { delete static_cast<meshuv::Table*>(t); }

// The scene (with placeholders of both kinds), the bump table and the torus table: as torus_render's; and the side table.
int meshuv_render(void* scene, void* bumps, void* tori, void* uvs, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed,
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
  return meshuv::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                        *static_cast<torus::Table*>(tori), *static_cast<meshuv::Table*>(uvs), x0, y0, w, h, n_threads, rgb_out,
                        counters_out);
}

// ---- KAT hook: (tu, tv) of n rows at n barycentrics (rows: [n][6]; u, v: [n]) into out[n][2]
void meshuv_kat_texcoord_many(const double* rows, const double* u, const double* v, uint32_t n, double* out) {
  for (uint32_t i = 0; i < n; ++i) meshuv::texcoord(rows + 6ull * i, u[i], v[i], out + 2ull * i, out + 2ull * i + 1);
}

}  // extern "C"
