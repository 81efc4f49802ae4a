// bump_oracle.cpp — CPU checker of normal perturbation (libbump_oracle.so).  TEST INFRASTRUCTURE.
//
// Materials whose shading normal is bumped (include/rtc.h rtc_scene_set_bumps) on top of the
// spot-light checker: spot_oracle.cpp is included, read-only, and with it the motion, camera-sampling and area-light
// checkers and the oracle's sources.  What is restated here is only what bumps change:
//   - PreComputations' normal step: the geometric normal ng stays the motion checker's (inside, over_point, under_point,
//     n1 / n2); the shading normal ns - the unit local normal plus the field at B * local point times the amplitude,
//     through normalToWorld, negated by the same `inside` - replaces `normal` and feeds reflectv;
//   - through it shadeHit (lighting of point, spot and area lights, cos_i and the refracted direction, schlick), colorAt,
//     and the pass loop that calls colorAt.
// Intersection, patterns, isShadowed, the cone's factor, area lighting and the sample rays are the included checkers'.
// Nothing of the product is included or linked.
#include "spot_oracle.cpp"

namespace bump {

struct Row {
  uint8_t kind = RTC_BUMP_NONE;
  double amplitude = 0.0;
  uint32_t octaves = 3;
  double persistence = 0.8;
  double inv[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
};

struct Table {
  std::vector<Row> rows;                         // per material row (mat_* order)
  std::unordered_map<size_t, uint32_t> mat_of;   // a leaf's Shape.id -> its material row
};

// The field at q, each operation correctly rounded (-ffp-contract=off), in the order rtc.h writes them
void field(uint32_t kind, const double q[3], uint32_t octaves, double persistence, double d[3]) {
  d[0] = d[1] = d[2] = 0.0;
  if (kind == RTC_BUMP_NOISE) {
    d[0] = orc::octaveNoise(q[0], q[1], q[2], octaves, persistence);
    d[1] = orc::octaveNoise(q[0], q[1], q[2] + 1.0, octaves, persistence);
    d[2] = orc::octaveNoise(q[0], q[1], q[2] + 2.0, octaves, persistence);
  } else if (kind == RTC_BUMP_RIPPLES) {
    const double r = std::sqrt(q[0] * q[0] + q[2] * q[2]);
    if (r == 0.0) return;
    const double v = 2.0 * (r - std::floor(r)) - 1.0;
    const double h = (4.0 * v) * (1.0 - std::fabs(v));
    d[0] = h * (q[0] / r);
    d[2] = h * (q[2] / r);
  }
}

// Step 2 of the contract: ns of the local normal ln at the local point lp of `obj`, given ng and step 1's `inside`
orc::Tuple shadingNormal(const orc::Shape* obj, orc::Tuple ln, orc::Tuple lp, orc::Tuple ng, bool inside, const Row& R) {
  if (R.kind == RTC_BUMP_NONE || R.amplitude == 0.0) return ng;  // the unperturbed branch
  const double m = std::sqrt((ln.x * ln.x + ln.y * ln.y) + ln.z * ln.z);
  if (m == 0.0) return ng;
  const double q[3] = {((R.inv[0] * lp.x + R.inv[1] * lp.y) + R.inv[2] * lp.z) + R.inv[3],
                       ((R.inv[4] * lp.x + R.inv[5] * lp.y) + R.inv[6] * lp.z) + R.inv[7],
                       ((R.inv[8] * lp.x + R.inv[9] * lp.y) + R.inv[10] * lp.z) + R.inv[11]};
  double d[3];
  field(R.kind, q, R.octaves, R.persistence, d);
  const orc::Tuple bumped = orc::vec3(ln.x / m + d[0] * R.amplitude, ln.y / m + d[1] * R.amplitude, ln.z / m + d[2] * R.amplitude);
  const orc::Tuple ns = obj->normalToWorld(bumped);
  return inside ? orc::negate(ns) : ns;
}

const Row& rowOf(const Table& T, const orc::Shape* obj) {
  const auto it = T.mat_of.find(obj->id);
  if (it == T.mat_of.end()) throw std::runtime_error("bump checker: a hit on a shape that is no leaf of the description");
  return T.rows[it->second];
}

// PreComputations.new (world.zig:212-270): the motion checker's, then `normal` and `reflectv` from ns
orc::PreComputations precompute(const motion::Motion& M, const Table& T, const orc::Intersection& h, const orc::Ray& ray,
                                const orc::Intersections& xs) {
  orc::PreComputations c = motion::precompute(M, h, ray, xs);
  const Row& R = rowOf(T, h.object);
  if (R.kind == RTC_BUMP_NONE || R.amplitude == 0.0) return c;
  const orc::Tuple lp = h.object->worldToObject(motion::shift(c.point, M.t, motion::dispOf(M, h.object)));
  const orc::Tuple ln = h.object->localNormalAt(lp, h);
  c.normal = shadingNormal(h.object, ln, lp, c.normal, c.inside, R);
  c.reflectv = orc::reflect(ray.direction, c.normal);
  return c;
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const Table& T, const orc::Ray& ray,
                   size_t remaining, const area::Jitter& J);

// spot::shadeHit with bump::colorAt below it: comps.normal is ns, comps.over_point / under_point come from ng
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const Table& T,
                    const orc::PreComputations& comps, size_t remaining, const area::Jitter& J) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  for (uint32_t l = 0; l < S.lights.size(); ++l) {
    const area::Light& L = S.lights[l];
    const orc::Color color = motion::colorAtPoint(M, obj, comps.over_point);
    if (!L.is_area) {
      const orc::Tuple point_to_light = orc::normalized(orc::sub(L.corner, comps.over_point));
      const double f = spot::coneFactor(K[l], point_to_light);
      if (f == 0.0) {
        surface = orc::cadd(surface, orc::cmul(orc::cemul(color, L.intensity), m.ambient));
        continue;
      }
      const bool shadowed = motion::isShadowed(S, M, comps.over_point, L.corner);
      surface = orc::cadd(surface, spot::spotLighting(m, color, L, point_to_light, comps.eyev, comps.normal, shadowed, f));
    } else {
      surface = orc::cadd(surface, motion::areaLighting(S, M, m, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    reflected = orc::cmul(colorAt(S, M, K, T, orc::Ray{comps.over_point, comps.reflectv}, remaining - 1, J), m.reflective);
  }
  {  // world.zig:171-189
    const double n_ratio = comps.n1 / comps.n2;
    const double cos_i = orc::dot(comps.eyev, comps.normal);
    const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
    if (!(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0) {
      const double cos_t = std::sqrt(1.0 - sin2_t);
      const orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
      orc::counters().secondary++;
      refracted = orc::cmul(colorAt(S, M, K, T, orc::Ray{comps.under_point, direction}, remaining - 1, J), m.transparency);
    }
  }
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const Table& T, const orc::Ray& ray,
                   size_t remaining, const area::Jitter& J) {
  const orc::Intersections xs = motion::intersect(S, M, ray);
  const long h = orc::hit(xs);
  if (h >= 0) return shadeHit(S, M, K, T, precompute(M, T, xs[h], ray, xs), remaining, J);
  return {0.0, 0.0, 0.0};
}

// spot::render's pixel loop with bump::colorAt
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const Table& T, uint32_t x0,
           uint32_t y0, uint32_t w, uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
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
              sum = orc::cadd(sum, colorAt(S, M, cones, T, motion::passRay(camera, smp, x, y, k, g), max_depth, J));
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

}  // namespace bump

extern "C" {

// The bump table of a description: one row per material (rtc_bump; NULL: every kind none), and which row each leaf has.
// The description is read here only; the table does not keep it.
int bump_table_create(const rtc_scene_desc* desc, const rtc_bump* b, void** out) {
  try {
    auto t = std::make_unique<bump::Table>();
    t->rows.resize(desc->n_materials);
    if (b) {
      if (b->n_materials != desc->n_materials) throw std::runtime_error("InvalidArgument: n_materials");
      for (uint32_t i = 0; i < b->n_materials; ++i) {
        bump::Row& R = t->rows[i];
        if (b->kind[i] > RTC_BUMP_RIPPLES) throw std::runtime_error("InvalidArgument: kind");
        R.kind = b->kind[i];
        if (R.kind == RTC_BUMP_NONE) continue;
        R.amplitude = b->amplitude[i];
        if (R.kind == RTC_BUMP_NOISE) {
          R.octaves = b->octaves[i];
          R.persistence = b->persistence[i];
        }
        if (b->inverse) std::memcpy(R.inv, b->inverse + 12ull * i, sizeof R.inv);
      }
    }
    for (uint32_t l = 0; l < desc->n_leaves; ++l) t->mat_of[desc->leaf_id[l]] = desc->leaf_material[l];
    *out = t.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void bump_table_destroy(void* t) { delete static_cast<bump::Table*>(t); }

// The scene: area_scene_create / area_scene_destroy of the included checkers; every other argument as spot_render's, and
// the bump table.  rgb_out [h][w][3]; counters_out [primary, secondary, shadow calls].
int bump_render(void* scene, void* table, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
                uint32_t pass, const double* disp, uint32_t n_roots, const uint8_t* cone, const double* axis, const double* cos_inner,
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
  return bump::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(table), x0, y0, w, h,
                      n_threads, rgb_out, counters_out);
}

// ---- KAT hooks
// d = field(kind, q)
void bump_kat_field(uint32_t kind, const double* q, uint32_t octaves, double persistence, double* d) {
  bump::field(kind, q, octaves, persistence, d);
}
// The three octaveNoise calls of the oracle at q, q + (0, 0, 1), q + (0, 0, 2): what the noise field must equal
void bump_kat_octave_noise(const double* q, uint32_t octaves, double persistence, double* out) {
  out[0] = orc::octaveNoise(q[0], q[1], q[2], octaves, persistence);
  out[1] = orc::octaveNoise(q[0], q[1], q[2] + 1.0, octaves, persistence);
  out[2] = orc::octaveNoise(q[0], q[1], q[2] + 2.0, octaves, persistence);
}
// ns of (ln, lp, row) on a shape whose inverse-transpose is inv_t (4 x 4, row-major; NULL: the identity), outward (`inside`
// 0) or negated (1); ng is normalToWorld(ln), negated likewise.
void bump_kat_normal(const double* ln, const double* lp, const double* inv_t, uint32_t inside, uint32_t kind, double amplitude,
                     uint32_t octaves, double persistence, const double* inverse, double* ns) {
  orc::Shape s = orc::Shape::make(orc::SPHERE);
  if (inv_t) std::memcpy(s.inverse_transpose.d, inv_t, sizeof s.inverse_transpose.d);
  bump::Row R;
  R.kind = static_cast<uint8_t>(kind);
  R.amplitude = amplitude;
  R.octaves = octaves;
  R.persistence = persistence;
  if (inverse) std::memcpy(R.inv, inverse, sizeof R.inv);
  orc::Tuple ng = s.normalToWorld(orc::vec3(ln[0], ln[1], ln[2]));
  if (inside) ng = orc::negate(ng);
  const orc::Tuple n = bump::shadingNormal(&s, orc::vec3(ln[0], ln[1], ln[2]), orc::point(lp[0], lp[1], lp[2]), ng, inside != 0, R);
  ns[0] = n.x;
  ns[1] = n.y;
  ns[2] = n.z;
}
// PreComputations of the first hit of a ray (static scene, shutter time 0): out = [hit (0 / 1), inside, over_point xyz,
// under_point xyz, normal xyz (ns), n1, n2, reflectv xyz] (16 doubles)
int bump_kat_comps(void* scene, void* table, const double* origin, const double* direction, double* out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  try {
    const std::vector<double> zero(3 * S.os->world.objects.size(), 0.0);
    const motion::Motion M = motion::make(S, zero.data(), static_cast<uint32_t>(S.os->world.objects.size()));
    const orc::Ray ray{orc::point(origin[0], origin[1], origin[2]), orc::vec3(direction[0], direction[1], direction[2])};
    const orc::Intersections xs = motion::intersect(S, M, ray);
    const long h = orc::hit(xs);
    for (int i = 0; i < 16; ++i) out[i] = 0.0;
    if (h >= 0) {
      const orc::PreComputations c = bump::precompute(M, *static_cast<bump::Table*>(table), xs[h], ray, xs);
      const double v[16] = {1.0, c.inside ? 1.0 : 0.0, c.over_point.x, c.over_point.y, c.over_point.z, c.under_point.x, c.under_point.y,
                            c.under_point.z, c.normal.x, c.normal.y, c.normal.z, c.n1, c.n2, c.reflectv.x, c.reflectv.y, c.reflectv.z};
      std::memcpy(out, v, sizeof v);
    }
    orc::Arena::mine().reset();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // extern "C"
