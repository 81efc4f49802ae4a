// torus_oracle.cpp — CPU checker of torus primitives (libtorus_oracle.so).  TEST INFRASTRUCTURE.
//
// The torus (include/rtc.h RTC_TORUS) on top of the normal-perturbation checker: bump_oracle.cpp is
// included, read-only, and with it the spot, motion, camera-sampling and area-light checkers and the oracle's sources.
// The oracle's Shape is a closed switch without a torus, so the checker receives its scene with every torus replaced by a
// placeholder leaf - a sphere with the torus's transform, material, shadow flag, Shape.id and place in the tree - and a
// side table Shape.id -> (R, r).  What is restated here is what a new leaf kind changes:
//   - the torus's localIntersect (steps 1 to 5 of rtc.h, operation for operation) and localNormalAt;
//   - Shape.intersect for a leaf, a group (box test, children, stable sort) and a csg (csgFilter reused), with the torus's
//     entries in place of the placeholder's; through it World.intersect (the motion checker's loop over shifted roots)
//     and isShadowed;
//   - PreComputations' normal step (motion's geometric normal, bump's shading normal) with the torus's normal;
//   - through them the area intensity, shadeHit, colorAt and the pass loop, as bump_oracle.cpp has them.
// Patterns, the cone's factor, lighting and the sample rays are the included checkers'.  Nothing of the product is
// included or linked.
#include "bump_oracle.cpp"

namespace torus {

struct Radii {
  double R, r;
};
struct Table {
  std::unordered_map<size_t, Radii> of;  // a placeholder's Shape.id -> its torus's radii
};
const Radii* radiiOf(const Table& Q, const orc::Shape* s) {
  const auto it = Q.of.find(s->id);
  return it == Q.of.end() ? nullptr : &it->second;
}

struct Coeffs {
  double t0, c4, c3, c2, c1, c0;
};
// steps 1 and 3
Coeffs coefficients(const double o[3], const double d[3], double R, double r) {
  Coeffs k;
  const double alpha = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  k.t0 = -((o[0] * d[0] + o[1] * d[1]) + o[2] * d[2]) / alpha;
  const double px = o[0] + k.t0 * d[0], py = o[1] + k.t0 * d[1], pz = o[2] + k.t0 * d[2];
  const double beta = 2.0 * ((px * d[0] + py * d[1]) + pz * d[2]);
  const double gamma = (((px * px + py * py) + pz * pz) + R * R) - r * r;
  const double f = 4.0 * (R * R);
  k.c4 = alpha * alpha;
  k.c3 = (2.0 * alpha) * beta;
  k.c2 = (beta * beta + (2.0 * alpha) * gamma) - f * (d[0] * d[0] + d[2] * d[2]);
  k.c1 = (2.0 * beta) * gamma - (2.0 * f) * (px * d[0] + pz * d[2]);
  k.c0 = gamma * gamma - f * (px * px + pz * pz);
  return k;
}

struct Poly {
  double a4, a3, a2, a1, a0;
  double P(double x) const { return (((a4 * x + a3) * x + a2) * x + a1) * x + a0; }
  double D(double x) const { return (((4.0 * a4) * x + 3.0 * a3) * x + 2.0 * a2) * x + a1; }
};
struct Roots {
  double s[4];
  uint32_t n = 0;
  void emit(uint32_t cap, double x) {
    if (n >= cap || (n != 0 && !(x > s[n - 1]))) return;
    s[n++] = x;
  }
};
double refine(const Poly& p, double l, double h, double fa) {
  double x = 0.5 * (l + h);
  for (int it = 0; it < 80; ++it) {
    const double fx = p.P(x);
    if (fx == 0.0) break;
    if ((fx < 0.0) == (fa < 0.0)) l = x;
    else h = x;
    const double d = p.D(x);
    double xn = d != 0.0 ? x - fx / d : l;
    if (!(xn > l && xn < h)) xn = 0.5 * (l + h);
    const double m = 0.5 * (l + h);
    const bool stop = xn == x || !(l < h) || m == l || m == h;
    x = xn;
    if (stop) break;
  }
  return x;
}
Roots scan(const Poly& p, const Roots& points, uint32_t cap, double lo, double hi) {
  Roots out;
  double a = lo, fa = p.P(lo);
  for (uint32_t i = 0; i <= points.n; ++i) {
    const double b = i == points.n ? hi : points.s[i];
    if (i < points.n && !(b > a && b < hi)) continue;
    const double fb = p.P(b);
    if (fa == 0.0) out.emit(cap, a);
    else if ((fa < 0.0) != (fb < 0.0) && fb != 0.0) out.emit(cap, refine(p, a, b, fa));
    a = b;
    fa = fb;
  }
  if (fa == 0.0) out.emit(cap, a);
  return out;
}
// step 4: the roots of c4 s^4 + ... + c0 in [lo, hi], ascending
Roots quartic(double c4, double c3, double c2, double c1, double c0, double lo, double hi) {
  Roots none;
  if (!(lo < hi) || !(hi - lo < orc::INF)) return none;
  const Poly dq{0.0, 4.0 * c4, 3.0 * c3, 2.0 * c2, c1};
  Roots crit;
  const double q0 = 3.0 * dq.a3, q1 = 2.0 * dq.a2, q2 = dq.a1;
  const double disc = q1 * q1 - (4.0 * q0) * q2;
  if (disc >= 0.0) {
    const double sq = std::sqrt(disc);
    const double k0 = (-q1 - sq) / (2.0 * q0), k1 = (-q1 + sq) / (2.0 * q0);
    crit.s[0] = k1 < k0 ? k1 : k0;
    crit.s[1] = k1 < k0 ? k0 : k1;
    crit.n = 2;
  }
  const Roots turning = scan(dq, crit, 3, lo, hi);
  return scan(Poly{c4, c3, c2, c1, c0}, turning, 4, lo, hi);
}
// steps 1 to 5: the entries' t of the ray (o, d) in the torus's object space
Roots roots(const double o[3], const double d[3], double R, double r) {
  Roots none;
  const Coeffs k = coefficients(o, d, R, r);
  const double bxz = (R + r) * (1.0 + 1e-9), by = r * (1.0 + 1e-9);
  orc::Intersections box;
  slabIntersect(orc::point(-bxz, -by, -bxz), orc::point(bxz, by, bxz), orc::Ray{orc::point(o[0], o[1], o[2]), orc::vec3(d[0], d[1], d[2])},
                nullptr, box);
  if (box.empty()) return none;
  Roots s = quartic(k.c4, k.c3, k.c2, k.c1, k.c0, box[0].t - k.t0, box[1].t - k.t0);
  for (uint32_t i = 0; i < s.n; ++i) s.s[i] = k.t0 + s.s[i];
  return s;
}
orc::Tuple localNormal(orc::Tuple p, double R) {
  const double rho = std::sqrt(p.x * p.x + p.z * p.z);
  if (rho == 0.0) return orc::vec3(0.0, p.y, 0.0);
  return orc::vec3(p.x - R * (p.x / rho), p.y, p.z - R * (p.z / rho));
}

// Shape.intersect (shape.zig:313-335) with Group.localIntersect (group.zig:39-62) and Csg.localIntersect (csg.zig:74-95)
orc::Intersections intersectShape(const Table& Q, const orc::Shape& s, const orc::Ray& ray) {
  if (s.kind == orc::GROUP || s.kind == orc::CSG) {
    orc::Intersections xs;
    static const orc::Matrix kIdentity = orc::Matrix::identity();
    orc::counters().bbox_tests++;
    orc::Intersections bbox_xs;
    orc::slabIntersect(s.bmin, s.bmax, ray.transform(kIdentity), &s, bbox_xs);
    if (bbox_xs.empty()) return xs;
    if (s.kind == orc::GROUP) {
      for (const orc::Shape& child : s.children) {
        const orc::Intersections cx = intersectShape(Q, child, ray);
        xs.insert(xs.end(), cx.begin(), cx.end());
      }
      orc::sortIntersections(xs);
      return xs;
    }
    xs = intersectShape(Q, s.children[0], ray);
    const orc::Intersections rightxs = intersectShape(Q, s.children[1], ray);
    xs.insert(xs.end(), rightxs.begin(), rightxs.end());
    orc::sortIntersections(xs);
    return orc::csgFilter(s, xs);
  }
  const Radii* q = radiiOf(Q, &s);
  if (!q) return s.intersect(ray);
  orc::counters().leaf_tests++;
  orc::counters().xforms++;
  const orc::Ray lr = ray.transform(s.inverse);
  const double o[3] = {lr.origin.x, lr.origin.y, lr.origin.z}, d[3] = {lr.direction.x, lr.direction.y, lr.direction.z};
  const Roots k = roots(o, d, q->R, q->r);
  orc::Intersections xs;
  for (uint32_t i = 0; i < k.n; ++i) xs.push_back({k.s[i], &s});
  return xs;
}

// Shape.normalAt (shape.zig:338-350)
orc::Tuple normalAt(const Table& Q, const orc::Shape* s, orc::Tuple p, const orc::Intersection& h) {
  const Radii* q = radiiOf(Q, s);
  if (!q) return s->normalAt(p, h);
  return s->normalToWorld(localNormal(s->worldToObject(p), q->R));
}

// motion::intersect with intersectShape
orc::Intersections intersect(const area::Scene& S, const motion::Motion& M, const Table& Q, const orc::Ray& ray) {
  orc::Intersections all;
  const auto& objects = S.os->world.objects;
  for (size_t r = 0; r < objects.size(); ++r) {
    const orc::Ray rr{motion::shift(ray.origin, M.t, M.disp[r]), ray.direction};
    const orc::Intersections xs = intersectShape(Q, objects[r], rr);
    all.insert(all.end(), xs.begin(), xs.end());
  }
  orc::sortIntersections(all);
  return all;
}

// motion::isShadowed with torus::intersect
bool isShadowed(const area::Scene& S, const motion::Motion& M, const Table& Q, orc::Tuple pt, orc::Tuple light_pos) {
  orc::counters().shadow++;
  const orc::Tuple direction = orc::sub(light_pos, pt);
  const double distance = orc::magnitude(direction);
  const orc::Ray shadow_ray{pt, orc::normalized(direction)};
  const orc::Intersections xs = intersect(S, M, Q, shadow_ray);
  long i = orc::hit(xs);
  while (i >= 0) {
    if (xs[i].t < distance && xs[i].object->casts_shadow) return true;
    i = orc::hit(xs, static_cast<size_t>(i) + 1);
  }
  return false;
}

// motion::precompute, then bump::precompute, with the torus's normal (n1 / n2 do not depend on the normal; the
// placeholder's own normal, which PreComputations.make computes first, is replaced)
orc::PreComputations precompute(const motion::Motion& M, const bump::Table& T, const Table& Q, const orc::Intersection& h,
                                const orc::Ray& ray, const orc::Intersections& xs) {
  orc::PreComputations c = orc::PreComputations::make(h, ray, xs);
  const double epsilon = 1e-5;
  const orc::Tuple sp = motion::shift(c.point, M.t, motion::dispOf(M, h.object));
  orc::Tuple normal = normalAt(Q, h.object, sp, h);
  bool inside = false;
  if (orc::dot(normal, c.eyev) < 0) {
    normal = orc::negate(normal);
    inside = true;
  }
  c.normal = normal;
  c.inside = inside;
  c.over_point = orc::add(c.point, orc::mul(normal, epsilon));
  c.under_point = orc::sub(c.point, orc::mul(normal, epsilon));
  c.reflectv = orc::reflect(ray.direction, normal);
  const bump::Row& R = bump::rowOf(T, h.object);
  if (R.kind == RTC_BUMP_NONE || R.amplitude == 0.0) return c;
  const orc::Tuple lp = h.object->worldToObject(sp);
  const Radii* q = radiiOf(Q, h.object);
  const orc::Tuple ln = q ? localNormal(lp, q->R) : h.object->localNormalAt(lp, h);
  c.normal = bump::shadingNormal(h.object, ln, lp, c.normal, c.inside, R);
  c.reflectv = orc::reflect(ray.direction, c.normal);
  return c;
}

// motion::intensityAt / areaLighting with torus::isShadowed
double intensityAt(const area::Scene& S, const motion::Motion& M, const Table& Q, const area::Light& L, uint32_t l, orc::Tuple pt,
                   const area::Jitter& J) {
  uint32_t lit = 0;
  for (uint32_t v = 0; v < L.vsteps; ++v)
    for (uint32_t u = 0; u < L.usteps; ++u) {
      const uint32_t k = v * L.usteps + u;
      const double ju = J.at(L, l, k, 0), jv = J.at(L, l, k, 1);
      if (!isShadowed(S, M, Q, pt, area::pointOnLight(L, u, v, ju, jv))) ++lit;
    }
  return static_cast<double>(lit) / static_cast<double>(L.samples());
}
orc::Color areaLighting(const area::Scene& S, const motion::Motion& M, const Table& Q, const orc::Material& m, orc::Color color,
                        const area::Light& L, uint32_t l, orc::Tuple pt, orc::Tuple eyev, orc::Tuple normal, const area::Jitter& J) {
  const orc::Color effective = orc::cemul(color, L.intensity);
  const orc::Color ambient = orc::cmul(effective, m.ambient);
  const orc::Color sum = area::areaSum(m, effective, L, l, pt, eyev, normal, J);
  if (sum.r == 0.0 && sum.g == 0.0 && sum.b == 0.0) {
    orc::counters().shadow += L.samples();
    return ambient;
  }
  const double n = static_cast<double>(L.samples());
  const double inten = intensityAt(S, M, Q, L, l, pt, J);
  return {ambient.r + (sum.r / n) * inten, ambient.g + (sum.g / n) * inten, ambient.b + (sum.b / n) * inten};
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T, const Table& Q,
                   const orc::Ray& ray, size_t remaining, const area::Jitter& J);

// bump::shadeHit with torus::isShadowed, areaLighting and colorAt
orc::Color shadeHit(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T, const Table& Q,
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
      const bool shadowed = isShadowed(S, M, Q, comps.over_point, L.corner);
      surface = orc::cadd(surface, spot::spotLighting(m, color, L, point_to_light, comps.eyev, comps.normal, shadowed, f));
    } else {
      surface = orc::cadd(surface, areaLighting(S, M, Q, m, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    reflected = orc::cmul(colorAt(S, M, K, T, Q, orc::Ray{comps.over_point, comps.reflectv}, remaining - 1, J), m.reflective);
  }
  {  // world.zig:171-189
    const double n_ratio = comps.n1 / comps.n2;
    const double cos_i = orc::dot(comps.eyev, comps.normal);
    const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
    if (!(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0) {
      const double cos_t = std::sqrt(1.0 - sin2_t);
      const orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
      orc::counters().secondary++;
      refracted = orc::cmul(colorAt(S, M, K, T, Q, orc::Ray{comps.under_point, direction}, remaining - 1, J), m.transparency);
    }
  }
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const area::Scene& S, const motion::Motion& M, const std::vector<spot::Cone>& K, const bump::Table& T, const Table& Q,
                   const orc::Ray& ray, size_t remaining, const area::Jitter& J) {
  const orc::Intersections xs = intersect(S, M, Q, ray);
  const long h = orc::hit(xs);
  if (h >= 0) return shadeHit(S, M, K, T, Q, precompute(M, T, Q, xs[h], ray, xs), remaining, J);
  return {0.0, 0.0, 0.0};
}

// bump::render's pixel loop with torus::colorAt
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, const std::vector<spot::Cone>& cones, const bump::Table& T, const Table& Q, uint32_t x0,
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
              sum = orc::cadd(sum, colorAt(S, M, cones, T, Q, motion::passRay(camera, smp, x, y, k, g), max_depth, J));
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

}  // namespace torus

extern "C" {

// The side table: n placeholders, ids[i] the Shape.id (leaf_id) of the leaf that stands for a torus of radii
// (major[i], minor[i]).  n == 0: a scene without a torus.
int torus_table_create(const size_t* ids, const double* major, const double* minor, uint32_t n, void** out) {
  try {
    auto t = std::make_unique<torus::Table>();
    for (uint32_t i = 0; i < n; ++i) {
      if (!(0.0 < minor[i] && minor[i] < major[i])) throw std::runtime_error("InvalidArgument: torus radii");
      t->of[ids[i]] = torus::Radii{major[i], minor[i]};
    }
    *out = t.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void torus_table_destroy(void* t) { delete static_cast<torus::Table*>(t); }

// The scene (with placeholders): area_scene_create / area_scene_destroy of the included checkers; the bump table:
// bump_table_create; every other argument as bump_render's, and the side table.
int torus_render(void* scene, void* bumps, void* tori, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed,
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
  return torus::render(S, cam, max_depth, light_seed, sampling, pass, disp, n_roots, cones, *static_cast<bump::Table*>(bumps),
                       *static_cast<torus::Table*>(tori), x0, y0, w, h, n_threads, rgb_out, counters_out);
}

// ---- KAT hooks
// out = [t0, c4, c3, c2, c1, c0] of the ray (o, d) against the torus (R, r)
void torus_kat_coefficients(const double* o, const double* d, double R, double r, double* out) {
  const torus::Coeffs k = torus::coefficients(o, d, R, r);
  const double v[6] = {k.t0, k.c4, k.c3, k.c2, k.c1, k.c0};
  std::memcpy(out, v, sizeof v);
}
// the entries' t, ascending, into t_out[4]; returns their number
uint32_t torus_kat_roots(const double* o, const double* d, double R, double r, double* t_out) {
  const torus::Roots k = torus::roots(o, d, R, r);
  for (uint32_t i = 0; i < k.n; ++i) t_out[i] = k.s[i];
  orc::Arena::mine().reset();
  return k.n;
}
// many rays at once (o, d: [n][3]; R, r: [n]): n_out[n], t_out[n][4]
void torus_kat_roots_many(const double* o, const double* d, const double* R, const double* r, uint32_t n, uint32_t* n_out, double* t_out) {
  for (uint32_t i = 0; i < n; ++i) n_out[i] = torus_kat_roots(o + 3ull * i, d + 3ull * i, R[i], r[i], t_out + 4ull * i);
}
void torus_kat_normal(const double* p, double R, double* n_out) {
  const orc::Tuple n = torus::localNormal(orc::point(p[0], p[1], p[2]), R);
  n_out[0] = n.x;
  n_out[1] = n.y;
  n_out[2] = n.z;
}
// World.intersect of a static scene (shutter time 0): up to cap entries' t and Shape.id; returns their number
int torus_kat_intersect(void* scene, void* tori, const double* origin, const double* direction, uint32_t cap, double* t_out,
                        uint64_t* id_out, uint32_t* n_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  try {
    const std::vector<double> zero(3 * S.os->world.objects.size(), 0.0);
    const motion::Motion M = motion::make(S, zero.data(), static_cast<uint32_t>(S.os->world.objects.size()));
    const orc::Ray ray{orc::point(origin[0], origin[1], origin[2]), orc::vec3(direction[0], direction[1], direction[2])};
    const orc::Intersections xs = torus::intersect(S, M, *static_cast<torus::Table*>(tori), ray);
    *n_out = static_cast<uint32_t>(xs.size());
    for (uint32_t i = 0; i < xs.size() && i < cap; ++i) {
      t_out[i] = xs[i].t;
      id_out[i] = xs[i].object->id;
    }
    orc::Arena::mine().reset();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}

}  // extern "C"
