// motion_oracle.cpp — CPU checker of motion blur (libmotion_oracle.so).  TEST INFRASTRUCTURE.
//
// Motion blur (include/rtc.h rtc_scene_set_motion) on top of the sample-pass and camera-sampling
// checkers: their scene build, sample rays, hash and Jitter are used as they are (camera_oracle.cpp is included,
// read-only, and with it the area-light checker and the oracle's sources; the pass ray and the area key are restated as
// progressive_oracle.cpp has them, which is a library of its own).  What is restated here is only what motion changes:
//   - World.intersect as a loop over the roots, root r tested with the ray's origin shifted by -t * D_r, then the
//     reference's stable sort;
//   - PreComputations.new with the normal taken at p - t * D_r (over_point, under_point, reflectv from that normal);
//   - the pattern's object point, over_point - t * D_r;
//   - isShadowed, every root shifted;
//   - the time of a sample: the camera hash on axis 255 at the global sample index.
// Everything else - shadeHit, colorAt, reflectedColor, refractedColor, lighting of both light kinds - is the included
// checkers' code with those calls swapped in.  Nothing of the product is included or linked.
#include "camera_oracle.cpp"

#include <unordered_map>

namespace motion {

constexpr uint64_t kTimeAxis = 255;

struct Motion {
  std::vector<orc::Tuple> disp;                            // per World.objects entry
  std::unordered_map<const orc::Shape*, uint32_t> root_of;  // every shape below a root -> the root
  double t = 0.0;                                          // the shutter time of the sample being traced
};

void collect(const orc::Shape& s, uint32_t root, Motion& M) {
  M.root_of[&s] = root;
  for (const orc::Shape& c : s.children) collect(c, root, M);
}

Motion make(const area::Scene& S, const double* disp, uint32_t n_roots) {
  const auto& objects = S.os->world.objects;
  if (n_roots != objects.size()) throw std::runtime_error("InvalidArgument: n_roots");
  Motion M;
  for (uint32_t r = 0; r < n_roots; ++r) {
    M.disp.push_back(orc::vec3(disp[3 * r], disp[3 * r + 1], disp[3 * r + 2]));
    collect(objects[r], r, M);
  }
  return M;
}

// p - t * D, component by component (a point)
orc::Tuple shift(orc::Tuple p, double t, orc::Tuple D) { return orc::point(p.x - t * D.x, p.y - t * D.y, p.z - t * D.z); }

orc::Tuple dispOf(const Motion& M, const orc::Shape* s) {
  const auto it = M.root_of.find(s);
  if (it == M.root_of.end()) throw std::runtime_error("motion checker: a hit outside every root");
  return M.disp[it->second];
}

// World.intersect (world.zig:71-83), root r tested with its own ray
orc::Intersections intersect(const area::Scene& S, const Motion& M, const orc::Ray& ray) {
  orc::Intersections all;
  const auto& objects = S.os->world.objects;
  for (size_t r = 0; r < objects.size(); ++r) {
    const orc::Ray rr{shift(ray.origin, M.t, M.disp[r]), ray.direction};
    const orc::Intersections xs = objects[r].intersect(rr);
    all.insert(all.end(), xs.begin(), xs.end());
  }
  orc::sortIntersections(all);
  return all;
}

// isShadowed (world.zig:126-154) towards one point, every root shifted
bool isShadowed(const area::Scene& S, const Motion& M, orc::Tuple pt, orc::Tuple light_pos) {
  orc::counters().shadow++;
  const orc::Tuple direction = orc::sub(light_pos, pt);
  const double distance = orc::magnitude(direction);
  const orc::Ray shadow_ray{pt, orc::normalized(direction)};
  const orc::Intersections xs = intersect(S, M, shadow_ray);
  long i = orc::hit(xs);
  while (i >= 0) {
    if (xs[i].t < distance && xs[i].object->casts_shadow) return true;
    i = orc::hit(xs, static_cast<size_t>(i) + 1);
  }
  return false;
}

// PreComputations.new (world.zig:212-270) with the normal at p - t * D of the hit's root
orc::PreComputations precompute(const Motion& M, const orc::Intersection& h, const orc::Ray& ray, const orc::Intersections& xs) {
  orc::PreComputations c = orc::PreComputations::make(h, ray, xs);  // (n1 / n2 do not depend on the normal)
  const double epsilon = 1e-5;
  orc::Tuple normal = h.object->normalAt(shift(c.point, M.t, dispOf(M, h.object)), h);
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
  return c;
}

// the pattern's colour at over_point - t * D (pattern.zig:128-131)
orc::Color colorAtPoint(const Motion& M, const orc::Shape* obj, orc::Tuple pt) {
  return obj->material.pattern.patternAt(obj->worldToObject(shift(pt, M.t, dispOf(M, obj))));
}

// Material.lighting (material.zig:40-74) with the colour given
orc::Color pointLighting(const orc::Material& m, orc::Color color, const area::Light& L, orc::Tuple pt, orc::Tuple eyev, orc::Tuple normal,
                         bool in_shadow) {
  const orc::Color effective_color = orc::cemul(color, L.intensity);
  const orc::Tuple point_to_light = orc::normalized(orc::sub(L.corner, pt));
  const orc::Color ambient_ = orc::cmul(effective_color, m.ambient);
  if (in_shadow) return ambient_;
  orc::Color diffuse_{0.0, 0.0, 0.0}, specular_{0.0, 0.0, 0.0};
  const double light_dot_normal = orc::dot(point_to_light, normal);
  if (light_dot_normal >= 0.0) {
    diffuse_ = orc::cmul(effective_color, m.diffuse * light_dot_normal);
    const double reflect_dot_eye = orc::dot(orc::negate(orc::reflect(point_to_light, normal)), eyev);
    if (reflect_dot_eye > 0.0) specular_ = orc::cmul(L.intensity, m.specular * orc::zig_pow(reflect_dot_eye, m.shininess));
  }
  return orc::cadd(orc::cadd(ambient_, diffuse_), specular_);
}

// area::intensityAt / areaLighting with the moving isShadowed
double intensityAt(const area::Scene& S, const Motion& M, const area::Light& L, uint32_t l, orc::Tuple pt, const area::Jitter& J) {
  uint32_t lit = 0;
  for (uint32_t v = 0; v < L.vsteps; ++v)
    for (uint32_t u = 0; u < L.usteps; ++u) {
      const uint32_t k = v * L.usteps + u;
      const double ju = J.at(L, l, k, 0), jv = J.at(L, l, k, 1);
      if (!isShadowed(S, M, pt, area::pointOnLight(L, u, v, ju, jv))) ++lit;
    }
  return static_cast<double>(lit) / static_cast<double>(L.samples());
}

orc::Color areaLighting(const area::Scene& S, const Motion& M, const orc::Material& m, orc::Color color, const area::Light& L, uint32_t l,
                        orc::Tuple pt, orc::Tuple eyev, orc::Tuple normal, const area::Jitter& J) {
  const orc::Color effective = orc::cemul(color, L.intensity);
  const orc::Color ambient = orc::cmul(effective, m.ambient);
  const orc::Color sum = area::areaSum(m, effective, L, l, pt, eyev, normal, J);
  if (sum.r == 0.0 && sum.g == 0.0 && sum.b == 0.0) {
    orc::counters().shadow += L.samples();
    return ambient;
  }
  const double n = static_cast<double>(L.samples());
  const double inten = intensityAt(S, M, L, l, pt, J);
  return {ambient.r + (sum.r / n) * inten, ambient.g + (sum.g / n) * inten, ambient.b + (sum.b / n) * inten};
}

orc::Color colorAt(const area::Scene& S, const Motion& M, const orc::Ray& ray, size_t remaining, const area::Jitter& J);

orc::Color shadeHit(const area::Scene& S, const Motion& M, const orc::PreComputations& comps, size_t remaining, const area::Jitter& J) {
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  for (uint32_t l = 0; l < S.lights.size(); ++l) {
    const area::Light& L = S.lights[l];
    const orc::Color color = colorAtPoint(M, obj, comps.over_point);
    if (!L.is_area) {
      const bool shadowed = isShadowed(S, M, comps.over_point, L.corner);
      surface = orc::cadd(surface, pointLighting(m, color, L, comps.over_point, comps.eyev, comps.normal, shadowed));
    } else {
      surface = orc::cadd(surface, areaLighting(S, M, m, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  orc::Color reflected{0.0, 0.0, 0.0}, refracted{0.0, 0.0, 0.0};
  if (remaining != 0 && m.reflective != 0.0) {  // world.zig:157-167
    orc::counters().secondary++;
    reflected = orc::cmul(colorAt(S, M, orc::Ray{comps.over_point, comps.reflectv}, remaining - 1, J), m.reflective);
  }
  {  // world.zig:171-189
    const double n_ratio = comps.n1 / comps.n2;
    const double cos_i = orc::dot(comps.eyev, comps.normal);
    const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
    if (!(sin2_t > 1.0) && remaining != 0 && m.transparency != 0.0) {
      const double cos_t = std::sqrt(1.0 - sin2_t);
      const orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
      orc::counters().secondary++;
      refracted = orc::cmul(colorAt(S, M, orc::Ray{comps.under_point, direction}, remaining - 1, J), m.transparency);
    }
  }
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const area::Scene& S, const Motion& M, const orc::Ray& ray, size_t remaining, const area::Jitter& J) {
  const orc::Intersections xs = intersect(S, M, ray);
  const long h = orc::hit(xs);
  if (h >= 0) return shadeHit(S, M, precompute(M, xs[h], ray, xs), remaining, J);
  return {0.0, 0.0, 0.0};
}

// the time of sample g (global index) of the whole-image pixel p
double time(uint64_t seed, uint64_t p, uint64_t g) { return camsmp::hash(seed, p, g, kTimeAxis); }

// progressive_oracle.cpp's pass ray and area key (that checker is a library of its own: restated, not included)
orc::Ray passRay(const orc::Camera& c, const camsmp::Sampling& s, size_t x, size_t y, uint32_t k, uint64_t g) {
  const uint32_t j = k / s.grid, i = k % s.grid;
  const uint64_t p = static_cast<uint64_t>(y) * c.hsize + x;
  const double jx = s.jitter ? camsmp::hash(s.seed, p, g, 0) : 0.5;
  const double jy = s.jitter ? camsmp::hash(s.seed, p, g, 1) : 0.5;
  const double n = static_cast<double>(s.grid);
  const double ox = (static_cast<double>(i) + jx) / n;
  const double oy = (static_cast<double>(j) + jy) / n;
  const double xoffset = (static_cast<double>(x) + ox) * c.pixel_size;
  const double yoffset = (static_cast<double>(y) + oy) * c.pixel_size;
  const double world_x = c.half_width - xoffset;
  const double world_y = c.half_height - yoffset;
  if (s.aperture == 0.0) {
    const orc::Tuple pixel = c.inverse.tupleMul(orc::point(world_x, world_y, -1.0));
    const orc::Tuple origin = c.inverse.tupleMul(orc::point(0.0, 0.0, 0.0));
    return {origin, orc::normalized(orc::sub(pixel, origin))};
  }
  double lx = 0.0, ly = 0.0;
  for (uint32_t t = 0; t < 32; ++t) {
    const double a = 2.0 * camsmp::hash(s.seed, p, g, 2 + 2 * t) - 1.0;
    const double b = 2.0 * camsmp::hash(s.seed, p, g, 3 + 2 * t) - 1.0;
    if ((a * a) + (b * b) <= 1.0) {
      lx = a;
      ly = b;
      break;
    }
  }
  const double f = s.focal;
  const orc::Tuple origin = c.inverse.tupleMul(orc::point(s.aperture * lx, s.aperture * ly, 0.0));
  const orc::Tuple pixel = c.inverse.tupleMul(orc::point(world_x * f, world_y * f, -f));
  return {origin, orc::normalized(orc::sub(pixel, origin))};
}

// One threaded pixel loop.  fixed_t >= 0: every sample at that time (the KATs), else the hash's.
int render(const area::Scene& S, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
           uint32_t pass, const double* disp, uint32_t n_roots, double fixed_t, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
           uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const orc::Camera camera = cameraFrom(*cam);
  try {
    const Motion base = make(S, disp, n_roots);
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
      Motion M = base;
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
              M.t = fixed_t >= 0.0 ? fixed_t : time(smp.seed, p, g);
              sum = orc::cadd(sum, colorAt(S, M, passRay(camera, smp, x, y, k, g), max_depth, J));
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

}  // namespace motion

extern "C" {

// The scene: area_scene_create / area_scene_destroy of the included checker; disp [n_roots][3] in World.objects order.
// rgb_out [h][w][3] of the rectangle [x0, x0 + w) x [y0, y0 + h); counters_out [primary, secondary, shadow calls]
int motion_render(void* scene, const rtc_camera* cam, uint32_t max_depth, uint64_t light_seed, const rtc_sampling* sampling,
                  uint32_t pass, const double* disp, uint32_t n_roots, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                  uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  return motion::render(*static_cast<area::Scene*>(scene), cam, max_depth, light_seed, sampling, pass, disp, n_roots, -1.0, x0, y0,
                        w, h, n_threads, rgb_out, counters_out);
}

// ---- KAT hooks: one centred sample per pixel (no sampling, pass 0) with every sample at time t; the time hash
int motion_kat_render_at(void* scene, const rtc_camera* cam, uint32_t max_depth, const double* disp, uint32_t n_roots, double t,
                         uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, double* rgb_out) {
  if (!(t >= 0.0 && t < 1.0)) {
    g_error = "InvalidArgument: t";
    return 1;
  }
  return motion::render(*static_cast<area::Scene*>(scene), cam, max_depth, 0, nullptr, 0, disp, n_roots, t, x0, y0, w, h, 0, rgb_out,
                        nullptr);
}

void motion_kat_time(uint64_t seed, const uint64_t* p, const uint64_t* g, uint64_t n, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = motion::time(seed, p[i], g[i]);
}

}  // extern "C"
