// area_oracle.cpp — CPU checker of the area lights (libarea_oracle.so).  TEST INFRASTRUCTURE.
//
// The book's bonus chapter "Rendering soft shadows", restated on top of the CPU oracle: the oracle's own scene build
// from a description, intersections, PreComputations, patterns and zig_pow are used as they are (the two files are
// included, read-only); what is restated here are free functions that mirror World's methods with World.lights of two
// kinds - point_on_light, intensity_at and the area form of lighting, then shadeHit, colorAt, reflectedColor,
// refractedColor and the threaded pixel loop.  Nothing of the product is included or linked.
//
// Jitter (include/rtc.h) is keyed on the whole image's pixel; the KAT hooks take an explicit
// sequence instead, as the book's cyclic sequence does.
#include "../../oracle/oracle_capi.cpp"

namespace area {

struct Light {
  bool is_area = false;
  orc::Tuple corner;  // a point light's position
  orc::Tuple uvec, vvec;  // cell vectors: full edge / steps
  uint32_t usteps = 1, vsteps = 1;
  bool jitter = false;
  orc::Color intensity;
  uint32_t samples() const { return usteps * vsteps; }
};

// The jitter: a sequence of values in [0, 1), one per call.
struct Sequence {
  virtual double next() = 0;
  virtual ~Sequence() = default;
};
struct Centre : Sequence {  // no jitter
  double next() override { return 0.5; }
};
struct Cyclic : Sequence {  // the book's deterministic sequence
  std::vector<double> v;
  size_t i = 0;
  double next() override {
    const double r = v[i];
    i = (i + 1) % v.size();
    return r;
  }
};

uint64_t mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double hashJitter(uint64_t seed, uint64_t p, uint64_t n_lights, uint64_t l, uint64_t k, uint64_t axis) {
  const uint64_t c = ((p * n_lights + l) << 32) | (2 * k + axis);
  return static_cast<double>(mix(seed + 0x9E3779B97F4A7C15ull * (c + 1)) >> 11) * 0x1.0p-53;
}

// ju / jv of sample k of light l for one pixel
struct Jitter {
  Sequence* seq = nullptr;  // the KAT hooks
  uint64_t seed = 0, pixel = 0, n_lights = 0;
  double at(const Light& L, uint32_t l, uint32_t k, uint32_t axis) const {
    if (!L.jitter) return 0.5;
    if (seq) return seq->next();
    return hashJitter(seed, pixel, n_lights, l, k, axis);
  }
};

orc::Tuple pointOnLight(const Light& L, uint32_t u, uint32_t v, double ju, double jv) {
  return orc::add(orc::add(L.corner, orc::mul(L.uvec, u + ju)), orc::mul(L.vvec, v + jv));
}

// isShadowed (world.zig:126-154) towards one point: counts one shadow call
bool isShadowedFrom(const orc::World& w, orc::Tuple pt, orc::Tuple light_pos) {
  const orc::Light tmp{light_pos, {1.0, 1.0, 1.0}};
  return w.isShadowed(pt, tmp);
}

double intensityAt(const orc::World& w, const Light& L, uint32_t l, orc::Tuple pt, const Jitter& J) {
  uint32_t lit = 0;
  for (uint32_t v = 0; v < L.vsteps; ++v)
    for (uint32_t u = 0; u < L.usteps; ++u) {
      const uint32_t k = v * L.usteps + u;
      const double ju = J.at(L, l, k, 0), jv = J.at(L, l, k, 1);
      if (!isShadowedFrom(w, pt, pointOnLight(L, u, v, ju, jv))) ++lit;
    }
  return static_cast<double>(lit) / static_cast<double>(L.samples());
}

// lighting() of an area light: ambient + (sum / samples) * intensity_at.  The one exact skip: a sum of exactly zero
// (every sample behind the surface, or diffuse == specular == 0) is `ambient` whatever intensity_at says - its rays are
// counted as calls and not traced.
// the diffuse + specular terms summed over the samples, in order
orc::Color areaSum(const orc::Material& m, orc::Color effective, const Light& L, uint32_t l, orc::Tuple pt, orc::Tuple eyev,
                   orc::Tuple normal, const Jitter& J) {
  orc::Color sum{0.0, 0.0, 0.0};
  if (!(m.diffuse == 0.0 && m.specular == 0.0)) {
    Jitter J1 = J;  // (a cyclic sequence restarts for the second pass: the same samples)
    Cyclic restart;
    if (J.seq) {
      if (auto* cyc = dynamic_cast<Cyclic*>(J.seq)) {
        restart = *cyc;
        J1.seq = &restart;
      }
    }
    for (uint32_t v = 0; v < L.vsteps; ++v)
      for (uint32_t u = 0; u < L.usteps; ++u) {
        const uint32_t k = v * L.usteps + u;
        const double ju = J1.at(L, l, k, 0), jv = J1.at(L, l, k, 1);
        const orc::Tuple lightv = orc::normalized(orc::sub(pointOnLight(L, u, v, ju, jv), pt));
        const double ldn = orc::dot(lightv, normal);
        if (ldn >= 0.0) {
          sum = orc::cadd(sum, orc::cmul(effective, m.diffuse * ldn));
          const double rde = orc::dot(orc::negate(orc::reflect(lightv, normal)), eyev);
          if (rde > 0.0) sum = orc::cadd(sum, orc::cmul(L.intensity, m.specular * orc::zig_pow(rde, m.shininess)));
        }
      }
  }
  return sum;
}

orc::Color areaLighting(const orc::World& w, const orc::Material& m, orc::Color color, const Light& L, uint32_t l, orc::Tuple pt,
                        orc::Tuple eyev, orc::Tuple normal, const Jitter& J) {
  const orc::Color effective = orc::cemul(color, L.intensity);
  const orc::Color ambient = orc::cmul(effective, m.ambient);
  const orc::Color sum = areaSum(m, effective, L, l, pt, eyev, normal, J);
  if (sum.r == 0.0 && sum.g == 0.0 && sum.b == 0.0) {
    orc::counters().shadow += L.samples();
    return ambient;
  }
  const double n = static_cast<double>(L.samples());
  const double inten = intensityAt(w, L, l, pt, J);
  return {ambient.r + (sum.r / n) * inten, ambient.g + (sum.g / n) * inten, ambient.b + (sum.b / n) * inten};
}

struct Scene {
  OracleScene* os = nullptr;
  std::vector<Light> lights;
  ~Scene() { delete os; }
};

orc::Color colorAt(const Scene& S, const orc::Ray& ray, size_t remaining, const Jitter& J);

orc::Color reflectedColor(const Scene& S, const orc::PreComputations& comps, size_t remaining, const Jitter& J) {  // world.zig:157-167
  if (remaining == 0 || comps.intersection.object->material.reflective == 0.0) return {0.0, 0.0, 0.0};
  orc::counters().secondary++;
  const orc::Ray reflected{comps.over_point, comps.reflectv};
  return orc::cmul(colorAt(S, reflected, remaining - 1, J), comps.intersection.object->material.reflective);
}

orc::Color refractedColor(const Scene& S, const orc::PreComputations& comps, size_t remaining, const Jitter& J) {  // world.zig:171-189
  const double n_ratio = comps.n1 / comps.n2;
  const double cos_i = orc::dot(comps.eyev, comps.normal);
  const double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
  if (sin2_t > 1.0) return {0.0, 0.0, 0.0};
  if (remaining == 0 || comps.intersection.object->material.transparency == 0.0) return {0.0, 0.0, 0.0};
  const double cos_t = std::sqrt(1.0 - sin2_t);
  const orc::Tuple direction = orc::sub(orc::mul(comps.normal, n_ratio * cos_i - cos_t), orc::mul(comps.eyev, n_ratio));
  orc::counters().secondary++;
  const orc::Ray refracted{comps.under_point, direction};
  return orc::cmul(colorAt(S, refracted, remaining - 1, J), comps.intersection.object->material.transparency);
}

orc::Color shadeHit(const Scene& S, const orc::PreComputations& comps, size_t remaining, const Jitter& J) {  // world.zig:86-108
  const orc::World& w = S.os->world;
  orc::Color surface{0.0, 0.0, 0.0};
  const orc::Shape* obj = comps.intersection.object;
  const orc::Material& m = obj->material;
  for (uint32_t l = 0; l < S.lights.size(); ++l) {
    const Light& L = S.lights[l];
    if (!L.is_area) {  // material.zig:40-74 as the reference has it
      const orc::Light pl{L.corner, L.intensity};
      const bool shadowed = w.isShadowed(comps.over_point, pl);
      surface = orc::cadd(surface, m.lighting(pl, obj, comps.over_point, comps.eyev, comps.normal, shadowed));
    } else {
      const orc::Color color = m.pattern.patternAt(obj->worldToObject(comps.over_point));
      surface = orc::cadd(surface, areaLighting(w, m, color, L, l, comps.over_point, comps.eyev, comps.normal, J));
    }
  }
  const orc::Color reflected = reflectedColor(S, comps, remaining, J);
  const orc::Color refracted = refractedColor(S, comps, remaining, J);
  if (m.reflective > 0.0 && m.transparency > 0.0) {
    const double reflectance = comps.schlick();
    return orc::cadd(orc::cadd(surface, orc::cmul(reflected, reflectance)), orc::cmul(refracted, 1.0 - reflectance));
  }
  return orc::cadd(orc::cadd(surface, reflected), refracted);
}

orc::Color colorAt(const Scene& S, const orc::Ray& ray, size_t remaining, const Jitter& J) {  // world.zig:111-121
  const orc::Intersections xs = S.os->world.intersect(ray);
  const long h = orc::hit(xs);
  if (h >= 0) return shadeHit(S, orc::PreComputations::make(xs[h], ray, xs), remaining, J);
  return {0.0, 0.0, 0.0};
}

std::vector<Light> lightsFrom(const rtc_light_desc& d) {
  std::vector<Light> out;
  for (uint32_t i = 0; i < d.n_lights; ++i) {
    Light L;
    L.is_area = d.kind[i] == RTC_LIGHT_AREA;
    L.corner = orc::point(d.corner[3 * i], d.corner[3 * i + 1], d.corner[3 * i + 2]);
    L.intensity = {d.rgb[3 * i], d.rgb[3 * i + 1], d.rgb[3 * i + 2]};
    if (L.is_area) {
      if (d.usteps[i] == 0 || d.vsteps[i] == 0) throw std::runtime_error("InvalidArgument: steps");
      L.usteps = d.usteps[i];
      L.vsteps = d.vsteps[i];
      L.uvec = orc::div(orc::vec3(d.uvec[3 * i], d.uvec[3 * i + 1], d.uvec[3 * i + 2]), L.usteps);
      L.vvec = orc::div(orc::vec3(d.vvec[3 * i], d.vvec[3 * i + 1], d.vvec[3 * i + 2]), L.vsteps);
      L.jitter = d.jitter[i] != 0;
    }
    out.push_back(L);
  }
  return out;
}

// The book's test light: corner, full edges, steps
Light bookLight(const double* corner, const double* fu, uint32_t us, const double* fv, uint32_t vs, bool jitter) {
  Light L;
  L.is_area = true;
  L.corner = orc::point(corner[0], corner[1], corner[2]);
  L.usteps = us;
  L.vsteps = vs;
  L.uvec = orc::div(orc::vec3(fu[0], fu[1], fu[2]), us);
  L.vvec = orc::div(orc::vec3(fv[0], fv[1], fv[2]), vs);
  L.jitter = jitter;
  L.intensity = {1.0, 1.0, 1.0};
  return L;
}

}  // namespace area

extern "C" {

const char* area_last_error(void) { return g_error.c_str(); }

int area_scene_create(const rtc_scene_desc* desc, const rtc_light_desc* lights, void** out) {
  try {
    auto s = std::make_unique<area::Scene>();
    s->os = buildScene(*desc);
    s->lights = area::lightsFrom(*lights);
    *out = s.release();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 1;
  }
}
void area_scene_destroy(void* s) { delete static_cast<area::Scene*>(s); }

// rgb_out [h][w][3] of the rectangle [x0, x0 + w) x [y0, y0 + h); counters_out [primary, secondary, shadow calls]
int area_render(void* scene, const rtc_camera* cam, uint32_t max_depth, uint64_t seed, uint32_t x0, uint32_t y0, uint32_t w,
                uint32_t h, uint32_t n_threads, double* rgb_out, uint64_t* counters_out) {
  const area::Scene& S = *static_cast<area::Scene*>(scene);
  const orc::Camera camera = cameraFrom(*cam);
  try {
    if (n_threads == 0) n_threads = std::max(1u, std::thread::hardware_concurrency());
    std::atomic<uint32_t> next_row{0};
    std::vector<orc::Counters> per_thread(n_threads);
    std::string error;
    std::atomic<bool> failed{false};
    auto worker = [&](uint32_t tid) {
      orc::counters() = orc::Counters{};
      try {
        for (;;) {
          const uint32_t r = next_row.fetch_add(1);
          if (r >= h || failed.load()) break;
          const uint32_t y = y0 + r;
          for (uint32_t i = 0; i < w; ++i) {
            const uint32_t x = x0 + i;
            orc::counters().primary++;
            area::Jitter J;
            J.seed = seed;
            J.pixel = static_cast<uint64_t>(y) * cam->hsize + x;
            J.n_lights = S.lights.size();
            const orc::Color c = area::colorAt(S, camera.rayForPixel(x, y), max_depth, J);
            double* px = rgb_out + 3 * (static_cast<size_t>(r) * w + i);
            px[0] = c.r;
            px[1] = c.g;
            px[2] = c.b;
            orc::Arena::mine().reset();
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

// ---- KAT hooks (the book's tests): an explicit jitter sequence (n_seq == 0: none, the cells' centres)
static area::Jitter katJitter(area::Cyclic& cyc, const double* seq, uint32_t n_seq) {
  area::Jitter J;
  if (n_seq > 0) {
    cyc.v.assign(seq, seq + n_seq);
    J.seq = &cyc;
  }
  return J;
}

// xyz_out[3]: point_on_light(u, v) of area_light(corner, full_uvec, usteps, full_vvec, vsteps)
int area_kat_point_on_light(const double* corner, const double* full_u, uint32_t us, const double* full_v, uint32_t vs,
                            const uint32_t* uv, uint32_t n_points, const double* seq, uint32_t n_seq, double* xyz_out) {
  const area::Light L = area::bookLight(corner, full_u, us, full_v, vs, n_seq > 0);
  area::Cyclic cyc;
  const area::Jitter J = katJitter(cyc, seq, n_seq);
  for (uint32_t i = 0; i < n_points; ++i) {
    const uint32_t u = uv[2 * i], v = uv[2 * i + 1], k = v * us + u;
    const double ju = J.at(L, 0, k, 0), jv = J.at(L, 0, k, 1);
    const orc::Tuple p = area::pointOnLight(L, u, v, ju, jv);
    xyz_out[3 * i] = p.x;
    xyz_out[3 * i + 1] = p.y;
    xyz_out[3 * i + 2] = p.z;
  }
  return 0;
}

// intensity_at of such a light (white) in the default world (world.zig:40-62), at each point; out_info[0..2] = the
// light's uvec, [3..5] vvec, [6] samples, [7..9] position (of the first call only)
int area_kat_intensity_at(const double* corner, const double* full_u, uint32_t us, const double* full_v, uint32_t vs,
                          const double* points, uint32_t n_points, const double* seq, uint32_t n_seq, double* out, double* info) {
  const orc::World w = orc::World::defaultWorld();
  const area::Light L = area::bookLight(corner, full_u, us, full_v, vs, n_seq > 0);
  area::Cyclic cyc;
  const area::Jitter J = katJitter(cyc, seq, n_seq);
  for (uint32_t i = 0; i < n_points; ++i)
    out[i] = area::intensityAt(w, L, 0, orc::point(points[3 * i], points[3 * i + 1], points[3 * i + 2]), J);
  if (info) {
    const double pos[3] = {(corner[0] + full_u[0] * 0.5) + full_v[0] * 0.5, (corner[1] + full_u[1] * 0.5) + full_v[1] * 0.5,
                           (corner[2] + full_u[2] * 0.5) + full_v[2] * 0.5};
    const double v[10] = {L.uvec.x, L.uvec.y, L.uvec.z, L.vvec.x, L.vvec.y, L.vvec.z, static_cast<double>(L.samples()), pos[0], pos[1], pos[2]};
    std::memcpy(info, v, sizeof v);
  }
  return 0;
}

// lighting() of an area light (white, unjittered) for a white surface of the given material (ambient, diffuse, specular,
// shininess) at pt with eyev and normal as given and intensity_at as given (the book passes 1.0); rgb_out[3]
int area_kat_lighting(const double* corner, const double* full_u, uint32_t us, const double* full_v, uint32_t vs, const double* mat4,
                      const double* pt, const double* eyev, const double* normal, double intensity, double* rgb_out) {
  const area::Light L = area::bookLight(corner, full_u, us, full_v, vs, false);
  orc::Material m;
  m.ambient = mat4[0];
  m.diffuse = mat4[1];
  m.specular = mat4[2];
  m.shininess = mat4[3];
  const area::Jitter J;
  const orc::Color effective = L.intensity;
  const orc::Color sum = area::areaSum(m, effective, L, 0, orc::point(pt[0], pt[1], pt[2]), orc::vec3(eyev[0], eyev[1], eyev[2]),
                                       orc::vec3(normal[0], normal[1], normal[2]), J);
  const double n = static_cast<double>(L.samples());
  rgb_out[0] = effective.r * m.ambient + (sum.r / n) * intensity;
  rgb_out[1] = effective.g * m.ambient + (sum.g / n) * intensity;
  rgb_out[2] = effective.b * m.ambient + (sum.b / n) * intensity;
  return 0;
}

// The jitter formula alone: out[i] = j(seed, p[i], n_lights[i], l[i], k[i], axis[i])
void area_kat_jitter(uint64_t seed, const uint64_t* p, const uint64_t* n_lights, const uint64_t* l, const uint64_t* k,
                     const uint64_t* axis, uint64_t n, double* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = area::hashJitter(seed, p[i], n_lights[i], l[i], k[i], axis[i]);
}

}  // extern "C"
