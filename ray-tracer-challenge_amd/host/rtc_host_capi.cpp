// rtc_host_capi.cpp — C entry points of librtc_host.so for non-C++ callers (the
// Python tests / bench harness use them through ctypes).  Everything here is
// scene loading and output formatting, i.e. the steps either side of the hot
// path; the per-pixel work is reached only through include/rtc.h.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rtc_host.h"
#include "rtc_api.hpp"
#include "rtc_loader.hpp"

namespace {

thread_local std::string g_error;

struct HostScene {
  rtc::SceneInfo info;
  rtc::FlatScene flat;
  rtc_scene_desc desc;
  rtc_light_desc lights;
};

template <typename F>
int guarded(F&& f) {
  try {
    g_error.clear();
    f();
    return 0;
  } catch (const rtc::Error& e) {
    g_error = e.what();
    return 1;
  } catch (const std::exception& e) {
    g_error = std::string("Unexpected: ") + e.what();
    return 2;
  }
}

}  // namespace

extern "C" {

// Error text of the last failing rtch_* call on this thread; begins with the Zig-style error name.
const char* rtch_last_error(void) { return g_error.c_str(); }

// parseScene (scene.zig:612-661) + flatten.  `data_dir` is where from-obj files are read
// from (the reference CLI reads "data/<file>", main.zig:14-21).
int rtch_scene_load(const char* scene_json, const char* data_dir, void** out) {
  return guarded([&] {
    auto hs = std::make_unique<HostScene>();
    hs->info = rtc::parseScene(scene_json, rtc::directoryLoader(data_dir ? data_dir : ""));
    hs->flat = rtc::flattenWorld(hs->info.world, hs->info.env_pattern ? &*hs->info.env_pattern : nullptr);
    hs->desc = hs->flat.desc();
    hs->lights = hs->flat.lights();
    *out = hs.release();
  });
}

// Threads parseScene may build a scene's objects on (0: what the process may use, at most 16; 1: one loop, as the
// reference).  The scene description does not depend on it.
void rtch_set_loader_threads(uint32_t threads) { rtc::setLoaderThreads(threads); }

void rtch_scene_free(void* h) { delete static_cast<HostScene*>(h); }

const rtc_scene_desc* rtch_scene_desc(void* h) { return &static_cast<HostScene*>(h)->desc; }
const rtc_light_desc* rtch_scene_lights(void* h) { return &static_cast<HostScene*>(h)->lights; }

int rtch_scene_sampling(void* h, rtc_sampling* out) {
  return guarded([&] {
    const rtc::CameraSampling& s = static_cast<HostScene*>(h)->info.sampling;
    *out = rtc_sampling{s.grid, s.jitter ? 1u : 0u, s.aperture, s.focal_distance, s.seed};
  });
}

int rtch_scene_passes(void* h, uint32_t* out) {
  return guarded([&] { *out = static_cast<HostScene*>(h)->info.sampling.passes; });
}

int rtch_scene_adaptive(void* h, int* enabled, rtc_adaptive* out) {
  return guarded([&] {
    const rtc::CameraSampling& s = static_cast<HostScene*>(h)->info.sampling;
    *enabled = s.adaptive ? 1 : 0;
    *out = s.adaptive ? rtc_adaptive{s.tile_w, s.tile_h, s.min_passes, s.passes, s.threshold} : rtc_adaptive{0u, 0u, 0u, 0u, 0.0};
  });
}

int rtch_scene_denoise(void* h, int* enabled, rtc_denoise_setting* out) {
  return guarded([&] {
    const rtc::CameraSampling& s = static_cast<HostScene*>(h)->info.sampling;
    *enabled = s.denoise ? 1 : 0;
    *out = rtc_denoise_setting{s.denoise_radius, s.denoise_patch, s.denoise_strength, s.denoise_cancel};
  });
}

int rtch_scene_robust(void* h, int* enabled, rtc_robust_setting* out) {
  return guarded([&] {
    const rtc::CameraSampling& s = static_cast<HostScene*>(h)->info.sampling;
    *enabled = s.robust ? 1 : 0;
    *out = rtc_robust_setting{s.robust_buckets, s.robust_gain};
  });
}

static rtc_film_setting filmSetting(const rtc::CameraFilm& f) {
  return rtc_film_setting{f.exposure, f.auto_key, f.bloom_radius, f.bloom_sigma, f.bloom_threshold, f.bloom_intensity, f.curve, f.white, f.transfer, f.gamma};
}

int rtch_scene_film(void* h, int* enabled, rtc_film_setting* out) {
  return guarded([&] {
    const rtc::CameraFilm& f = static_cast<HostScene*>(h)->info.film;
    *enabled = f.enabled ? 1 : 0;
    *out = filmSetting(f);
  });
}

int rtch_scene_motion(void* h, double* out, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->desc.n_roots)
      throw rtc::Error("InvalidArgument", "motion: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->desc.n_roots) + " roots");
    // (the description's roots are the World.objects entries in order, but for test shapes, which flattening drops)
    uint32_t r = 0;
    const auto& objects = hs->info.world.objects;
    for (size_t i = 0; i < objects.size() && r < n; ++i) {
      if (objects[i].kind == rtc::ShapeKind::TestShape) continue;
      for (int k = 0; k < 3; ++k) out[3ull * r + k] = hs->info.motion[3 * i + k];
      ++r;
    }
  });
}

int rtch_scene_spots(void* h, uint8_t* cone, double* axis, double* cos_inner, double* cos_outer, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->lights.n_lights)
      throw rtc::Error("InvalidArgument", "spots: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->lights.n_lights) + " lights");
    if (n != 0u && (!cone || !axis || !cos_inner || !cos_outer)) throw rtc::Error("InvalidArgument", "spots: null argument");
    for (uint32_t i = 0; i < n; ++i) {  // (World.lights order: the light table's)
      const rtc::SpotCone& c = hs->info.spots[i];
      cone[i] = c.cone;
      for (int k = 0; k < 3; ++k) axis[3ull * i + k] = c.axis[k];
      cos_inner[i] = c.cos_inner;
      cos_outer[i] = c.cos_outer;
    }
  });
}

int rtch_scene_bumps(void* h, uint8_t* kind, double* amplitude, uint32_t* octaves, double* persistence, double* inverse, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->desc.n_materials)
      throw rtc::Error("InvalidArgument", "bumps: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->desc.n_materials) + " materials");
    if (n != 0u && (!kind || !amplitude || !octaves || !persistence || !inverse)) throw rtc::Error("InvalidArgument", "bumps: null argument");
    for (uint32_t i = 0; i < n; ++i) {  // (mat_* order)
      const rtc::Bump& b = hs->flat.mat_bump[i];
      kind[i] = b.kind;
      amplitude[i] = b.amplitude;
      octaves[i] = b.octaves;
      persistence[i] = b.persistence;
      for (int k = 0; k < 12; ++k) inverse[12ull * i + k] = b.inverse.d[k / 4][k % 4];
    }
  });
}

// The materials' "roughness" (DESIGN.md section 20), in mat_* order, and the camera's "gloss-seed", as rtc_scene_set_gloss
// takes them; *present: some material of the file has the key.
int rtch_scene_gloss(void* h, double* reflection, double* transmission, uint64_t* seed, int* present, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->desc.n_materials)
      throw rtc::Error("InvalidArgument", "gloss: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->desc.n_materials) + " materials");
    if (n != 0u && (!reflection || !transmission)) throw rtc::Error("InvalidArgument", "gloss: null argument");
    for (uint32_t i = 0; i < n; ++i) {  // (mat_* order)
      reflection[i] = hs->flat.mat_gloss[2ull * i + 0];
      transmission[i] = hs->flat.mat_gloss[2ull * i + 1];
    }
    if (seed) *seed = hs->info.sampling.gloss_seed;
    if (present) *present = hs->flat.gloss_present ? 1 : 0;
  });
}

// The materials' "ambient-occlusion" radii, in mat_* order, and the camera's "occlusion-samples" and
// "occlusion-seed", as rtc_scene_set_occlusion takes them; *present: some material of the file has the key.
int rtch_scene_occlusion(void* h, double* radius, uint32_t* samples, uint64_t* seed, int* present, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->desc.n_materials)
      throw rtc::Error("InvalidArgument", "occlusion: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->desc.n_materials) + " materials");
    if (n != 0u && !radius) throw rtc::Error("InvalidArgument", "occlusion: null argument");
    for (uint32_t i = 0; i < n; ++i) radius[i] = hs->flat.mat_occlusion[i];  // (mat_* order)
    if (samples) *samples = hs->info.sampling.occlusion_samples;
    if (seed) *seed = hs->info.sampling.occlusion_seed;
    if (present) *present = hs->flat.occlusion_present ? 1 : 0;
  });
}

// The materials' "shadow-filter" rows, in mat_* order, three doubles each, as
// rtc_scene_set_shadow_filters takes them; *present: some material of the file has the key.
int rtch_scene_shadow_filters(void* h, double* rgb, int* present, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->desc.n_materials)
      throw rtc::Error("InvalidArgument", "shadow filters: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->desc.n_materials) + " materials");
    if (n != 0u && !rgb) throw rtc::Error("InvalidArgument", "shadow filters: null argument");
    for (size_t i = 0; i < 3u * static_cast<size_t>(n); ++i) rgb[i] = hs->flat.mat_shadow_filter[i];  // (mat_* order)
    if (present) *present = hs->flat.shadow_filter_present ? 1 : 0;
  });
}

// The materials' "absorption" rows, in mat_* order, three doubles each, and the scene's "atmosphere"
// (fog[0]: the density; fog[1..3]: the colour), as rtc_scene_set_media takes them; *present: some material of the file has
// the key, or the file has an atmosphere.
int rtch_scene_media(void* h, double* absorption, double* fog, int* present, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->desc.n_materials)
      throw rtc::Error("InvalidArgument", "media: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->desc.n_materials) + " materials");
    if ((n != 0u && !absorption) || !fog) throw rtc::Error("InvalidArgument", "media: null argument");
    for (size_t i = 0; i < 3u * static_cast<size_t>(n); ++i) absorption[i] = hs->flat.mat_absorption[i];  // (mat_* order)
    fog[0] = hs->info.fog_density;
    for (int c = 0; c < 3; ++c) fog[1 + c] = hs->info.fog_color[c];
    if (present) *present = (hs->flat.absorption_present || hs->info.atmosphere_present) ? 1 : 0;
  });
}

// The scene's "environment"  as rtc_scene_set_environment takes it: `out`'s rgb, pattern - a row of
// the description's pat_* tables, after every material's -, projection and n_suns; the suns' directions and intensities, as
// the file has them, into sun_direction and sun_rgb (3 * RTC_ENV_MAX_SUNS doubles each), which `out` then points to;
// *present: the file has the key.
int rtch_scene_environment(void* h, rtc_environment* out, double* sun_direction, double* sun_rgb, int* present) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (!out || !sun_direction || !sun_rgb) throw rtc::Error("InvalidArgument", "environment: null argument");
    std::memset(out, 0, sizeof(*out));
    for (int c = 0; c < 3; ++c) out->rgb[c] = hs->info.env_color[c];
    out->pattern = hs->flat.env_pattern;
    out->projection = hs->info.env_projection;
    out->n_suns = static_cast<uint32_t>(hs->info.sun_direction.size() / 3u);
    for (size_t i = 0; i < hs->info.sun_direction.size(); ++i) {
      sun_direction[i] = hs->info.sun_direction[i];
      sun_rgb[i] = hs->info.sun_intensity[i];
    }
    out->sun_direction = sun_direction;
    out->sun_rgb = sun_rgb;
    if (present) *present = hs->info.environment_present ? 1 : 0;
  });
}

// The environment's "light"  as rtc_scene_set_sky_light takes it; *present: the file has the key.
int rtch_scene_sky_light(void* h, rtc_sky_light* out, int* present) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (!out) throw rtc::Error("InvalidArgument", "sky light: null argument");
    std::memset(out, 0, sizeof(*out));
    out->gain = hs->info.sky_light_gain;
    out->samples = hs->info.sky_light_samples;
    out->seed = hs->info.sky_light_seed;
    if (present) *present = hs->info.sky_light_present ? 1 : 0;
  });
}

// The scene's "indirect" and the materials' "emission" rows, in mat_* order, three doubles each, as
// rtc_scene_set_indirect takes them; *out points to `emission`.  *present: the file has either key.
int rtch_scene_indirect(void* h, rtc_indirect* out, double* emission, int* present, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (!out) throw rtc::Error("InvalidArgument", "indirect: null argument");
    if (n != hs->desc.n_materials)
      throw rtc::Error("InvalidArgument", "indirect: room for " + std::to_string(n) + " materials, the scene has " + std::to_string(hs->desc.n_materials));
    if (n != 0u && !emission) throw rtc::Error("InvalidArgument", "indirect: null argument");
    for (size_t i = 0; i < 3u * static_cast<size_t>(n); ++i) emission[i] = hs->flat.mat_emission[i];  // (mat_* order)
    std::memset(out, 0, sizeof(*out));
    out->gain = hs->info.indirect_gain;
    out->bounces = hs->info.indirect_bounces;
    out->seed = hs->info.indirect_seed;
    out->emission = emission;
    out->n_materials = n;
    if (present) *present = (hs->info.indirect_present || hs->flat.emission_present) ? 1 : 0;
  });
}

// The "emitters" key of the scene's "indirect" (DESIGN.md section 28), as rtc_scene_set_emitters takes it.  *present: the file
// has the key (and it is not false).
int rtch_scene_emitters(void* h, rtc_emitters* out, int* present) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (!out) throw rtc::Error("InvalidArgument", "emitters: null argument");
    std::memset(out, 0, sizeof(*out));
    out->samples = hs->info.emitters_samples;
    out->seed = hs->info.emitters_seed;
    if (present) *present = hs->info.emitters_present ? 1 : 0;
  });
}

// The "mis" key inside the scene's "emitters" (DESIGN.md section 32), as rtc_scene_set_emitter_mis takes it: 1 where the file
// has the key and it is true, else 0.
int rtch_scene_emitter_mis(void* h, uint32_t* mode) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (!mode) throw rtc::Error("InvalidArgument", "emitter mis: null argument");
    *mode = (hs->info.emitters_present && hs->info.emitters_mis) ? 1u : 0u;
  });
}

// The triangles' texture rows (RTC_TEX_MESH), in tri_* order, as rtc_scene_set_mesh_uvs takes them.
int rtch_scene_mesh_uvs(void* h, double* uv, uint32_t n) {
  return guarded([&] {
    const HostScene* hs = static_cast<HostScene*>(h);
    if (n != hs->desc.n_tris)
      throw rtc::Error("InvalidArgument", "mesh uvs: n " + std::to_string(n) + ", the scene has " + std::to_string(hs->desc.n_tris) + " triangles");
    if (n != 0u && !uv) throw rtc::Error("InvalidArgument", "mesh uvs: null argument");
    for (size_t i = 0; i < 6ull * n; ++i) uv[i] = hs->flat.tri_uv[i];
  });
}

// Camera of the scene file; width/height 0 keep the file's values, otherwise they replace
// camera.width/height before Camera.new runs (the reference has no such override).
int rtch_scene_camera(void* h, uint32_t width, uint32_t height, rtc_camera* out) {
  return guarded([&] {
    const rtc::Camera& c0 = static_cast<HostScene*>(h)->info.camera;
    rtc::Camera c = rtc::Camera::create(width ? width : c0.hsize, height ? height : c0.vsize, c0.fov);
    c.setTransform(c0.transform);
    *out = rtc::flattenCamera(c);
  });
}

// lib.zig:166-190 on the scene's own camera (the "preheated" interactive mode): the next rtch_scene_camera
// returns the moved camera; the GPU scene handle is untouched.
int rtch_camera_rotate(void* h, double angle) {
  return guarded([&] { rtc::rotateCamera(static_cast<HostScene*>(h)->info.camera, angle); });
}
int rtch_camera_move(void* h, double distance) {
  return guarded([&] { rtc::moveCamera(static_cast<HostScene*>(h)->info.camera, distance); });
}

// Camera.new + viewTransform for callers that build cameras themselves (camera.zig:33-61).
int rtch_camera_make(uint32_t hsize, uint32_t vsize, double fov, const double from[3], const double to[3],
                     const double up[3], rtc_camera* out) {
  return guarded([&] {
    rtc::Camera c = rtc::Camera::create(hsize, vsize, fov);
    c.setTransform(rtc::Matrix4::viewTransform(rtc::Tuple::point(from[0], from[1], from[2]),
                                               rtc::Tuple::point(to[0], to[1], to[2]),
                                               rtc::Tuple::vec3(up[0], up[1], up[2])));
    *out = rtc::flattenCamera(c);
  });
}

// Canvas.ppm (canvas.zig:181-254) of an [h][w][3] f64 image.  Returns the number of bytes
// needed; writes at most `cap` bytes to `buf`.
size_t rtch_canvas_ppm(const double* rgb, uint32_t w, uint32_t h, char* buf, size_t cap) {
  rtc::Canvas c = rtc::Canvas::create(w, h);
  std::memcpy(static_cast<void*>(c.pixels.data()), rgb, sizeof(double) * 3 * w * h);
  const std::string s = c.ppm();
  if (buf && cap) std::memcpy(buf, s.data(), s.size() < cap ? s.size() : cap);
  return s.size();
}

// lib.zig:146-153: RGBA8 framebuffer, clamp()'d channels, alpha 255.
void rtch_canvas_rgba8(const double* rgb, uint32_t w, uint32_t h, uint8_t* out) {
  for (size_t i = 0; i < static_cast<size_t>(w) * h; ++i) {
    out[4 * i + 0] = rtc::clampChannel(rgb[3 * i + 0]);
    out[4 * i + 1] = rtc::clampChannel(rgb[3 * i + 1]);
    out[4 * i + 2] = rtc::clampChannel(rgb[3 * i + 2]);
    out[4 * i + 3] = 255;
  }
}

// Whole-path convenience for C callers: Camera.render(world) through the GPU library.
int rtch_scene_render(void* h, uint32_t width, uint32_t height, uint32_t max_depth, double* rgb_out) {
  return guarded([&] {
    HostScene* hs = static_cast<HostScene*>(h);
    rtc_camera cam;
    const rtc::Camera& c0 = hs->info.camera;
    rtc::Camera c = rtc::Camera::create(width ? width : c0.hsize, height ? height : c0.vsize, c0.fov);
    c.setTransform(c0.transform);
    cam = rtc::flattenCamera(c);
    // (several sample passes: each rendered into `frame`, summed in pass order into rgb_out, divided once by their
    // number - the bits of rtc_scene_accumulate_device's mean)
    const uint32_t passes = hs->info.sampling.passes;
    const size_t n = 3ull * cam.hsize * cam.vsize;
    std::vector<double> frame(passes > 1u && !hs->info.sampling.denoise && !hs->info.film.enabled && !hs->info.sampling.robust ? n : 0u);
    rtc_scene* scene = nullptr;
    // (a scene with area lights: its light table; point lights only: the description alone, as before)
    int st = hs->flat.has_area_light ? rtc_scene_create_with_lights(&hs->desc, &hs->lights, &scene) : rtc_scene_create(&hs->desc, &scene);
    if (st == RTC_OK) {
      rtc_sampling smp;
      if (rtch_scene_sampling(h, &smp) != 0) smp = rtc_sampling{1u, 0u, 0.0, 1.0, 0u};
      st = rtc_scene_set_sampling(scene, &smp);
      if (st == RTC_OK) {  // (the top-level objects' "motion"; all zero: static)
        std::vector<double> disp(3ull * hs->desc.n_roots);
        if (rtch_scene_motion(h, disp.data(), hs->desc.n_roots) != 0) throw rtc::Error("InvalidArgument", g_error);
        const rtc_motion m{hs->desc.n_roots, disp.data()};
        st = rtc_scene_set_motion(scene, &m);
      }
      if (st == RTC_OK) {  // (the "spot-light" entries' cones; none: the handle as it is)
        const uint32_t nl = hs->lights.n_lights;
        std::vector<uint8_t> cone(nl);
        std::vector<double> axis(3ull * nl), ci(nl), co(nl);
        if (rtch_scene_spots(h, cone.data(), axis.data(), ci.data(), co.data(), nl) != 0) throw rtc::Error("InvalidArgument", g_error);
        const rtc_spot sp{nl, cone.data(), axis.data(), ci.data(), co.data()};
        st = rtc_scene_set_spots(scene, &sp);
      }
      if (st == RTC_OK) {  // (the materials' "normal-perturbation" entries; none: the handle as it is)
        const uint32_t nm = hs->desc.n_materials;
        std::vector<uint8_t> kind(nm);
        std::vector<uint32_t> oct(nm);
        std::vector<double> amp(nm), per(nm), inv(12ull * nm);
        if (rtch_scene_bumps(h, kind.data(), amp.data(), oct.data(), per.data(), inv.data(), nm) != 0) throw rtc::Error("InvalidArgument", g_error);
        const rtc_bump bp{nm, kind.data(), amp.data(), oct.data(), per.data(), inv.data()};
        st = rtc_scene_set_bumps(scene, &bp);
      }
      if (st == RTC_OK && hs->desc.n_tris != 0u) {  // (the triangles' texture rows; all zero: the handle as it is)
        const std::vector<double>& rows = hs->flat.tri_uv;
        bool any = false;
        for (const double x : rows) any = any || x != 0.0;
        const rtc_mesh_uvs mu{hs->desc.n_tris, rows.data()};
        if (any) st = rtc_scene_set_mesh_uvs(scene, &mu);
      }
      if (st == RTC_OK && hs->flat.gloss_present) {  // (the materials' roughness; all zero: the handle as it is)
        const uint32_t nm = hs->desc.n_materials;
        std::vector<double> refl(nm), trans(nm);
        for (uint32_t i = 0; i < nm; ++i) refl[i] = hs->flat.mat_gloss[2ull * i], trans[i] = hs->flat.mat_gloss[2ull * i + 1];
        const rtc_gloss gl{nm, refl.data(), trans.data(), hs->info.sampling.gloss_seed};
        st = rtc_scene_set_gloss(scene, &gl);
      }
      if (st == RTC_OK && hs->flat.occlusion_present) {  // (the materials' occlusion radii; all zero: the handle as it is)
        const rtc_occlusion oc{hs->desc.n_materials, hs->flat.mat_occlusion.data(), hs->info.sampling.occlusion_samples,
                               hs->info.sampling.occlusion_seed};
        st = rtc_scene_set_occlusion(scene, &oc);
      }
      if (st == RTC_OK && hs->flat.shadow_filter_present) {  // (the materials' shadow filters; all zero: the handle as it is)
        const rtc_shadow_filters sf{hs->desc.n_materials, hs->flat.mat_shadow_filter.data()};
        st = rtc_scene_set_shadow_filters(scene, &sf);
      }
      if (st == RTC_OK && (hs->flat.absorption_present || hs->info.atmosphere_present)) {  // (the media; all zero: the handle as it is)
        const rtc_media me{hs->desc.n_materials, hs->flat.mat_absorption.data(), hs->info.fog_density,
                           {hs->info.fog_color[0], hs->info.fog_color[1], hs->info.fog_color[2]}};
        st = rtc_scene_set_media(scene, &me);
      }
      if (st == RTC_OK && hs->info.environment_present) {  // (the environment; no sky and no sun: the handle as it is)
        const rtc_environment ev{{hs->info.env_color[0], hs->info.env_color[1], hs->info.env_color[2]},
                                 hs->flat.env_pattern,
                                 hs->info.env_projection,
                                 static_cast<uint32_t>(hs->info.sun_direction.size() / 3u),
                                 hs->info.sun_direction.data(),
                                 hs->info.sun_intensity.data()};
        st = rtc_scene_set_environment(scene, &ev);
      }
      if (st == RTC_OK && hs->info.sky_light_present) {  // (the sky light; a gain of zero: the handle as it is)
        const rtc_sky_light sl{hs->info.sky_light_gain, hs->info.sky_light_samples, hs->info.sky_light_seed};
        st = rtc_scene_set_sky_light(scene, &sl);
      }
      if (st == RTC_OK && (hs->info.indirect_present || hs->flat.emission_present)) {  // (indirect light; nothing to form or emit: the handle as it is)
        const rtc_indirect in{hs->info.indirect_gain, hs->info.indirect_bounces, hs->info.indirect_seed, hs->flat.mat_emission.data(),
                              hs->desc.n_materials};
        st = rtc_scene_set_indirect(scene, &in);
      }
      if (st == RTC_OK && hs->info.emitters_present) {  // (emitter sampling: the list is derived from the tables set above)
        const rtc_emitters em{hs->info.emitters_samples, hs->info.emitters_seed};
        st = rtc_scene_set_emitters(scene, &em);
        if (st == RTC_OK) st = rtc_scene_set_emitter_mis(scene, hs->info.emitters_mis ? 1u : 0u);  // (after the emitter table)
      }
      const rtc::CameraSampling& cs = hs->info.sampling;
      if (cs.robust && st == RTC_OK) {  // (bucket sums and their resolve, then the file's denoiser and film stage, section 31)
        const rtc_robust_setting rb{cs.robust_buckets, cs.robust_gain};
        const rtc_denoise_setting dn{cs.denoise_radius, cs.denoise_patch, cs.denoise_strength, cs.denoise_cancel};
        const rtc_film_setting film = filmSetting(hs->info.film);
        st = rtc_render_robust(scene, &cam, max_depth, passes, &rb, cs.denoise ? &dn : nullptr, hs->info.film.enabled ? &film : nullptr,
                               rgb_out, nullptr, nullptr, nullptr, nullptr);
      } else if (hs->info.film.enabled && st == RTC_OK) {  // (the whole path on the device, the film stage last, section 30)
        const rtc_adaptive a{cs.tile_w, cs.tile_h, cs.min_passes, cs.passes, cs.threshold};
        const rtc_denoise_setting dn{cs.denoise_radius, cs.denoise_patch, cs.denoise_strength, cs.denoise_cancel};
        const rtc_film_setting film = filmSetting(hs->info.film);
        st = rtc_render_filmed(scene, &cam, max_depth, passes, cs.adaptive ? &a : nullptr, cs.denoise ? &dn : nullptr, &film, rgb_out, nullptr, nullptr);
      } else if (cs.denoise && st == RTC_OK) {  // (the denoiser over the accumulated passes, or over an adaptive run, section 29)
        const rtc_adaptive a{cs.tile_w, cs.tile_h, cs.min_passes, cs.passes, cs.threshold};
        const rtc_denoise_setting dn{cs.denoise_radius, cs.denoise_patch, cs.denoise_strength, cs.denoise_cancel};
        st = rtc_render_denoised(scene, &cam, max_depth, passes, cs.adaptive ? &a : nullptr, &dn, rgb_out, nullptr);
      } else if (cs.adaptive && st == RTC_OK) {  // (adaptive sampling: each tile's mean after its own passes, section 15)
        const rtc_adaptive a{cs.tile_w, cs.tile_h, cs.min_passes, cs.passes, cs.threshold};
        st = rtc_render_adaptive(scene, &cam, max_depth, &a, rgb_out, nullptr);
      }
      const bool on_host = !cs.adaptive && !cs.denoise && !hs->info.film.enabled && !cs.robust;  // (the passes summed here)
      for (uint32_t p = 0; p < passes && st == RTC_OK && on_host; ++p) {
        if (p > 0u) st = rtc_scene_set_sample_pass(scene, p);
        if (st == RTC_OK) st = rtc_render(scene, &cam, max_depth, 0, 0, cam.hsize, cam.vsize, p == 0u ? rgb_out : frame.data());
        if (st == RTC_OK && p > 0u)
          for (size_t i = 0; i < n; ++i) rgb_out[i] = rgb_out[i] + frame[i];
      }
      if (st == RTC_OK && passes > 1u && on_host)
        for (size_t i = 0; i < n; ++i) rgb_out[i] = rgb_out[i] / static_cast<double>(passes);
      rtc_scene_destroy(scene);
    }
    if (st != RTC_OK) throw rtc::Error(rtc_status_name(st), rtc_last_error());
  });
}

}  // extern "C"
