// rtc_loader.hpp — scene JSON + OBJ loaders (the step immediately before the hot
// path).  Restates src/parsing/scene.zig and
// src/parsing/obj.zig; see rtc_loader.cpp for the line-by-line citations.
#pragma once
#include <functional>
#include <map>
#include <optional>
#include <string>
#include <string_view>
#include <vector>

#include "rtc_scene.hpp"

namespace rtc {

// scene.zig:612-618 `load_file_data` callback: file name -> bytes.
using FileLoader = std::function<std::string(const std::string& file_name)>;
FileLoader directoryLoader(const std::string& dir);  // main.zig:14-21 ("data/" + name)

// The camera's optional "sampling" (not in the reference): camera samples per pixel, as
// rtc_scene_set_sampling takes them.  Absent: one centred ray per pixel.
struct CameraSampling {
  uint32_t grid = 1;
  bool jitter = false;
  double aperture = 0.0;
  double focal_distance = 1.0;  // (absent with an aperture: |to - from|)
  uint64_t seed = 0;
  uint32_t passes = 1;  // sample passes rtch_scene_render averages (rtc_scene_set_sample_pass 0 .. passes-1; section 13)
  // "adaptive" (section 15): passes only for tiles still noisy; "passes" is then the most a tile takes
  bool adaptive = false;
  double threshold = 0.0;
  uint32_t min_passes = 4;
  uint32_t tile_w = 16, tile_h = 16;
  // "denoise" (section 29): rtch_scene_render filters the accumulated image (rtc_render_denoised); rtc_denoise_setting's values
  bool denoise = false;
  uint32_t denoise_radius = 7, denoise_patch = 2;
  double denoise_strength = 0.45, denoise_cancel = 1.0;
  // "robust" (section 31): rtch_scene_render resolves bucket sums (rtc_render_robust); rtc_robust_setting's values
  bool robust = false;
  uint32_t robust_buckets = 5;
  double robust_gain = 1.0;
  uint64_t gloss_seed = 0;  // "gloss-seed" (section 20): rtc_gloss::seed of the materials' "roughness"
  uint32_t occlusion_samples = 1;  // "occlusion-samples" (section 21): rtc_occlusion::samples of the materials' "ambient-occlusion"
  uint64_t occlusion_seed = 0;     // "occlusion-seed": rtc_occlusion::seed
};

// The camera's optional "film" (not in the reference): rtc_film_setting's values, as rtc_render_filmed
// takes them.  Absent or false: no film stage, rtch_scene_render gives the linear image.
struct CameraFilm {
  bool enabled = false;
  double exposure = 1.0, auto_key = 0.0;
  uint32_t bloom_radius = 0;
  double bloom_sigma = 4.0, bloom_threshold = 1.0, bloom_intensity = 0.0;
  uint32_t curve = 2;  // RTC_FILM_CURVE_ACES
  double white = 4.0;
  uint32_t transfer = 1;  // RTC_FILM_TRANSFER_SRGB
  double gamma = 2.2;
};

// A "spot-light" entry's cone (not in the reference), as rtc_scene_set_spots takes it: the axis as
// given ("to" - position, or "direction"), and the cosines of the half-angles (std::cos).  cone 0: a light without one.
struct SpotCone {
  uint8_t cone = 0;
  double axis[3] = {0.0, 0.0, 0.0};
  double cos_inner = 1.0, cos_outer = 1.0;
};

struct SceneInfo {  // scene.zig:608-610
  Camera camera;
  World world;
  CameraSampling sampling;
  CameraFilm film;
  std::vector<double> motion;  // [objects][3]: each top-level object's optional "motion" (DESIGN.md section 14), else 0
  std::vector<SpotCone> spots;  // [lights]: a "spot-light" entry's cone (section 16); cone 0 for every other light
  // the scene's "atmosphere": {"density": d, "color": [r, g, b]} (section 23): rtc_media's fog; all zero without the key
  bool atmosphere_present = false;
  double fog_density = 0.0;
  double fog_color[3] = {0.0, 0.0, 0.0};
  // the scene's "environment" (section 24): rtc_environment's sky and suns; nothing without the key
  bool environment_present = false;
  double env_color[3] = {0.0, 0.0, 0.0};
  std::optional<Pattern> env_pattern;
  uint32_t env_projection = 0u;            // RTC_ENV_SPHERE / RTC_ENV_CUBE
  std::vector<double> sun_direction;       // [suns][3], as the file has them
  std::vector<double> sun_intensity;       // [suns][3]
  // the environment's "light" (section 25): rtc_sky_light's values; gain 0 without the key
  bool sky_light_present = false;
  double sky_light_gain = 0.0;
  uint32_t sky_light_samples = 1u;
  uint64_t sky_light_seed = 0u;
  // the scene's "indirect" (section 27): rtc_indirect's values; gain 0 and bounces 0 without the key
  bool indirect_present = false;
  double indirect_gain = 0.0;
  uint32_t indirect_bounces = 0u;
  uint64_t indirect_seed = 0u;
  // the "emitters" key of "indirect" (section 28): rtc_emitters' values; samples 1 and seed 0 without the key
  bool emitters_present = false;
  uint32_t emitters_samples = 1u;
  uint64_t emitters_seed = 0u;
  // the "mis" key inside the object form of "emitters" (section 32): rtc_scene_set_emitter_mis' mode 1; false without the key
  bool emitters_mis = false;
};

// scene.zig:612-661.  Throws rtc::Error whose .name is the Zig error name
// (UnknownDefinition, NotInvertible, MissingField, UnknownField, ...).
SceneInfo parseScene(const std::string& scene_json, const FileLoader& load_file_data);
// The entries of "objects" are independent of each other (definitions are read-only, an object's transform, material and
// divide(8) are its own): parseScene builds them on up to this many threads - 0: what the process may use (CPU affinity,
// cgroup quota), at most 16; 1: the reference's one loop.  The World is the same to the bit whatever the count (ids
// included: ShapeIdScope); `load_file_data` must then be callable from several threads at once (directoryLoader is).
void setLoaderThreads(unsigned threads);
unsigned loaderThreads();

// obj.zig:11-286
class ObjParser {
 public:
  struct InheritedState {  // obj.zig:186-189
    std::optional<Material> material;
    std::optional<bool> casts_shadow;
  };

  ObjParser();
  void loadObj(const std::string& obj, const InheritedState& state, bool normalize);  // obj.zig:191-279
  Shape toGroup() const { return default_group; }                                      // obj.zig:281-283
  Shape takeGroup() { return std::move(default_group); }  // the same, for a parser that is done (no copy of a kilobyte per triangle)

  Shape default_group;
  std::map<std::string, size_t> named_groups;  // name -> index in default_group.children
  Tuple offset = Tuple::vec3(0.0, 0.0, 0.0);
  double scale = 1.0;
  std::vector<Tuple> vertices;
  std::vector<Tuple> normals;
  // "texture-coordinates" of from-obj (not in the reference).  false: `vt` lines are ignored lines
  // and a face vertex's t field is never read, as in obj.zig.  true: `vt u v [w]` lines fill `texcoords`, and a face
  // vertex's t field, 1-indexed into them, gives its triangles' texture rows ((0, 0) for a vertex without one).
  bool texture_coordinates = false;
  std::vector<std::pair<double, double>> texcoords;
  size_t lines_ignored = 0;
  // the same count by the name of the line error that made the line an ignored one ("UnknownFirstToken",
  // "IncompleteVertex", "InvalidCharacter", ...): what a refusal by name of one line is, where a line error never leaves
  // the parser (obj.zig:277)
  std::map<std::string, size_t> ignored_by_error;

 private:
  long active_group_ = -1;  // -1: default group, else index into default_group.children
  Shape& activeGroup() { return active_group_ < 0 ? default_group : default_group.children[active_group_]; }
  void handleLine(std::string_view line, const InheritedState& state);
  std::vector<std::string_view> line_tokens_;  // (scratch of handleLine)
};

}  // namespace rtc
