// rtc_flatten.hpp — World(T) -> flat SoA tables (include/rtc.h: rtc_scene_desc).
//
// Walks World.objects depth-first in the order World.intersect / Group.localIntersect
// visit them (world.zig:74, group.zig:52), so that leaf index == the position the
// reference's nested stable sorts give an intersection among equal t's.
// One node per reference Group, with the Group's own _bbox: identical boxes give
// identical candidate sets.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rtc.h"
#include "rtc_scene.hpp"

namespace rtc {

struct FlatScene {
  std::vector<double> xf_inv, xf_inv_t;
  std::vector<uint8_t> leaf_kind, leaf_shadow;
  std::vector<uint32_t> leaf_xform, leaf_material, leaf_id, leaf_geom;
  std::vector<double> cyl_min, cyl_max;
  std::vector<uint8_t> cyl_closed;
  std::vector<double> tri_p1, tri_e1, tri_e2, tri_n1, tri_n2, tri_n3;
  std::vector<double> tri_uv;  // [n_tris][6]: each triangle's texture row (rtch_scene_mesh_uvs; not part of rtc_scene_desc)
  std::vector<double> mat_params;
  std::vector<uint32_t> mat_pattern;
  std::vector<double> mat_gloss;  // [n_materials][2]: each row's "roughness" (reflection, transmission) (rtch_scene_gloss; not part of rtc_scene_desc)
  bool gloss_present = false;     // some material of the scene has the "roughness" key
  std::vector<double> mat_occlusion;  // [n_materials]: each row's "ambient-occlusion" radius (rtch_scene_occlusion; not part of rtc_scene_desc)
  bool occlusion_present = false;     // some material of the scene has the "ambient-occlusion" key
  std::vector<double> mat_shadow_filter;  // [n_materials][3]: each row's "shadow-filter" (rtch_scene_shadow_filters; not part of rtc_scene_desc)
  bool shadow_filter_present = false;     // some material of the scene has the "shadow-filter" key
  std::vector<double> mat_absorption;  // [n_materials][3]: each row's "absorption" (rtch_scene_media; not part of rtc_scene_desc)
  bool absorption_present = false;     // some material of the scene has the "absorption" key
  std::vector<double> mat_emission;    // [n_materials][3]: each row's "emission" (rtch_scene_indirect; not part of rtc_scene_desc)
  bool emission_present = false;       // some material of the scene has the "emission" key
  uint32_t env_pattern = 0xFFFFFFFFu;  // the environment's pattern row (rtch_scene_environment), or RTC_ENV_NO_PATTERN; not part of rtc_scene_desc
  std::vector<Bump> mat_bump;  // [n_materials]: each row's "normal-perturbation" (rtch_scene_bumps; not part of rtc_scene_desc)
  std::vector<uint8_t> pat_kind;
  std::vector<double> pat_inv, pat_rgb;
  std::vector<uint32_t> pat_a, pat_b;
  std::vector<double> node_min, node_max;
  std::vector<uint32_t> node_first, node_count, children, roots;
  std::vector<uint8_t> node_op;
  // texture maps (rtc.h tex_*, uv_*, img_*)
  std::vector<uint8_t> tex_mapping, uv_kind, uv_interp;
  std::vector<uint32_t> tex_uv, uv_sub, uv_image, img_width, img_height;
  std::vector<double> uv_size;
  std::vector<uint64_t> img_offset;
  std::vector<float> img_rgb;
  std::vector<double> light_pos, light_rgb;
  // World.lights of both kinds (rtc_light_desc): light_pos / light_rgb above hold every light as a point light - an
  // area light at its centre, so that a caller of rtc_scene_create alone still renders a valid world (hard shadows
  // from the centres); rtc_scene_create_with_lights takes this table instead.
  std::vector<uint8_t> light_kind, light_jitter;
  std::vector<double> light_corner, light_uvec, light_vvec;
  std::vector<uint32_t> light_usteps, light_vsteps;
  bool has_area_light = false;

  // View over the vectors above; valid while *this is alive and unmodified.
  rtc_scene_desc desc() const;
  rtc_light_desc lights() const;

  size_t leafCount() const { return leaf_kind.size(); }
  size_t nodeCount() const { return node_first.size(); }
};

// (environment_pattern: the "environment"'s pattern, DESIGN.md section 24 - its rows, and the images it names, are interned
// after every material's: the tables of the same file without the key, and then those rows; FlatScene::env_pattern)
FlatScene flattenWorld(const World& world, const Pattern* environment_pattern = nullptr);
rtc_camera flattenCamera(const Camera& camera);

}  // namespace rtc
