/*
 * rtc_host.h — C entry points of librtc_host.so: the steps either side of the
 * hot path (scene JSON / OBJ / PNG loading and flattening before it, Canvas
 * output after it), for callers that are not C++.  The per-pixel work is
 * reached only through include/rtc.h; nothing here renders on the CPU.
 *
 * Reference counterparts:
 *   rtch_scene_load      parseScene, src/parsing/scene.zig:612-661 (+ obj.zig, zigimg PNG decode), then the
 *                        depth-first flattening into rtc_scene_desc
 *   rtch_scene_camera    SceneInfo.camera (scene.zig:633-648); width/height override the file's values
 *   rtch_camera_rotate   Renderer.rotateCamera, src/lib.zig:166-178
 *   rtch_camera_move     Renderer.moveCamera,   src/lib.zig:180-190
 *   rtch_camera_make     Camera.new + Matrix.viewTransform, camera.zig:33-61, matrix.zig:54-67
 *   rtch_canvas_ppm      Canvas.ppm, canvas.zig:181-254
 *   rtch_canvas_rgba8    the RGBA8 framebuffer of lib.zig:146-153 (clamp, color.zig:61-71)
 *   rtch_scene_render    main.zig:92: load -> Camera.render -> Canvas, through rtc_scene_create / rtc_render
 *                        (rtc_scene_create_with_lights when the scene has an area light; the camera's
 *                        sampling, rtch_scene_sampling, through rtc_scene_set_sampling; its sample passes,
 *                        rtch_scene_passes, through rtc_scene_set_sample_pass, averaged on the host; the
 *                        top-level objects' motion, rtch_scene_motion, through rtc_scene_set_motion; its adaptive
 *                        sampling, rtch_scene_adaptive, through rtc_render_adaptive; its spot lights,
 *                        rtch_scene_spots, through rtc_scene_set_spots; its materials' normal perturbation,
 *                        rtch_scene_bumps, through rtc_scene_set_bumps; its triangles' texture rows,
 *                        rtch_scene_mesh_uvs, through rtc_scene_set_mesh_uvs; its materials' roughness,
 *                        rtch_scene_gloss, through rtc_scene_set_gloss; its materials' occlusion radii,
 *                        rtch_scene_occlusion, through rtc_scene_set_occlusion; its materials' shadow filters,
 *                        rtch_scene_shadow_filters, through rtc_scene_set_shadow_filters; its materials' absorption
 *                        and its atmosphere, rtch_scene_media, through rtc_scene_set_media; its environment,
 *                        rtch_scene_environment, through rtc_scene_set_environment; its sky light,
 *                        rtch_scene_sky_light, through rtc_scene_set_sky_light; its indirect light,
 *                        rtch_scene_indirect, through rtc_scene_set_indirect; its emitter sampling,
 *                        rtch_scene_emitters, through rtc_scene_set_emitters, and its MIS mode, rtch_scene_emitter_mis,
 *                        through rtc_scene_set_emitter_mis; its denoiser, rtch_scene_denoise,
 *                        through rtc_render_denoised; its film stage, rtch_scene_film, through rtc_render_filmed;
 *                        its robust accumulation, rtch_scene_robust, through rtc_render_robust)
 *
 * Every function that returns int returns 0 on success; otherwise rtch_last_error()
 * holds "<ZigStyleErrorName>: detail" (thread-local).
 */
#ifndef RTC_HOST_H
#define RTC_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "rtc.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *rtch_last_error(void);

/* Parses a scene description; files it names (OBJ meshes, PNG textures) are read from data_dir + name. */
int rtch_scene_load(const char *scene_json, const char *data_dir, void **out_handle);
/* Threads rtch_scene_load may build the scene's objects on: 0 (the default) = what the process may use, at most 16;
 * 1 = one loop over "objects", as scene.zig:650-655.  The description is the same to the bit either way. */
void rtch_set_loader_threads(uint32_t threads);
void rtch_scene_free(void *handle);
/* The flattened World, valid while the handle lives; pass it to rtc_scene_create. */
const rtc_scene_desc *rtch_scene_desc(void *handle);
/* World.lights of both kinds (point and area lights, in order), valid while the handle lives; pass it to
 * rtc_scene_create_with_lights.  The description's light_pos / light_rgb hold every light as a point light - an area
 * light at its centre - so rtc_scene_create alone renders the same world with hard shadows from the centres. */
const rtc_light_desc *rtch_scene_lights(void *handle);
/* The camera's "sampling" of the scene file (anti-aliasing, focal blur), or the defaults - grid 1, no jitter,
 * aperture 0 - when it has none; pass it to rtc_scene_set_sampling.  Camera rotate / move leave it alone. */
int rtch_scene_sampling(void *handle, rtc_sampling *out);
/* The camera's "sampling": {"passes": n} of the scene file (1 when absent): rtch_scene_render renders sample passes
 * 0 .. n-1 (rtc_scene_set_sample_pass), sums them in pass order and divides by n once - the bits of
 * rtc_scene_accumulate_device's mean after n passes. */
int rtch_scene_passes(void *handle, uint32_t *out);
/* The camera's "sampling": {"adaptive": {"threshold": t, "min-passes": m, "tile": n or [w, h]}} of the scene file
 * (adaptive sampling; min-passes 4 and tile 16 when absent, "passes" the maximum): *enabled = 1
 * and the setting, or *enabled = 0 when the file has none.  rtch_scene_render then renders through rtc_render_adaptive. */
int rtch_scene_adaptive(void *handle, int *enabled, rtc_adaptive *out);
/* The camera's "sampling": {"denoise": true | {"radius": R, "patch": F, "strength": k, "cancel": a}} of the scene file
 * (the denoiser; radius 7, patch 2, strength 0.45, cancel 1.0 where absent; false is the same as no
 * key): *enabled = 1 and the setting, or *enabled = 0 and the defaults when the file has none.  The file then has "passes"
 * of 2 or more, or "adaptive".  rtch_scene_render then renders through rtc_render_denoised, with the file's adaptive
 * setting when it has one. */
int rtch_scene_denoise(void *handle, int *enabled, rtc_denoise_setting *out);
/* The camera's "film": true | {"exposure": m | {"stops": s}, "auto-exposure": true | k, "bloom": true | {"radius": R,
 * "sigma": s, "threshold": t, "intensity": i}, "tone-curve": "linear" | "reinhard" | "aces" | "hable", "white": w,
 * "transfer": "linear" | "srgb" | {"gamma": g}} of the scene file (the film stage; exposure 1, no
 * automatic exposure, no bloom, ACES, white 4, sRGB where absent; {"stops": s} is exp2(s), "auto-exposure": true the key 0.18,
 * "bloom": true radius 12, sigma 4, threshold 1, intensity 0.15, and a bloom's sigma without a value its radius / 3; false is the
 * same as no key): *enabled = 1 and the setting, or *enabled = 0 and the defaults when the file has none.  The key needs no
 * "passes".  rtch_scene_render then renders through rtc_render_filmed, with the file's passes, adaptive and denoise settings,
 * and its rgb_out is the film's out: display values, not radiance. */
int rtch_scene_film(void *handle, int *enabled, rtc_film_setting *out);
/* The camera sampling's "robust": true | M | {"buckets": M, "gain": g} of the scene file (robust accumulation, DESIGN.md
 * section 31; buckets 5 and gain 1.0 where absent; false is the same as no key): *enabled = 1 and the setting, or
 * *enabled = 0 and the defaults when the file has none.  The key needs "passes" of M or more and does not go with "adaptive".
 * rtch_scene_render then renders through rtc_render_robust, with the file's passes, denoise and film settings. */
int rtch_scene_robust(void *handle, int *enabled, rtc_robust_setting *out);
/* The top-level objects' "motion" of the scene file (motion blur): out[3 r .. 3 r + 2] = the
 * displacement of root r over the shutter, (0, 0, 0) for a root without one; n must be the description's n_roots.  Pass
 * it to rtc_scene_set_motion.  rtch_scene_render applies it. */
int rtch_scene_motion(void *handle, double *out, uint32_t n);
/* The scene file's "spot-light" entries (spot lights), in World.lights order: cone[i] 1 with the
 * axis ("to" - position, or "direction") and the cosines of the half-angles (std::cos of "inner-angle", "outer-angle"),
 * cone[i] 0 for every other light; n must be the light table's n_lights.  Pass them to rtc_scene_set_spots.
 * rtch_scene_render applies them; rtch_scene_lights reports a spot as the point light it is. */
int rtch_scene_spots(void *handle, uint8_t *cone, double *axis, double *cos_inner, double *cos_outer, uint32_t n);
/* The materials' "normal-perturbation" entries, in mat_* order: {"type": "noise" | "ripples",
 * "amplitude": a >= 0, "octaves": 1 .. RTC_BUMP_MAX_OCTAVES (3), "persistence": p (0.8), "transform": a pattern's list};
 * kind[i] RTC_BUMP_* (RTC_BUMP_NONE for a material without the key), inverse[12 i ..] rows 0..2 of the transform's
 * inverse; n must be the description's n_materials.  A material with the key is a mat_* row of its own.  Pass them to
 * rtc_scene_set_bumps.  rtch_scene_render applies them. */
int rtch_scene_bumps(void *handle, uint8_t *kind, double *amplitude, uint32_t *octaves, double *persistence, double *inverse, uint32_t n);
/* The triangles' texture rows (UV-mapped mesh textures), in tri_* order: out[6 i ..] = (a1, b1, a2,
 * b2, a3, b3), the (u, v) of triangle i's p1, p2, p3 - from a "from-obj" with "texture-coordinates": true (`vt` lines and
 * the faces' t fields) or a "triangle" with "uv1", "uv2", "uv3"; six zeros for every other triangle; n must be the
 * description's n_tris.  Pass them to rtc_scene_set_mesh_uvs.  rtch_scene_render applies them. */
int rtch_scene_mesh_uvs(void *handle, double *out, uint32_t n);
/* The materials' "roughness" (glossy reflection and refraction), in mat_* order: a number (both
 * values) or {"reflection": a, "transmission": b}, each in [0, 1]; and *seed, the camera's "sampling": {"gloss-seed": n}
 * (0 without).  n must be the description's n_materials.  A material with the key is a mat_* row of its own only when a
 * value is non-zero.  *present: 1 when a material of the file has the key.  Pass them to rtc_scene_set_gloss.
 * rtch_scene_render applies them. */
int rtch_scene_gloss(void *handle, double *reflection, double *transmission, uint64_t *seed, int *present, uint32_t n);
/* The materials' "ambient-occlusion" (DESIGN.md section 21), in mat_* order: a number (the radius) or {"radius": r},
 * finite and >= 0; *samples and *seed, the camera's "sampling": {"occlusion-samples": n, "occlusion-seed": s} (1 and 0
 * without).  n must be the description's n_materials.  A material with the key is a mat_* row of its own only when the
 * value is non-zero.  *present: 1 when a material of the file has the key.  Pass them to rtc_scene_set_occlusion.
 * rtch_scene_render applies them. */
int rtch_scene_occlusion(void *handle, double *radius, uint32_t *samples, uint64_t *seed, int *present, uint32_t n);
/* The materials' "shadow-filter" (DESIGN.md section 22), in mat_* order, three doubles a row: a number f - (f, f, f) -, an
 * array [r, g, b], or true - the material's transparency in each channel -, every value finite and in [0, 1].  n must be
 * the description's n_materials; rgb holds 3 * n doubles.  A material with the key is a mat_* row of its own only when a
 * value is non-zero.  *present: 1 when a material of the file has the key.  Pass them to rtc_scene_set_shadow_filters.
 * rtch_scene_render applies them. */
int rtch_scene_shadow_filters(void *handle, double *rgb, int *present, uint32_t n);
/* The materials' "absorption" (DESIGN.md section 23), in mat_* order, three doubles a row: a number a - (a, a, a) -, an
 * array [r, g, b], or {"color": [r, g, b], "distance": d} - white light has that colour after d units: -log(color.c) / d,
 * color.c in (0, 1], d > 0 -, every value finite and >= 0; and the scene's "atmosphere": {"density": d, "color": [r, g, b]}
 * in fog[4]: the density, then the colour (all zero without the key).  n must be the description's n_materials; absorption
 * holds 3 * n doubles.  A material with the key is a mat_* row of its own only when a value is non-zero.  *present: 1 when
 * a material of the file has the key or the file has an atmosphere.  Pass them to rtc_scene_set_media.  rtch_scene_render
 * applies them. */
int rtch_scene_media(void *handle, double *absorption, double *fog, int *present, uint32_t n);
/* The scene's "environment" (DESIGN.md section 24): {"color": [r, g, b], "pattern": {...}, "projection": "sphere" | "cube",
 * "suns": [{"direction": [x, y, z], "intensity": [r, g, b]}, ...]}, every key optional - color defaults to (1, 1, 1) with a
 * pattern and (0, 0, 0) without, projection to "sphere" -, as rtc_scene_set_environment takes it: *out's rgb, pattern (a row
 * of the description's pat_* tables - the environment's rows follow every material's -, or RTC_ENV_NO_PATTERN), projection
 * and n_suns; the suns' rows, as the file has them, go to sun_direction and sun_rgb (room for 3 * RTC_ENV_MAX_SUNS doubles
 * each), which *out then points to.  *present: 1 when the file has the key.  rtch_scene_render applies it. */
int rtch_scene_environment(void *handle, rtc_environment *out, double *sun_direction, double *sun_rgb, int *present);
/* The environment's "light" (DESIGN.md section 25): g, or {"gain": g, "samples": n, "seed": s} - gain defaults to 1.0,
 * samples to 1, seed to 0 -, as rtc_scene_set_sky_light takes it.  *present: 1 when the file has the key; without it *out is
 * gain 0, samples 1, seed 0.  The key adds no table row.  rtch_scene_render applies it. */
int rtch_scene_sky_light(void *handle, rtc_sky_light *out, int *present);
/* The scene's "indirect" (DESIGN.md section 27): g, or {"gain": g, "bounces": n, "seed": s} - gain defaults to 1.0, bounces
 * to 1, seed to 0 -, and the materials' "emission" (e, or [r, g, b]) in mat_* order, as rtc_scene_set_indirect takes them:
 * `emission` has room for 3 * n doubles, n the description's n_materials, and *out points to it.  *present: 1 when the file
 * has either key; without "indirect" *out is gain 0, bounces 0, seed 0.  Neither key adds a table row.  rtch_scene_render
 * applies them. */
int rtch_scene_indirect(void *handle, rtc_indirect *out, double *emission, int *present, uint32_t n);
/* The "emitters" key inside the scene's "indirect" (DESIGN.md section 28): true, n, or {"samples": n, "seed": s} - samples
 * defaults to 1, seed to 0 -, as rtc_scene_set_emitters takes it.  *present: 1 when the file has the key and it is not false;
 * without it *out is samples 1, seed 0.  The key adds no table row.  rtch_scene_render applies it, after the indirect table. */
int rtch_scene_emitters(void *handle, rtc_emitters *out, int *present);
/* The "mis" key inside the object form of the scene's "emitters" (DESIGN.md section 32): true | false, as
 * rtc_scene_set_emitter_mis takes it - *mode is 1 where the file has the key and it is true, else 0 (false: as without the key).
 * The key adds no table row.  rtch_scene_render applies it, after the emitter table. */
int rtch_scene_emitter_mis(void *handle, uint32_t *mode);
int rtch_scene_camera(void *handle, uint32_t width, uint32_t height, rtc_camera *out);
int rtch_camera_rotate(void *handle, double angle);
int rtch_camera_move(void *handle, double distance);
int rtch_camera_make(uint32_t hsize, uint32_t vsize, double fov, const double from[3], const double to[3],
                     const double up[3], rtc_camera *out);
/* Returns the number of bytes the PPM needs; writes at most cap bytes. */
size_t rtch_canvas_ppm(const double *rgb, uint32_t w, uint32_t h, char *buf, size_t cap);
void rtch_canvas_rgba8(const double *rgb, uint32_t w, uint32_t h, uint8_t *out);
int rtch_scene_render(void *handle, uint32_t width, uint32_t height, uint32_t max_depth, double *rgb_out);

#ifdef __cplusplus
}
#endif
#endif /* RTC_HOST_H */
