/*
 * rtc_diag.h - diagnostics and tuning of librtc_hip.so: NOT part of the render path a host binds (that is rtc.h - create /
 * clone / destroy, the render forms, canvas registration, the tile entries, stats, errors; the precedent is the twelve
 * exports of the reference's /root/reference/src/lib.zig:233-309).  The test suite, bench.py and tools/ use these; no
 * rendered value depends on any of them.
 */
#ifndef RTC_DIAG_H
#define RTC_DIAG_H

#include "rtc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Tuning and test options, process-wide; none changes a rendered value.  Read when a scene is created (bvh_*,
 * blocks_per_cu, build_threads) or a launch is enqueued (the rest).  Every option is one atomic number: setting one from
 * a thread while another thread creates scenes or enqueues launches is safe; a launch already enqueued is not affected.  Names: "simple3_min_chunks" (chunks from which a world of
 * top-level spheres / planes / cubes runs the three-waves-per-SIMD kernel; 0 always, < 0 the library's choice),
 * "sched_off" (!= 0: no schedule, packet i is chunk i), "cut_above" (shares of a wave above which a chunk is cut into
 * runs of pixels; < 0 never, 0 the library's choice), "pack_rounds", "pull_min_idle", "blocks_per_cu", "sched_tmin",
 * "bvh_leaf", "bvh_one_axis", "bvh_check", "host_bands" (bands of a host-output frame, 1 .. 4; 0 by size),
 * "waves3" (the general kernel at three waves per SIMD: 1 always, 0 never, < 0 measured per handle),
 * "sched_mix" (a | b << 8: behind every wave's first packet the schedule takes a packets from its long end, then b from
 * its short end, ...; 0 longest first throughout), "measure_every" (a view that moves in small steps is measured
 * every n-th frame; 1), "inflight_chunks_per_wave" (a launch of a scene with several handles - frames in flight -
 * runs on at most one wave per this many chunks; 3, 0 = no cap), "build_threads" (threads rtc_scene_create builds the
 * groups' candidate BVHs with, one top-level group each; 0 = the library's choice, at most 16; the tables do not depend
 * on it), "box_cull" (read at create: a world of top-level spheres / planes / cubes runs the kernels whose root loop
 * rejects by world boxes - 1 - or by bounding spheres - 0; < 0: boxes if it has more cubes than spheres),
 * "containers_own_root" (read at create; 1: a root that is alone - rtc_diag_root_flags - is marked so in the handle's
 * tables and a hit on it takes n1 and n2 from its own entries; 0: no root is marked and every such hit makes the
 * containers pass, so that the two can be held to each other),
 * "sampling_kernels" (!= 0: the camera-sampling kernels even with the default sampling - one centred ray per pixel -, so
 * that their one-sample images can be held to the other kernels'), "motion_kernels" (!= 0: the motion kernels even on a
 * static handle, with every displacement zero, so that their images can be held to the sampling kernels'), "spot_kernels"
 * (!= 0: the spot kernels even on a handle without cones, every flag zero, so that their images can be held to the
 * motion kernels'), "bump_kernels" (!= 0: the bump kernels even on a handle without bumps, every row of kind none, so that
 * their images can be held to the spot kernels'), "torus_kernels" (!= 0: the torus kernels even on a handle without a
 * torus, so that their images can be held to the bump kernels'), "meshuv_kernels" (!= 0: the meshuv kernels even on a
 * handle without a texture map of mapping RTC_TEX_MESH, so that their images can be held to the handle's ordinary kernels'),
 * "gloss_kernels" (!= 0: the gloss kernels even on a handle without a rough material, every roughness row zero, so that
 * their images can be held to the handle's ordinary kernels'), "occlusion_kernels" (!= 0: the occlusion kernels even on a
 * handle without an occlusion radius, every radius row zero, so that their images can be held to the handle's ordinary
 * kernels'), "shadow_filter_kernels" (!= 0: the shadow-filter kernels even on a handle without a filter, every filter row
 * zero, so that their images can be held to the handle's ordinary kernels'), "media_kernels" (!= 0: the media kernels even
 * on a handle without media, every absorption row and the fog density zero, so that their images can be held to the
 * handle's ordinary kernels'), "environment_kernels" (!= 0: the environment kernels even on a handle without an environment,
 * no sky and no sun, so that their images can be held to the handle's ordinary kernels'), "sky_light_kernels" (!= 0: the
 * sky-light kernels even on a handle without a sky light, the gain zero, so that their images can be held to the handle's
 * ordinary kernels'), "indirect_kernels" (!= 0: the indirect kernels even on a handle without an indirect table, the gain
 * zero and no emission, so that their images can be held to the handle's ordinary kernels'), "emitter_kernels" (!= 0: the
 * emitter kernels even on a handle without an emitter list, the count zero, so that their images can be held to the handle's
 * ordinary kernels'), "mis_kernels" (!= 0: the MIS kernels even on a handle whose MIS mode is 0 or whose emitter list is
 * empty, the mode zero, so that their images can be held to the handle's ordinary kernels'), "denoise_naive" (!= 0: rtc_denoise_device runs rtc_denoise_naive_kernel, the literal form of rtc.h's
 * loops with one thread per pixel, in place of the tiled kernels, so that the two can be held to each other and timed
 * against each other; the bits are the same), "film_naive" (!= 0: a rtc_film_device that blooms runs rtc_film_naive_row_kernel
 * and rtc_film_naive_resolve_kernel, the literal forms of rtc.h's loops with one thread per pixel and no LDS, in place of the
 * tiled kernels, for the same two purposes; the bits are the same), "robust_naive" (!= 0: rtc_robust_device runs
 * rtc_robust_naive_kernel, the literal form of rtc.h's loops with one thread per pixel, the bucket count a run-time value and
 * every bucket mean formed again wherever it is used, in place of the register forms, for the same two purposes; the bits
 * are the same).
 * RTC_ERR_INVALID_ARGUMENT for a name the library does not know.
 * (The library reads no environment variables.)
 */
int rtc_set_option(const char *name, double value);

/* Diagnostic: the name of the render kernel the last launch on this handle ran
 * (the name rocprofv3 shows - which variant is picked depends on what the world
 * contains and on the size of the launch); "" before the first launch.  Static storage.
 * (After an rtc_render that went to the host in bands, this, rtc_get_schedule and
 * rtc_get_tile_costs describe the frame's first band; rtc_get_stats the whole frame.) */
const char *rtc_last_kernel_name(const rtc_scene *scene);

/* Diagnostic: the schedule the NEXT launch of the handle's current pixel map would run - the order in which the
 * persistent waves are handed pixels (results never depend on it) - as `*n_packets` rows of 16 items; an item is
 * chunk | first_pixel << 20 | (pixels - 1) << 26 (pixels of an 8x8 chunk in row-major order), 0xFFFFFFFF = none.
 * Synchronises.  `*n_packets` = 0 when the handle has no schedule (no launch yet, or a launch of fewer than 64 chunks).
 * RTC_ERR_INVALID_ARGUMENT if `capacity_items` is too small (`*n_packets` says how many rows there are). */
int rtc_get_schedule(rtc_scene *scene, uint32_t *items, size_t capacity_items, uint32_t *n_packets);

/* Diagnostic (tools/estimate_probe.py): for the pixel map of the handle's last scheduled launch, per 8x8 chunk what the
 * first-frame estimate (rtc_estimate_kernel, for camera `cam`) says it costs and what the last measuring launch measured,
 * both in the packer's ticks of 16 shader cycles.  Either array may be NULL.  Scheduling only: no result depends on it. */
int rtc_get_chunk_times(rtc_scene *scene, const rtc_camera *cam, uint32_t *estimated, uint32_t *measured, size_t capacity,
                        uint32_t *n_chunks);

/* Diagnostic (tests/test_build_threads_cpu.py, tools/): the HOST half of rtc_scene_create by itself - validation and the
 * device tables (depth-first leaf order, bounding spheres, the candidate BVHs and their eight-wide form) - without a
 * device: `*digest` = a 64-bit FNV-1a hash over the tables the kernel walks (eight-wide nodes, leaf list, root records,
 * bounding spheres, reference-tree parents), `*build_ms` = the wall time of the table build.  Either may be NULL.  What
 * "build_threads" must not change. */
int rtc_diag_build_tables(const rtc_scene_desc *desc, uint64_t *digest, double *build_ms);

/* Diagnostic (tests/test_emitters_cpu.py): the emitter list rtc_scene_set_emitters derives (rtc.h) for
 * a description, an emission table `emission` ([n_materials][3], as rtc_indirect's; NULL: no material emits) and a filter
 * table `filter` ([n_materials][3], as rtc_shadow_filters'; NULL: no table), without a device: `rows[18 k ...]` = origin,
 * eu, ev, the unit normal, the emission, W / (E.r + E.g + E.b), 1.0 for a triangle, the depth-first leaf; `cdf[k]` the
 * running sum of the weights; `*count` the entries.  Either array may be NULL (then only *count).
 * RTC_ERR_UNSUPPORTED for more than RTC_MAX_EMITTERS entries. */
int rtc_diag_emitters(const rtc_scene_desc *desc, const double *emission, const double *filter, uint32_t capacity, double *rows,
                      double *cdf, uint32_t *count);
/* Diagnostic: the entry the kernels' search picks for the draw u0 from a CDF of `count` >= 1 entries, W = cdf[count - 1]. */
int rtc_diag_emitter_pick(const double *cdf, uint32_t count, double u0, uint32_t *entry);
/* Diagnostic (tests/test_mis_cpu.py): the two weights of rtc_scene_set_emitter_mis' balance heuristic (rtc.h, DESIGN.md section
 * 32) for one direction, on the host with the kernels' own expression: `samples` = n (1 .. RTC_EMITTER_MAX_SAMPLES), `q` the
 * entry's W / (E.r + E.g + E.b), `cos_s` the cosine at the shaded point (cos_x of a sample, cos_b of a child), `cos_e` the
 * cosine at the emitter (its absolute value already taken), `r` the distance.  Where a skip rule holds - cos_s <= 0,
 * cos_e == 0 or r <= 2e-4 - *w_e = 0 and *w_b = 1; else *w_e = b / (b + a) and *w_b = a / (b + a), a = q * (cos_s * cos_e),
 * b = n * (RTC_PI * (r * r)).  RTC_ERR_INVALID_ARGUMENT for a NULL pointer or `samples` outside its range. */
int rtc_diag_mis_weights(uint32_t samples, double q, double cos_s, double cos_e, double r, double *w_e, double *w_b);

/* Diagnostic (tests/test_root_boxes_cpu.py): the FP32 world boxes phase 1 of the render kernels' root loop tests
 * (DESIGN.md section 3), as rtc_scene_create builds them, without a device: per table position i (the tables are sorted
 * by kind) `boxes[7 i ...]` = lo x y z, hi x y z, line_only (no finite bound: -3e38 / +3e38), `world_index[i]` = the
 * World.objects entry it belongs to, `scales` = {largest |coordinate| of a finite box, the "parallel rule" factor}:
 * what the test needs to replay the kernel's arithmetic on the host.  Either array may be NULL (then only *n_roots). */
int rtc_diag_root_boxes(const rtc_scene_desc *desc, float *boxes, uint32_t *world_index, uint32_t capacity, uint32_t *n_roots,
                        float *scales);

/* Diagnostic (tests/test_containers_cpu.py): the FP32 bounding spheres phase 1 tests in the simple kernels that cull by
 * spheres, in the same table order as rtc_diag_root_boxes (its `world_index`): `spheres[4 i ...]` = centre x y z, radius
 * squared (no finite bound: +inf), `*cmax` = the largest |centre| of a bounded root (the scale of the kernel's rounding
 * margin).  `spheres` may be NULL (then only *n_roots and *cmax). */
int rtc_diag_root_spheres(const rtc_scene_desc *desc, float *spheres, uint32_t capacity, uint32_t *n_roots, float *cmax);

/* Diagnostic (tests/test_own_root_cpu.py): the `kind_flags` word of every root record as rtc_scene_create builds it,
 * without a device, in the table order of rtc_diag_root_boxes (its `world_index`): the leaf kind in bits 0-7, casts a
 * shadow 0x100, a closed cylinder or cone 0x200, a room 0x400, alone 0x800 (RTC_ROOT_ALONE_FLAG: a top-level sphere or
 * cube of a world of spheres, planes and cubes that no other root can share a containers list with),
 * a csg 0x4000, a group 0x8000.  Option "containers_own_root" is not applied: at 0 a handle's tables are left without
 * bit 0x800, at create.  (rtc_diag_build_tables digests the tables before that bit is set.)  `flags` may be NULL (then
 * only *n_roots). */
#define RTC_ROOT_ALONE_FLAG 0x800u
int rtc_diag_root_flags(const rtc_scene_desc *desc, uint32_t *flags, uint32_t capacity, uint32_t *n_roots);

/* Diagnostic (tests/test_denoise_gpu.py): the output tile of the tiled denoise kernels, so that tests
 * can name image sizes relative to it.  No device needed. */
int rtc_diag_denoise_tile(uint32_t *w, uint32_t *h);

/* Diagnostic (tests/test_film_gpu.py): the extents of the tiled film kernels' output tiles - the row
 * kernel's width, the resolve kernel's width and height - so that tests can name image sizes relative to them.  No device
 * needed. */
int rtc_diag_film_tile(uint32_t *row_w, uint32_t *col_w, uint32_t *col_h);

/* Diagnostic (tests/test_robust_gpu.py): the cap of rtc_robust_device's grid in blocks and the threads of a block (DESIGN.md
 * section 31), so that tests can name a pixel count above what one sweep of the grid covers.  No device needed. */
int rtc_diag_robust_grid(uint32_t *max_blocks, uint32_t *block);

#ifdef __cplusplus
}
#endif
#endif /* RTC_DIAG_H */
