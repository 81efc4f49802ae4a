/*
 * rtc.h — C ABI of the MI355X render path (librtc_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of SinclaM/ray-tracer-challenge:
 *
 *     Camera(T).render(self, allocator, world) !Canvas(T)      src/raytracer/camera.zig:80-125
 *       -> rayForPixel                                         src/raytracer/camera.zig:64-76
 *       -> World.colorAt(ray, 5)                               src/raytracer/world.zig:111-121
 *            intersect / shadeHit / isShadowed /
 *            reflectedColor / refractedColor                   src/raytracer/world.zig:71-189
 *
 * The reference has no FFI for this path (it is pure Zig); the only C-ABI
 * precedent is the WASM export table src/lib.zig:233-309 (global renderer,
 * error returned as a NUL-terminated error *name*).  A Zig host binds the
 * functions below with `extern fn` declarations and calls
 * them from the body of Camera.render; the JSON scene loader and the
 * canvas/PPM writer stay untouched.
 *
 * Conventions
 *   - all reals are IEEE binary64 (the reference renders scenes in f64:
 *     src/main.zig:71, src/lib.zig:194,223);
 *   - matrices are row-major 4x4 (src/raytracer/matrix.zig:15), 16 doubles;
 *   - all input arrays are caller-owned and are copied by rtc_scene_create();
 *     the library never retains a host pointer;
 *   - every function returns an rtc_status; the message/name of the last
 *     failure on the calling thread is available from rtc_last_error();
 *   - a handle may be used from one thread at a time; distinct handles are
 *     independent;
 *   - renders on ONE handle run one after the other, whatever streams they are
 *     enqueued on: a handle owns one set of counters, work counter and per-lane
 *     scratch, so every launch records an event and a launch on a different
 *     stream makes that stream wait for it first (no host synchronisation).
 *     Two handles on two streams overlap freely.
 *
 * Limits (a scene beyond them is refused or reported, never rendered differently):
 *   - more than 8 gradient / radial-gradient / blend patterns nested inside one
 *     another: rtc_scene_create returns RTC_ERR_UNSUPPORTED;
 *   - pattern select-chains (stripes / checkers / rings / perturb / texture map)
 *     deeper than 64: RTC_ERR_UNSUPPORTED at create;
 *   - more than 64 csg nodes under one csg: RTC_ERR_UNSUPPORTED at create;
 *   - a lane's list of the intersections of one ray with one csg unit (the list
 *     Csg.filterIntersections works on, csg.zig:51-95) starts with 32 slots: when a
 *     frame needs more, the frame itself says how many (the longest list any lane
 *     wanted): rtc_render / rtc_render_rgba8 size the lists for that and render
 *     again (up to 1024; the handle keeps the longer lists), while the asynchronous
 *     entry points count the lanes that ran out in rtc_stats::overflow - callers
 *     check rtc_get_stats and call rtc_grow_csg_lists, then render the frame again
 *     (rtc_multi.h does that for its handles); beyond 1024 entries, or a group tree
 *     deeper than the traversal stack: RTC_ERR_OVERFLOW, never a truncated image;
 *   - two leaves with the same Shape.id: RTC_ERR_UNSUPPORTED (identity in the
 *     containers walk is the leaf);
 *   - reproducibility: geometry and every branch are bit-identical from run to
 *     run; the colour of a pixel whose ray tree was shared between lanes is the
 *     sum of the lanes' shares in completion order (f64 atomic adds), so two
 *     renders of one frame agree to ~1e-15, not bitwise.  A pixel whose tree
 *     stayed in one lane (every pixel of a scene without transparent
 *     reflective materials) is bitwise reproducible.
 */
#ifndef RTC_H
#define RTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTC_ABI_VERSION 3u

/* ---- status codes; names mirror the reference's Zig error names where one exists ---- */
typedef enum rtc_status {
  RTC_OK = 0,
  RTC_ERR_INVALID_ARGUMENT = 1, /* null pointer, zero-sized image, tile out of range ...           */
  RTC_ERR_OUT_OF_MEMORY = 2,    /* Zig: error.OutOfMemory -> @panic in camera.zig:118               */
  RTC_ERR_NOT_INVERTIBLE = 3,   /* Zig: MatrixError.NotInvertible, matrix.zig:7                     */
  RTC_ERR_UNSUPPORTED = 4,      /* a shape/pattern kind this build of the kernel does not implement */
  RTC_ERR_BAD_INDEX = 5,        /* an index array points outside its table                          */
  RTC_ERR_NO_DEVICE = 6,        /* no HIP device / HIP runtime failure; message carries hipError    */
  RTC_ERR_NOT_AFFINE = 7,       /* a shape/pattern inverse whose last row is not (0,0,0,1)          */
  RTC_ERR_OVERFLOW = 8          /* a per-lane device stack or csg intersection list overflowed        */
} rtc_status;

/* ---- leaf kinds: the Shape(T).Variant tags that can be hit (shape.zig:99-111) ---- */
enum {
  RTC_SPHERE = 0,          /* shapes/sphere.zig   */
  RTC_PLANE = 1,           /* shapes/plane.zig    */
  RTC_CUBE = 2,            /* shapes/cube.zig     */
  RTC_CYLINDER = 3,        /* shapes/cylinder.zig */
  RTC_TRIANGLE = 4,        /* shapes/triangle.zig:17-81   */
  RTC_SMOOTH_TRIANGLE = 5, /* shapes/triangle.zig:210-274 */
  RTC_CONE = 6,            /* shapes/cone.zig; geometry in the cyl_* tables like a cylinder */
  RTC_TORUS = 7            /* a ring torus (below); its two radii in the cyl_* tables */
};

/*
 * RTC_TORUS - the book's last shape.  In object space the torus lies in the xz plane around the y axis:
 *
 *     (x^2 + y^2 + z^2 + R^2 - r^2)^2 = 4 R^2 (x^2 + z^2)        0 < r < R, both finite
 *
 * leaf_geom indexes the cyl_* tables: cyl_min = R (major radius), cyl_max = r (minor radius), cyl_closed is ignored.
 * rtc_scene_create refuses a leaf_geom out of range (RTC_ERR_BAD_INDEX) and radii that are not finite or not
 * 0 < r < R (RTC_ERR_INVALID_ARGUMENT).  Every operation below is an IEEE double operation, correctly rounded, in the
 * order and with the parentheses written; only + - * / sqrt fabs and comparisons occur.
 *
 * localIntersect of the ray (o, d) emits up to four entries (t, 0, 0), t strictly ascending:
 *   1. alpha = (dx dx + dy dy) + dz dz;   t0 = -((ox dx + oy dy) + oz dz) / alpha;   p = o + t0 d  (px = ox + t0 dx, ...)
 *   2. bxz = (R + r) (1 + 1e-9), by = r (1 + 1e-9): the line against the box (-bxz, -by, -bxz) .. (bxz, by, bxz) with
 *      Cube.localIntersect's arithmetic (checkAxis per axis on (o, d) with these bounds - |direction| < 1e-5 is
 *      "parallel": numerator * infinity -, tmin = max of the three, tmax = min of the three, NaN operands ignored).
 *      tmin > tmax: no entries.  Otherwise lo = tmin - t0, hi = tmax - t0; unless lo < hi and hi - lo is finite: no entries.
 *      The box is part of the contract: a line that misses it has no entries, and no entry lies outside it.
 *   3. beta = 2 ((px dx + py dy) + pz dz);   gamma = (((px px + py py) + pz pz) + R R) - r r;   f = 4 (R R)
 *      c4 = alpha alpha                       c3 = (2 alpha) beta
 *      c2 = (beta beta + (2 alpha) gamma) - f (dx dx + dz dz)
 *      c1 = (2 beta) gamma - (2 f) (px dx + pz dz)
 *      c0 = gamma gamma - f (px px + pz pz)          q(s) = c4 s^4 + c3 s^3 + c2 s^2 + c1 s + c0,  s = t - t0
 *   4. A polynomial (a4 .. a0) is evaluated as P(x) = (((a4 x + a3) x + a2) x + a1) x + a0, its derivative
 *      (b3 .. b0) = (4 a4, 3 a3, 2 a2, a1) as D(x) = ((b3 x + b2) x + b1) x + b0.  The cubic q' is the polynomial
 *      (0, 4 c4, 3 c3, 2 c2, c1).  Its critical points: with (q0, q1, q2) = (3 (4 c4), 2 (3 c3), 2 c2) and
 *      disc = q1 q1 - (4 q0) q2, none if not disc >= 0, else (-q1 - sqrt(disc)) / (2 q0) and (-q1 + sqrt(disc)) / (2 q0),
 *      the smaller first.
 *      scan(P, points, cap): a = lo, fa = P(lo); for every point b in turn, then for hi - a point is skipped unless
 *      a < b < hi -: fb = P(b); if fa == 0 then emit a, else if (fa < 0) != (fb < 0) and fb != 0 then emit refine(a, b);
 *      a = b, fa = fb.  After hi: if fa == 0 emit a.  emit(x) appends x unless the list holds cap roots or x is not above
 *      the last one.
 *      refine(l, h), with fa of the piece's lower end: x = (l + h) / 2; at most 80 times: fx = P(x); fx == 0 ends; if
 *      (fx < 0) == (fa < 0) then l = x else h = x; d = D(x); xn = x - fx / d (l if d == 0); unless l < xn < h,
 *      xn = (l + h) / 2; m = (l + h) / 2; stop = xn == x or not l < h or m == l or m == h; x = xn; stop ends.  The root is x.
 *      The roots of q' are scan(q', the critical points, 3); the roots of q are scan(q, the roots of q', 4).
 *   5. t = t0 + s for each root s.
 *
 * localNormalAt(p): rho = sqrt(px px + pz pz);  n = (px - R (px / rho), py, pz - R (pz / rho)), and (0, py, 0) if rho == 0.
 */

/* ---- pattern kinds: Pattern(T).Variant tags (patterns/pattern.zig:34-45) ---- */
enum {
  RTC_PAT_SOLID = 0,           /* patterns/solid.zig    */
  RTC_PAT_STRIPES = 1,         /* patterns/stripes.zig  */
  RTC_PAT_RINGS = 2,           /* patterns/rings.zig    */
  RTC_PAT_GRADIENT = 3,        /* patterns/gradient.zig */
  RTC_PAT_RADIAL_GRADIENT = 4, /* patterns/gradient.zig */
  RTC_PAT_CHECKERS = 5,        /* patterns/checkers.zig */
  RTC_PAT_BLEND = 6,           /* patterns/blend.zig    */
  RTC_PAT_PERTURB = 7,         /* patterns/perturb.zig: pat_a = the perturbed pattern, pat_rgb = PerturbInfo
                                  {scale_value, octaves, persistence} (defaults 0.3, 3, 0.8) */
  RTC_PAT_TEXTURE_MAP = 8,     /* patterns/texture_map.zig: pat_a = index into the tex_* tables */
  RTC_PAT_TEST = 9             /* TestPattern, pattern.zig:136-150: colour = pattern-space point */
};

/* rtc_scene_desc::tex_mapping: TextureMap variants (texture_map.zig:173-305) */
#define RTC_TEX_SPHERICAL 0u
#define RTC_TEX_PLANAR 1u
#define RTC_TEX_CYLINDRICAL 2u
#define RTC_TEX_CUBIC 3u
#define RTC_TEX_MESH 4u /* not in the reference: (u, v) from the hit triangle's texture row, see rtc_scene_set_mesh_uvs */
/* rtc_scene_desc::uv_kind: UvPattern variants (texture_map.zig:9-121) */
#define RTC_UV_ALIGN_CHECK 0u /* uv_sub = central, upper-left, upper-right, bottom-left, bottom-right */
#define RTC_UV_CHECKERS 1u    /* uv_size = width, height; uv_sub[0..1] = a, b                        */
#define RTC_UV_IMAGE 2u       /* uv_image = image index, uv_interp = 0 none / 1 bilinear             */
#define RTC_UV_TEST 3u        /* UvTestPattern: colour = (u, v, 0)                                   */

/* rtc_scene_desc::node_op (shapes/csg.zig:16-20) */
#define RTC_CSG_NONE 0u
#define RTC_CSG_UNION 1u
#define RTC_CSG_INTERSECTION 2u
#define RTC_CSG_DIFFERENCE 3u

/* Children / roots are encoded as one u32: high bit set = group node index, else leaf index. */
#define RTC_CHILD_NODE_BIT 0x80000000u

/* Number of doubles per material row: ambient, diffuse, specular, shininess,
 * reflective, transparency, refractive_index (material.zig:18-25).              */
#define RTC_MAT_STRIDE 7

/*
 * Flattened World(T) (world.zig:24-25): SoA tables, caller-owned.
 *
 * Leaves are the hit-able Shapes; `leaf_*` arrays are indexed by leaf.  The
 * order in which leaves are reached by a depth-first walk of roots[] /
 * children[] is the order the reference's nested stable sorts preserve for
 * equal-t intersections (world.zig:81, group.zig:59) and is used as the
 * tie-break; the leaf arrays themselves may be in any order.
 *
 * Groups store no transform of their own (shape.zig:286-296): every leaf holds
 * the full world<->object matrices, so only the inverse and its transpose are
 * needed on the path (shape.zig:133-145, 313-318).  Transforms are a table so
 * that the thousands of triangles of one OBJ instance share one entry.
 */
typedef struct rtc_scene_desc {
  uint32_t abi_version;      /* RTC_ABI_VERSION */

  uint32_t n_xforms;
  const double *xf_inv;      /* [n_xforms][16]  Shape._inverse_transform           */
  const double *xf_inv_t;    /* [n_xforms][16]  Shape._inverse_transform_transpose */

  uint32_t n_leaves;
  const uint8_t *leaf_kind;      /* RTC_SPHERE ...                                        */
  const uint32_t *leaf_xform;    /* index into xf_*                                       */
  const uint32_t *leaf_material; /* index into mat_*                                      */
  const uint8_t *leaf_shadow;    /* Shape.casts_shadow (shape.zig:119)                    */
  const uint32_t *leaf_id;       /* Shape.id (shape.zig:113): containers walk identity    */
  const uint32_t *leaf_geom;     /* cylinder/cone: index into cyl_*; triangles: into tri_* */

  uint32_t n_cyls;               /* cylinder.zig:26-28 (also cones) */
  const double *cyl_min;
  const double *cyl_max;
  const uint8_t *cyl_closed;

  uint32_t n_tris;               /* triangle.zig:21-26, 214-221 */
  const double *tri_p1;          /* [n_tris][3] */
  const double *tri_e1;          /* [n_tris][3] p2 - p1 */
  const double *tri_e2;          /* [n_tris][3] p3 - p1 */
  const double *tri_n1;          /* [n_tris][3] smooth: n1; flat: the stored face normal (shape.zig:190) */
  const double *tri_n2;          /* [n_tris][3] smooth only */
  const double *tri_n3;          /* [n_tris][3] smooth only */

  uint32_t n_materials;
  const double *mat_params;      /* [n_materials][RTC_MAT_STRIDE] */
  const uint32_t *mat_pattern;   /* index into pat_*              */

  uint32_t n_patterns;
  const uint8_t *pat_kind;       /* RTC_PAT_*                                              */
  const double *pat_inv;         /* [n_patterns][16] Pattern._inverse_transform            */
  const double *pat_rgb;         /* [n_patterns][3]  solid colour                          */
  const uint32_t *pat_a;         /* sub-pattern a (stripes/checkers/...), else 0           */
  const uint32_t *pat_b;         /* sub-pattern b                                          */

  uint32_t n_nodes;              /* one node per reference Group (group.zig:17-23)         */
  const double *node_min;        /* [n_nodes][3] Group._bbox min (bounding_box.zig:21)     */
  const double *node_max;        /* [n_nodes][3]                                           */
  const uint32_t *node_first;    /* first entry of this group's children in children[]     */
  const uint32_t *node_count;    /* Group.children.items.len; exactly 2 for a csg node     */
  const uint8_t *node_op;        /* [n_nodes] RTC_CSG_NONE for a Group, else the Csg.operation
                                    (csg.zig:16-20): children[first] is `left`, [first+1] `right`,
                                    node_min/max the csg's _bbox (shape.zig:257-261)          */
  uint32_t n_children;
  const uint32_t *children;      /* mixed list, RTC_CHILD_NODE_BIT marks a sub-group       */

  uint32_t n_roots;              /* World.objects (world.zig:24), in order                 */
  const uint32_t *roots;         /* same encoding as children[]                            */

  uint32_t n_lights;             /* World.lights (world.zig:25), point lights (light.zig)  */
  const double *light_pos;       /* [n_lights][3] */
  const double *light_rgb;       /* [n_lights][3] */

  /* Texture maps (patterns/texture_map.zig); all counts may be 0 and the pointers NULL.    */
  uint32_t n_texmaps;            /* a pattern of kind RTC_PAT_TEXTURE_MAP names one by pat_a */
  const uint8_t *tex_mapping;    /* RTC_TEX_*                                              */
  const uint32_t *tex_uv;        /* [n_texmaps][6] uv-pattern per face, Cubic.Face order front, back, left,
                                    right, up, down (texture_map.zig:216); other mappings use entry 0 */
  uint32_t n_uvs;
  const uint8_t *uv_kind;        /* RTC_UV_*                                               */
  const double *uv_size;         /* [n_uvs][2] UvCheckers width, height                    */
  const uint32_t *uv_sub;        /* [n_uvs][5] pattern indices (see RTC_UV_*)              */
  const uint32_t *uv_image;      /* [n_uvs] image index (RTC_UV_IMAGE)                     */
  const uint8_t *uv_interp;      /* [n_uvs] UvImage.Interpolation: 0 None, 1 Bilinear      */
  uint32_t n_images;             /* Canvas(T) behind a UvImage (canvas.zig:34-46)          */
  const uint32_t *img_width;
  const uint32_t *img_height;
  const uint64_t *img_offset;    /* first pixel of the image in img_rgb                    */
  const float *img_rgb;          /* [pixels][3], row-major: the f32 colour zigimg's iterator yields, which
                                    canvas.zig:41 widens to T                               */
} rtc_scene_desc;

/* Camera(T) after Camera.new + setTransform (camera.zig:18-61). */
typedef struct rtc_camera {
  uint32_t hsize, vsize;
  double half_width, half_height, pixel_size; /* camera.zig:33-52 */
  double inv_view[16];                        /* Camera._inverse_transform */
} rtc_camera;

/* Ray counters of the most recent render on a handle ("ray" = one World.intersect call). */
typedef struct rtc_stats {
  uint64_t primary;       /* camera.zig:117-118: one per pixel                                  */
  uint64_t secondary;     /* reflectedColor + refractedColor calls that recurse (world.zig:164,186) */
  uint64_t shadow_calls;  /* isShadowed calls the reference makes (world.zig:92); a spot light makes no isShadowed call at a point outside its cone */
  uint64_t shadow_traced; /* shadow rays this library actually traced (skips provably inert ones) */
  uint64_t overflow;      /* lanes that overflowed a stack / csg list (must be 0)                */
} rtc_stats;

typedef struct rtc_scene rtc_scene; /* opaque; owns the device copies and one HIP stream */

/* Validates `desc`, copies it into HBM on the current HIP device. */
int rtc_scene_create(const rtc_scene_desc *desc, rtc_scene **out);

/* ---- area lights (the book's bonus chapter "Rendering soft shadows") ---- */
#define RTC_LIGHT_POINT 0u
#define RTC_LIGHT_AREA 1u
#define RTC_AREA_MAX_SAMPLES 4096u /* usteps * vsteps of one area light */

/*
 * World.lights of both kinds, in order (SoA, caller-owned, copied).  A point light is `corner` and `rgb`; an area
 * light is area_light(corner, uvec, usteps, vvec, vsteps, rgb, jitter) with uvec / vvec its FULL edges: its samples are
 *   point_on_light(u, v) = (corner + (uvec / usteps) * (u + ju)) + (vvec / vsteps) * (v + jv),
 * v outer, u inner, ju = jv = 0.5 without jitter, and its lighting is
 *   ambient + (sum over samples of the diffuse + specular terms / samples) * (unshadowed samples / samples).
 * With jitter, ju / jv are a pure function of (seed, whole-image pixel, light, sample, axis) - DESIGN.md section 11 -
 * so an image does not depend on how it was split into bands, tiles or launches.
 */
typedef struct rtc_light_desc {
  uint32_t n_lights;
  const uint8_t *kind;       /* RTC_LIGHT_*                                        */
  const double *corner;      /* [n_lights][3] an area light's corner; a point light's position */
  const double *uvec;        /* [n_lights][3] full edge (area lights only)         */
  const double *vvec;        /* [n_lights][3]                                      */
  const uint32_t *usteps;    /* [n_lights] >= 1 (area lights only)                 */
  const uint32_t *vsteps;    /* [n_lights] >= 1; usteps * vsteps <= RTC_AREA_MAX_SAMPLES */
  const uint8_t *jitter;     /* [n_lights] 0 / 1 (area lights only)                */
  const double *rgb;         /* [n_lights][3] intensity                            */
} rtc_light_desc;

/*
 * rtc_scene_create with World.lights given by `lights` (which replaces desc's light_pos / light_rgb; NULL: exactly
 * rtc_scene_create).  Validated before anything touches the device (kinds, steps, the sample cap, finite values).
 * A table of point lights only renders what rtc_scene_create renders, with the same kernel.
 */
int rtc_scene_create_with_lights(const rtc_scene_desc *desc, const rtc_light_desc *lights, rtc_scene **out);
/* The seed of the area lights' jitter on this handle (default 0; a clone starts with its source's). */
int rtc_scene_set_light_seed(rtc_scene *scene, uint64_t seed);

/* ---- camera samples per pixel: anti-aliasing and focal blur ---- */
#define RTC_SAMPLING_MAX_GRID 16u

/*
 * grid x grid samples per pixel, sample k = j * grid + i (j outer).  Sample k of pixel (x, y) goes through
 *   world_x = half_width - (x + (i + jx) / grid) * pixel_size,  world_y = half_height - (y + (j + jy) / grid) * pixel_size,
 * jx = jy = 0.5 without jitter.  aperture == 0: a pinhole, the ray of Camera.rayForPixel through that point (grid 1
 * without jitter is rayForPixel to the bit).  aperture > 0: a lens of that radius in camera units, the ray from a point
 * of the lens disc through (world_x, world_y, -1) * focal_distance; the lens is always jittered.  The pixel is the
 * mean of its samples' colours.  The jitter is a pure function of (seed, whole-image pixel, sample, axis), so an image
 * does not depend on how it was split into bands, tiles or launches; an area light's jitter is keyed on
 * pixel * samples + k.  rtc_stats.primary counts every sample.
 */
typedef struct rtc_sampling {
  uint32_t grid;          /* 1 .. RTC_SAMPLING_MAX_GRID                       */
  uint32_t jitter;        /* 0 / 1: the sub-pixel offsets jittered            */
  double aperture;        /* lens radius, finite, >= 0 (0: a pinhole)         */
  double focal_distance;  /* finite, > 0 when aperture > 0 (else ignored)     */
  uint64_t seed;
} rtc_sampling;

/*
 * This handle's sampling for every render entry point (rtc_render, _rgba8, _device, _tiles_device,
 * _tile_list_device; NULL: the default, grid 1, no jitter, aperture 0).  Validated before anything changes:
 * RTC_ERR_INVALID_ARGUMENT otherwise.  A clone starts with its source's setting; rtc_render's band clones follow.
 */
int rtc_scene_set_sampling(rtc_scene *scene, const rtc_sampling *sampling);

/* ---- progressive rendering: sample passes accumulated on the device ---- */
/* (pass + 1) * grid * grid may not exceed this: the camera hash holds a 24-bit global sample index. */
#define RTC_SAMPLING_INDEX_LIMIT 16777216u

/*
 * The sample pass this handle renders (default 0; a clone starts with its source's, rtc_render's band clones follow).
 * With S = grid * grid and N = hsize * vsize, pass P renders sample k of pixel p with the camera hash keyed on the
 * global sample index P * S + k (the sub-pixel stratum is still that of k) and an area light's jitter keyed on
 * (P * N + p) * S + k (u64, wrapping).  Pass 0 is the image of every earlier release.  A pass other than 0 always runs
 * the sampling kernels; under the default sampling (one centred ray, no lens) every pass renders the same image unless
 * the scene has a jittered area light.  RTC_ERR_INVALID_ARGUMENT, with nothing changed, unless
 * (pass + 1) * S <= RTC_SAMPLING_INDEX_LIMIT; rtc_scene_set_sampling refuses a grid that breaks it at the current pass.
 */
int rtc_scene_set_sample_pass(rtc_scene *scene, uint32_t pass);

/*
 * One pass into running sums on the device: sum += frame (passes == 1: sum = frame, nothing is read), sumsq += r^2 + g^2 + b^2,
 * and from the new sums, optionally, mean = sum / passes, rgba = the clamp of mean (the bits of rtc_rgba8_device(mean))
 * and noise = sqrt((1/n) * sum over pixels of max(0, sumsq - passes * |mean|^2) / (3 * (passes - 1) * passes)), the
 * RMS standard error of the running mean.  Plain adds and one correctly rounded divide: after P passes `sum` is the
 * in-order sum of the P frames to the bit; the noise is reduced in a fixed order (the same inputs give the same bits).
 * n_pixels is only a length: a rank accumulates its own tiles the same way.
 */
typedef struct rtc_accum {
  const double *frame;  /* [n][3], required: the pass just rendered                         */
  size_t n_pixels;      /* n >= 1                                                           */
  uint32_t passes;      /* passes in the sums after this call, >= 1 (1: overwrite)          */
  double *sum;          /* [n][3], required                                                 */
  double *sumsq;        /* [n] or NULL                                                      */
  double *mean;         /* [n][3] or NULL                                                   */
  uint32_t *rgba;       /* [n] or NULL                                                      */
  double *noise;        /* one device double or NULL; needs sumsq and passes >= 2           */
} rtc_accum;

/*
 * Enqueues the accumulation on `hip_stream` (NULL: the handle's own stream), ordered after the handle's renders on any
 * stream; every pointer is device memory on the handle's device.  Arguments are checked before the device is touched:
 * RTC_ERR_INVALID_ARGUMENT otherwise.
 */
int rtc_scene_accumulate_device(rtc_scene *scene, const rtc_accum *accum, void *hip_stream);

/* ---- motion blur: top-level objects that move while the shutter is open ---- */
/*
 * Root r (World.objects entry r, the scene description's roots[r]) moves by the world-space displacement
 * D_r = displacement[3 r .. 3 r + 2] over the shutter interval: at time t in [0, 1) the root and its whole subtree -
 * leaves, group boxes, normals, patterns - are where they rest, translated by t * D_r.  Lights and the camera do not
 * move; motion is translation only.  Camera sample k of the whole-image pixel p in sample pass P has the time
 * t = the camera hash of (seed, p, P * S + k) on axis 255 (the sub-pixel offsets use axes 0 and 1, the lens 2 .. 65):
 * independent of bands, tiles and clones, new with every pass, and shared by the sample's reflected, refracted and
 * shadow rays.  Root r is tested with the ray's origin shifted to (o.x - t * D.x, o.y - t * D.y, o.z - t * D.z) and the
 * direction as it is; the hit object's normal and pattern are taken at p - t * D_r, component by component.  A root with
 * D = (0, 0, 0) is tested with the very operands of a static one; a handle whose displacements are all zero is static
 * and renders the bits of before.
 */
typedef struct rtc_motion {
  uint32_t n_roots;            /* the handle's root count (rtc_scene_desc.n_roots) */
  const double *displacement;  /* [n_roots][3], finite                           */
} rtc_motion;

/*
 * This handle's motion for every render entry point (NULL: static).  Validated before anything changes:
 * RTC_ERR_INVALID_ARGUMENT unless n_roots equals the handle's root count and every value is finite.  A clone starts
 * with its source's motion; rtc_render's band clones follow.  librtc_multi renders static scenes.
 */
int rtc_scene_set_motion(rtc_scene *scene, const rtc_motion *motion);

/* ---- spot lights: point lights that shine into a cone with a soft edge ---- */
/*
 * Light i (World.lights entry i, as the handle's light table holds it: point and area rows alike) with cone[i] == 1 is a
 * point light with the unit axis a = axis[3 i .. 3 i + 2] / sqrt((x * x + y * y) + z * z) (tuple.zig's normalize) and
 * -1 <= cos_outer[i] <= cos_inner[i] <= 1.  At a shading point with lv = point_to_light (v / distance):
 *   c = -((lv.x * a.x + lv.y * a.y) + lv.z * a.z)
 *   f = 1 if c >= cos_inner; else 0 if c <= cos_outer; else s = (c - cos_outer) / (cos_inner - cos_outer),
 *       f = (s * s) * (3.0 - 2.0 * s)
 * f == 0: the light gives `ambient` alone, and isShadowed is not called (no shadow_calls, no shadow ray).  Otherwise
 * isShadowed runs as before, and an unshadowed point's diffuse and specular colours are each scaled by f once formed:
 * (ambient + diffuse * f) + specular * f.  f == 1 gives the plain point light's bits; ambient is never scaled.
 * cone[i] == 0: the light as it is (the entry's other fields are not read).
 */
typedef struct rtc_spot {
  uint32_t n_lights;        /* the handle's light count                        */
  const uint8_t *cone;      /* [n_lights]: 1 a cone, 0 none                    */
  const double *axis;       /* [n_lights][3]: the cone's axis, any length > 0 */
  const double *cos_inner;  /* [n_lights]: full light inside                  */
  const double *cos_outer;  /* [n_lights]: no light outside                   */
} rtc_spot;

/*
 * This handle's spot lights for every render entry point (NULL, or every flag 0: no cones, the handle's old kernels).
 * Validated before anything changes: RTC_ERR_INVALID_ARGUMENT for a flag other than 0 or 1, a value that is not finite,
 * an axis of zero or non-finite magnitude, a cosine outside [-1, 1], cos_outer > cos_inner, n_lights other than the
 * handle's light count, or a cone on an area light.  A clone starts with its source's spots; rtc_render's band clones
 * follow.  librtc_multi renders without cones.
 */
int rtc_scene_set_spots(rtc_scene *scene, const rtc_spot *spots);

/* ---- normal perturbation: materials whose shading normal is bumped ---- */
/*
 * A bump belongs to a material row (mat_* tables).  For a hit on a leaf whose material has one, PreComputations.new
 * (world.zig:196-250) changes in one place.  With lp the hit point in object space and ln the local normal exactly as
 * Shape.normalAt (shape.zig:338-350) computes them (for a moving root: through p - tm * D, as rtc_scene_set_motion says):
 *  1. The geometric normal ng is normalToWorld(ln), negated when dot(ng, eyev) < 0 (`inside`), as without a bump.
 *     `inside`, over_point, under_point, the containers walk and n1 / n2 use ng and nothing else: a bump never changes
 *     which object a shadow, reflected or refracted ray starts inside or outside of.
 *  2. The shading normal ns: m = sqrt((ln.x * ln.x + ln.y * ln.y) + ln.z * ln.z) (tuple.zig's normalize); m == 0 gives
 *     ns = ng.  Otherwise u = ln / m, q = B * lp with B = inverse[12] (rows 0..2 of a 4 x 4 affine inverse transform, each
 *     row ((r0 * x + r1 * y) + r2 * z) + r3), d = field(q), ln' = u + d * amplitude (per component), ns =
 *     normalToWorld(ln') (with its normalize), negated when `inside` is true - step 1's decision, not a new dot product.
 *  3. ns replaces normalv in Material.lighting (point, spot and area lights alike), in reflectv, in refractedColor
 *     (cos_i = dot(eyev, ns), and the refracted direction) and in schlick.  Nothing else reads it.
 * The fields use + - * / sqrt floor fabs only, each operation correctly rounded, in the order written:
 *   RTC_BUMP_NOISE    d = (N(q.x, q.y, q.z), N(q.x, q.y, q.z + 1.0), N(q.x, q.y, q.z + 2.0)), N = octaveNoise(...,
 *                     octaves, persistence) of noise.zig:35-49 - the three evaluations of perturb.zig:31-43.
 *   RTC_BUMP_RIPPLES  around the field's y axis: r = sqrt(q.x * q.x + q.z * q.z); r == 0 gives d = 0; otherwise
 *                     v = 2.0 * (r - floor(r)) - 1.0, h = (4.0 * v) * (1.0 - fabs(v)), d = (h * (q.x / r), 0, h * (q.z / r)).
 * A material of kind RTC_BUMP_NONE, or of amplitude 0 whatever its kind, takes the unperturbed branch: ln is never
 * normalized first, ns is ng, and its pixels have the bits they have without a bump table (its other fields are not read).
 */
#define RTC_BUMP_NONE 0u
#define RTC_BUMP_NOISE 1u
#define RTC_BUMP_RIPPLES 2u
#define RTC_BUMP_MAX_OCTAVES 16u

typedef struct rtc_bump {
  uint32_t n_materials;       /* the handle's material count                                          */
  const uint8_t *kind;        /* [n_materials]: RTC_BUMP_*                                            */
  const double *amplitude;    /* [n_materials]: >= 0                                                  */
  const uint32_t *octaves;    /* [n_materials]: 1 .. RTC_BUMP_MAX_OCTAVES (RTC_BUMP_NOISE; PerturbInfo's default is 3) */
  const double *persistence;  /* [n_materials]: finite (RTC_BUMP_NOISE; PerturbInfo's default is 0.8)   */
  const double *inverse;      /* [n_materials][12]: B, rows 0..2; NULL: the identity for every material */
} rtc_bump;

/*
 * This handle's bumps for every render entry point (NULL, or every material unperturbed: the handle's previous kernels and
 * their bits).  Validated before anything changes: RTC_ERR_INVALID_ARGUMENT for n_materials other than the handle's, an
 * unknown kind, a value that is not finite (the matrix included), a negative amplitude, or octaves of 0 or above
 * RTC_BUMP_MAX_OCTAVES.  A clone starts with its source's bumps; rtc_render's band clones follow.  librtc_multi renders
 * without bumps.
 */
int rtc_scene_set_bumps(rtc_scene *scene, const rtc_bump *bumps);

/* ---- UV-mapped mesh textures: OBJ texture coordinates on triangles ---- */
/*
 * RTC_TEX_MESH is a fifth tex_mapping.  It uses tex_uv entry 0, like every mapping but the cubic one.  Where the other
 * mappings find (u, v) from the pattern-space point, a texture map of this mapping is evaluated for a hit whose leaf is a
 * triangle (RTC_TRIANGLE or RTC_SMOOTH_TRIANGLE) with
 *   - that triangle's texture row (a1, b1, a2, b2, a3, b3): the (u, v) of p1, p2, p3, row leaf_geom of the table below;
 *   - the entry's barycentrics (u, v), exactly as Moller-Trumbore (triangle.zig:29-63, 225-259) produced them for the entry
 *     that became the hit - the values the smooth normal n2 * u + n3 * v + n1 * (1 - u - v) is formed with.
 *     w  = (1.0 - u) - v
 *     tu = (a2 * u + a3 * v) + a1 * w
 *     tv = (b2 * u + b3 * v) + b1 * w
 *     each of tu, tv: if it is < 0.0 or > 1.0, it becomes x - floor(x)      (tiling; 0.0 and 1.0 stay)
 * After that the uv pattern of tex_uv entry 0 - align check, uv checkers, uv image with either interpolation, uv test - is
 * evaluated at (tu, tv) as for every other mapping.  The pattern's own inverse transform is not applied to (tu, tv): the row
 * is the placement.  A sub-pattern the uv pattern selects (align check, uv checkers) is evaluated at the object point, as
 * for the other mappings.  On a hit whose leaf is not a triangle, and on a handle without a texture table, the row is six
 * zeros and (u, v) = (0, 0): tu = tv = 0.  The map may sit wherever a texture map may - below stripes, checkers, a perturb,
 * a blend -: the hit's triangle and barycentrics are constants of the whole pattern evaluation (a perturb moves the object
 * point, never them).  Only + - * floor and comparisons are added, each operation correctly rounded, in the order written.
 */
typedef struct rtc_mesh_uvs {
  uint32_t n_tris;  /* the handle's triangle count (rtc_scene_desc::n_tris) */
  const double *uv; /* [n_tris][6]: (a1, b1, a2, b2, a3, b3) per triangle, in tri_* order */
} rtc_mesh_uvs;

/*
 * This handle's texture rows for every render entry point (NULL: the all-zero rows).  Validated before anything changes:
 * RTC_ERR_INVALID_ARGUMENT for an n_tris other than the handle's, or a value that is not finite.  A clone starts with its
 * source's rows; rtc_render's band clones follow.  A handle whose description has a map of mapping RTC_TEX_MESH renders
 * with the meshuv kernels whether or not it has a table; librtc_multi refuses such a description.
 */
int rtc_scene_set_mesh_uvs(rtc_scene *scene, const rtc_mesh_uvs *uvs);

/* ---- glossy reflection and refraction: rough materials scatter their rays ---- */
/*
 * A material row has two roughness values, `reflection` and `transmission`, each finite and in [0, 1]; 0 is today's
 * perfectly sharp mirror or glass.
 *
 * Path code.  Every ray of a pixel's ray tree has one: the primary ray 1, the reflected child of a ray with code c 2 c,
 * the refracted child 2 c + 1 (max_depth <= RTC_MAX_DEPTH = 16: a code is below 2^17).
 *
 * Direction.  At a hit whose material has reflection > 0 the reflected direction d is formed exactly as without gloss,
 * from the shading normal, and then replaced:
 *   s  = the first of 32 draws (a, b, c), each component 2.0 * J(3 t + i) - 1.0 with t = 0 .. 31 and i = 0, 1, 2,
 *        for which ((a * a) + (b * b)) + (c * c) <= 1.0; if none passes, s = (0, 0, 0) (the lens sampler's rule)
 *   e  = d + s * roughness                                   (per component)
 *   m  = sqrt((e.x * e.x + e.y * e.y) + e.z * e.z)
 *   d' = e / m when m != 0, else d                           (tuple.zig's normalize)
 *   the child's direction is d' when dot(d', ng) > 0.0, otherwise d
 * ng is the geometric normal after its `inside` flip; dot is (x + y) + z.  d' is a unit vector, as the next hit's eyev must
 * be for Material.lighting.  For transmission > 0 the same steps are applied to the refracted direction, with the child's
 * code 2 c + 1, and d' is used when dot(d', ng) < 0.0.  Weights, n1 / n2, schlick, over_point, under_point and the counts
 * of secondary rays are untouched.  Only + - * / sqrt and comparisons are added, each correctly rounded, in the order written.
 *
 * Draws.  With GOLD = 0x9E3779B97F4A7C15 and rtc_mix64 splitmix64's finaliser (the camera hash's),
 *   J(axis) = (rtc_mix64(h + GOLD * (((code << 8) | axis) + 1)) >> 11) * 2^-53
 *   h       = rtc_mix64(key + GOLD * (((p << 32) | (g << 8)) + 1))
 *   key     = rtc_mix64(seed ^ 0x13198A2E03707344)
 * p is the whole-image pixel (y * hsize + x), g the global sample index sample_base + k of rtc_scene_set_sample_pass,
 * code the child's path code.  A ray's draws do not depend on bands, tiles, clones, the lane that traced it or the order;
 * they are new for every camera sample and every pass, so progressive and adaptive rendering converge a rough surface.
 * Like the lens, gloss is always sampled: a 1 x 1 grid without jitter at pass 0 still scatters.
 *
 * A row whose two values are 0 takes the unscattered branch and draws nothing: its pixels have the bits they have without
 * a table.
 */
typedef struct rtc_gloss {
  uint32_t n_materials;       /* the handle's material count (rtc_scene_desc::n_materials) */
  const double *reflection;   /* [n_materials], each finite and in [0, 1]; NULL: all zeros */
  const double *transmission; /* [n_materials], each finite and in [0, 1]; NULL: all zeros */
  uint64_t seed;              /* of the draws (above) */
} rtc_gloss;

/*
 * This handle's roughness rows for every render entry point.  Validated before anything changes: RTC_ERR_INVALID_ARGUMENT
 * for an n_materials other than the handle's, or a value that is not finite or outside [0, 1]; the previous table stays in
 * force.  NULL, or a table whose every row is zero, gives the handle its previous kernels back.  A clone starts with its
 * source's table; rtc_render's band clones follow.  A handle with a rough row renders with the gloss kernels
 * (rtc_render_kernel_gloss, _gloss_bigworld).  librtc_multi renders without gloss.
 */
int rtc_scene_set_gloss(rtc_scene *scene, const rtc_gloss *gloss);

/* ---- ambient occlusion: hemisphere rays dim a material's ambient term ---- */
/*
 * A material row has one value, `radius`, finite and >= 0; 0 is the material's ambient term as it is.  The table also has
 * `samples` (1 .. RTC_OCCLUSION_MAX_SAMPLES) and a `seed`.
 *
 * The step.  At every hit - of a primary or of a secondary ray - whose material row has radius > 0 and whose
 * material.ambient != 0.0, once, before the lights:
 *   for k = 0 .. samples - 1:
 *     s  = the gloss sampler's rule: the first of 32 triples (a, b, c), each component 2.0 * J(3 t + i) - 1.0 with
 *          t = 0 .. 31 and i = 0, 1, 2, for which q = ((a * a) + (b * b)) + (c * c) <= 1.0
 *     if no triple is accepted, or q == 0.0:  d = ng
 *     else  r = sqrt(q);  u = (a / r, b / r, c / r)
 *           e = ng + u                                          (per component)
 *           m = sqrt((e.x * e.x + e.y * e.y) + e.z * e.z)
 *           d = e / m when m != 0, else ng                      (tuple.zig's normalize)
 *     occluded_k = what World.isShadowed finds for a ray from over_point along d with distance = radius: the same
 *                  intersections, the same casts_shadow filter, the same comparison of t with distance; under motion at the
 *                  ray's shutter time, like every shadow ray
 *   vis = double(samples - count(occluded)) / double(samples)
 *   ka  = material.ambient * vis
 * ng is the geometric normal after its `inside` flip - the one over_point, under_point and the gloss side rule use -, not a
 * bumped shading normal.  ng + a unit vector is a cosine-weighted direction of ng's hemisphere: no side rule is needed.  ka
 * takes material.ambient's place in Material.lighting for every light of that hit, point, spot and area lights alike;
 * vis == 1.0 leaves the bits as they are.  Only + - * / sqrt and comparisons are added, each correctly rounded, in the
 * order written.
 *
 * Draws.  rtc_scene_set_gloss's functions with a key of their own:
 *   J(axis) = (rtc_mix64(h + GOLD * (((word << 8) | axis) + 1)) >> 11) * 2^-53,   word = (k << 17) | code
 *   h       = rtc_mix64(key + GOLD * (((p << 32) | (g << 8)) + 1))
 *   key     = rtc_mix64(seed ^ 0xA4093822299F31D0)
 * code is the path code of the ray that made the hit (below 2^17), k the sample (below 64: word is below 2^23), p the
 * whole-image pixel, g the global sample index.  The draws do not depend on bands, tiles, clones, the lane or the order;
 * they are new for every camera sample and every pass, so progressive and adaptive rendering converge the term.  Like gloss
 * and the lens, occlusion is always sampled.
 *
 * Counts.  Each such hit adds `samples` to shadow_calls and `samples` to shadow_traced.  A hit whose row is 0, or whose
 * material.ambient == 0.0, draws nothing and counts nothing: its pixels have the bits they have without a table.
 */
#define RTC_OCCLUSION_MAX_SAMPLES 64u

typedef struct rtc_occlusion {
  uint32_t n_materials; /* the handle's material count (rtc_scene_desc::n_materials) */
  const double *radius; /* [n_materials], each finite and >= 0; NULL: all zeros */
  uint32_t samples;     /* hemisphere rays per hit, 1 .. RTC_OCCLUSION_MAX_SAMPLES */
  uint64_t seed;        /* of the draws (above) */
} rtc_occlusion;

/*
 * This handle's occlusion radii for every render entry point.  Validated before anything changes: RTC_ERR_INVALID_ARGUMENT
 * for a radius that is not finite or below 0, for samples outside 1 .. RTC_OCCLUSION_MAX_SAMPLES, and then for an
 * n_materials other than the handle's; the previous table stays in force.  NULL, or a table whose every row is zero, gives
 * the handle its previous kernels back.  A clone starts with its source's table; rtc_render's band clones follow.  A handle
 * with a radius renders with the occlusion kernels (rtc_render_kernel_occl, _occl_bigworld).  librtc_multi renders without
 * occlusion.  rtc_scene_desc and RTC_ABI_VERSION are as they were.
 */
int rtc_scene_set_occlusion(rtc_scene *scene, const rtc_occlusion *occlusion);

/* ---- shadow filters: light through a filtering material is dimmed and tinted, not blocked ---- */
/*
 * A material row has a shadow filter: three doubles (fr, fg, fb), each finite and in [0, 1]; (0, 0, 0) is the material as
 * it is - it blocks light.
 *
 * The step.  Every call of World.isShadowed that a LIGHT makes - the point and spot branch of the lights loop, and each
 * sample of an area light - yields a transmittance instead of a bool:
 *   T = (1.0, 1.0, 1.0)
 *   for every entry (leaf, t) the reference's intersect would have appended, with 0.0 <= t < distance and the leaf
 *   casting a shadow:
 *     T.r = T.r * fr[material of leaf];  T.g = T.g * fg[...];  T.b = T.b * fb[...]
 *   blocked = T.r == 0.0 && T.g == 0.0 && T.b == 0.0          (the walk may stop as soon as this holds)
 * The entries that count are the ones isShadowed counts today: a sphere in the way gives two, a plane or a triangle one, a
 * csg unit those its rule lets through; an entry behind the origin (t < 0.0), or at or beyond the light (t >= distance),
 * gives none.  The order of the product is the walk's and is free: every factor is in [0, 1], a zero factor gives exactly
 * zero in any order, and two factors commute exactly; only three or more partial factors can differ, in the last bits.
 *
 * Point and spot lights (Material.lighting).  Where `blocked` holds, the shadowed branch as it is.  Otherwise
 *   (dr, dg, db) = (dr * T.r, dg * T.g, db * T.b)     the diffuse term, after the spot factor
 *   (pr, pg, pb) = (pr * T.r, pg * T.g, pb * T.b)     the specular term, after the spot factor
 * before the sum (ambient + diffuse) + specular.  T == (1, 1, 1) leaves the bits as they are.
 *
 * Area lights.  Sample k yields T_k; the scalar intensity = lit / samples becomes three values,
 *   intensity.c = (((0.0 + T_0.c) + T_1.c) + ...) / samples        per channel, in the loop's order: v outer, u inner
 * and (dr / samples) * intensity becomes (dr / samples) * intensity.r, and so for g and b.  When every T_k is (0, 0, 0) or
 * (1, 1, 1) the sum is the integer count and the bits are the ones without a table.
 *
 * Unchanged: shadow_matters, the light_dot_normal test and the spot cone's early answer, which decide whether isShadowed
 * is called and traced at all, and the counts shadow_calls and shadow_traced.  The occlusion rays of
 * rtc_scene_set_occlusion stay binary: any entry of a casts_shadow leaf within the radius occludes, whatever its filter -
 * a pane of glass still darkens the corner behind it.  A leaf with "shadow": false contributes nothing, whatever its
 * material's filter.  Only * and + and comparisons are added, each correctly rounded.
 */
typedef struct rtc_shadow_filters {
  uint32_t n_materials; /* the handle's material count (rtc_scene_desc::n_materials) */
  const double *rgb;    /* [n_materials][3], each finite and in [0, 1]; NULL: all zeros */
} rtc_shadow_filters;

/*
 * This handle's shadow filters for every render entry point.  Validated before anything changes:
 * RTC_ERR_INVALID_ARGUMENT for a value that is not finite or outside [0, 1], and then for an n_materials other than the
 * handle's; the previous table stays in force.  NULL, or a table whose every row is zero, gives the handle its previous
 * kernels back.  A clone starts with its source's table; rtc_render's band clones follow.  A handle with a non-zero row
 * renders with the shadow-filter kernels (rtc_render_kernel_sfilter, _sfilter_bigworld).  librtc_multi renders without
 * shadow filters.  rtc_scene_desc and RTC_ABI_VERSION are as they were.
 */
int rtc_scene_set_shadow_filters(rtc_scene *scene, const rtc_shadow_filters *filters);

/* ---- participating media: absorbing materials and a uniform fog attenuate a ray along its way ---- */
/*
 * Tables.  A material row has an absorption (ar, ag, ab) per unit of world distance, each finite and >= 0; (0, 0, 0) is the
 * material as it is.  The handle has one atmosphere: fog_density, finite and >= 0, and fog_color[3], each finite and >= 0.
 *
 * A ray's medium.  Every ray of the colorAt tree carries a medium: a material index, or RTC_NO_MEDIUM for the atmosphere.
 *   - A camera ray, with or without sampling or a lens, is in the atmosphere: the camera is taken to stand outside every
 *     solid.
 *   - A reflected child has its parent's medium.
 *   - A refracted child has the material whose ior the parent's hit took for n2 (PreComputations.new's containers walk),
 *     by exactly the selection made for n2:
 *       the hit's material, where the hit shape is not among the containers at the hit (the ray enters it);
 *       else the material of the last container that remains once the hit shape is removed, if there is one;
 *       else the hit's material, if the hit's t occurs twice or more among the hit shape's entries;
 *       else RTC_NO_MEDIUM - the case where n2 stays 1.0.
 *
 * The step.  Applied to every ray of the tree after its closest-hit trace, whatever its remaining depth, before shading and
 * before the children are formed.  W is the ray's weight, one value per channel; acc the pixel's colour; (dx, dy, dz) the
 * ray's direction; c runs over r, g, b:
 *   sigma = medium == RTC_NO_MEDIUM ? (fog_density, fog_density, fog_density) : absorption[medium]
 *   hit at t:  dist = t * sqrt((dx*dx + dy*dy) + dz*dz)
 *              T.c  = sigma.c == 0.0 ? 1.0 : exp(-(sigma.c * dist))
 *   miss:      T.c  = sigma.c == 0.0 ? 1.0 : 0.0
 *   if medium == RTC_NO_MEDIUM && fog_density > 0.0:
 *              acc.c = acc.c + W.c * ((1.0 - T.c) * fog_color.c)
 *   W.c = W.c * T.c
 * On a hit the ray goes on as before with W: the hit contributes W.c * s.c, the children get W.c * w_reflect and
 * W.c * w_refract.  On a miss the ray ends as before after the in-scatter term.  An all-zero table and a density of zero
 * leave every bit as it is: T == 1 multiplies exactly and the fog term is not formed.  Nothing is culled by a small weight:
 * primary, secondary, shadow_calls and shadow_traced are those of the same handle without media.  exp is the FP64 library
 * function: its last bits may differ between implementations.
 *
 * Unchanged.  Shadow rays - the products of rtc_scene_set_shadow_filters included - and occlusion rays are not attenuated
 * by media.  The fog is not lit by the lights: it is a constant in-scatter colour.  Gloss draws, sampling, motion,
 * accumulation and the adaptive loop stay as they are.
 */
#define RTC_NO_MEDIUM 0xFFFFFFFFu
typedef struct rtc_media {
  uint32_t n_materials;     /* the handle's material count (rtc_scene_desc::n_materials) */
  const double *absorption; /* [n_materials][3], each finite and >= 0; NULL: all zeros */
  double fog_density;       /* finite and >= 0; 0: no fog */
  double fog_color[3];      /* each finite and >= 0 */
} rtc_media;

/*
 * This handle's media for every render entry point.  Validated on the host before anything changes:
 * RTC_ERR_INVALID_ARGUMENT for a value that is not finite or is negative, and then for an n_materials other than the
 * handle's; the previous table stays in force.  NULL, or a table whose every row is zero with a density of zero, gives the
 * handle its previous kernels back.  A clone starts with its source's media; rtc_render's band clones follow.  A handle with
 * an absorbing row or a fog renders with the media kernels (rtc_render_kernel_media, _media_bigworld).  librtc_multi renders
 * without media.  rtc_scene_desc, rtc_camera and RTC_ABI_VERSION are as they were.
 */
int rtc_scene_set_media(rtc_scene *scene, const rtc_media *media);

/* ---- the environment: a sky behind the world and suns that light it ---- */
/*
 * The sky.  Applied to every ray of the colorAt tree whose closest-hit trace finds nothing, after the media step above - W,
 * the ray's weight per channel, is already multiplied by the miss transmittance -, in place of the reference's black
 * (world.zig:119).  (dx, dy, dz) is the ray's direction, c runs over r, g, b:
 *   len = sqrt((dx*dx + dy*dy) + dz*dz)            (RTC_ENV_SPHERE)
 *   len = max(|dx|, max(|dy|, |dz|))               (RTC_ENV_CUBE: where the direction meets the unit cube)
 *   p   = (dx / len, dy / len, dz / len)
 *   E.c = pattern == RTC_ENV_NO_PATTERN ? rgb.c : pattern_at(pattern, p).c * rgb.c
 *   acc.c = acc.c + W.c * E.c
 * pattern_at is the evaluation a material's pattern gets (Pattern.patternAt): p is taken as an object-space point and the
 * pattern's own inverse transform is applied to it, so a pattern transform turns the sky.  Every pattern kind is a sky.  A
 * spherical texture map does not depend on len; a cubic one wants RTC_ENV_CUBE.  A texture map of mapping RTC_TEX_MESH is
 * evaluated with no hit triangle (tri == RTC_NO_LEAF): the row of zeros.  A sky of colour zero without a pattern adds
 * nothing and the step is not run.  A miss stays a miss: primary and secondary are those of the handle without an
 * environment.  A miss in fog or inside an absorbing material has W == 0 and adds +0: a sky is not seen through an infinite
 * fog.  Occlusion rays and shadow rays do not see the sky.
 *
 * The suns.  sun_direction is the way the light TRAVELS, any length > 0; the host normalises once,
 *   a = direction / sqrt((x*x + y*y) + z*z),   lv = (-a.x, -a.y, -a.z),
 * and a row keeps lv and sun_rgb.  At every hit, after the loop over World.lights (world.zig:89-96) and in table order, a
 * sun is a point light in everything but its geometry: point_to_light = lv, distance = +infinity.  shadow_calls grows by
 * one per sun and hit.  With shadow_matters (the material's diffuse or specular is not zero) and light_dot_normal >= 0 the
 * shadow ray is traced from over_point along lv and counted in shadow_traced: every entry with et >= 0 on a casts_shadow
 * leaf counts, however far away, and the rows of rtc_scene_set_shadow_filters multiply as they do for any light.
 * Material.lighting adds ambient + diffuse + specular with sun_rgb as the intensity - the ambient term with the occlusion
 * step's ka, the normal the bumped shading normal.  Spot cones do not apply.  The fog does not dim a sun's shadow ray.
 * Suns do not count towards the light limit of the kernels that keep their tables in LDS.
 */
#define RTC_ENV_NO_PATTERN 0xFFFFFFFFu
#define RTC_ENV_SPHERE 0u
#define RTC_ENV_CUBE 1u
#define RTC_ENV_MAX_SUNS 16u
typedef struct rtc_environment {
  double rgb[3];               /* the sky's colour; with a pattern, the factor on the pattern's colour */
  uint32_t pattern;            /* a row of the handle's pat_* tables, or RTC_ENV_NO_PATTERN */
  uint32_t projection;         /* RTC_ENV_SPHERE / RTC_ENV_CUBE */
  uint32_t n_suns;             /* <= RTC_ENV_MAX_SUNS */
  const double *sun_direction; /* [n_suns][3] the way the light TRAVELS, any length > 0 */
  const double *sun_rgb;       /* [n_suns][3] intensity */
} rtc_environment;

/*
 * This handle's environment for every render entry point.  Validated on the host before any HIP call and before anything
 * changes: RTC_ERR_INVALID_ARGUMENT for a value that is not finite, a negative rgb or sun_rgb, a pattern that is
 * >= n_patterns and not RTC_ENV_NO_PATTERN, a projection other than 0 or 1, n_suns > RTC_ENV_MAX_SUNS, n_suns > 0 with a
 * NULL table, a direction of zero or non-finite magnitude; the previous table stays in force.  NULL, or rgb all zero with no
 * pattern and no suns, is no environment and gives the handle its previous kernels back.  A clone starts with its source's
 * environment; rtc_render's band clones follow.  A handle with an environment renders with the environment kernels
 * (rtc_render_kernel_env, _env_bigworld).  librtc_multi renders without it.  rtc_scene_desc, rtc_camera, rtc_stats and
 * RTC_ABI_VERSION are as they were.
 */
int rtc_scene_set_environment(rtc_scene *scene, const rtc_environment *environment);

/* ---- the sky light: hemisphere rays that reach the sky light diffuse surfaces ---- */
/*
 * A handle has one sky light: a gain (finite, >= 0), samples (1 .. RTC_SKY_LIGHT_MAX_SAMPLES) and a seed.  The step runs at
 * every hit, of a primary or a secondary ray, with material.diffuse != 0.0, gain > 0 and a handle whose environment has a sky
 * (a colour that is not zero, or a pattern).  It runs once per hit, and its result is added after the suns' loop above
 * (c runs over r, g, b):
 *   L = (0.0, 0.0, 0.0)
 *   for k = 0 .. samples - 1:
 *     d   = the occlusion step's direction rule, unchanged (the first accepted of 32 triples, e = ng + u, d = e / m, the two
 *           fall-backs to ng), with J drawn from this table's key (below)
 *     T   = what a sun's shadow ray yields for origin over_point, direction d, distance = +infinity: (1, 1, 1) times the
 *           row of rtc_scene_set_shadow_filters of every entry with et >= 0 on a casts_shadow leaf - a leaf without a filter
 *           row, or a handle without a filter table, gives (0, 0, 0) at the first such entry -, under motion at the ray's
 *           shutter time
 *     if T != (0, 0, 0):
 *       E   = the sky at d: the miss formula of the section above with (dx, dy, dz) = d (len, p = d / len, pattern or rgb)
 *       L.c = L.c + T.c * E.c                                  in k's order
 *   G.c = gain * (L.c / double(samples))
 *   s.c = s.c + (color.c * material.diffuse) * G.c             after the last sun's  s = s + l
 * ng is the geometric normal after its `inside` flip, as in the occlusion step, not the bumped shading normal; color is the
 * pattern colour the lights' loop uses at that hit.  A cosine-weighted direction has density cos / pi, so the mean of T * E
 * is the Lambertian irradiance estimate: no pi and no cosine appear.  A blocked sample adds nothing.  Only + - * / sqrt and
 * comparisons are added, each correctly rounded, in the order written.
 *
 * The draws are the occlusion step's functions with a key of their own: J(axis) = rtc_gloss_jitter(h, (k << 17) | code, axis),
 * h = rtc_gloss_sample_key(key, p, g), key = rtc_mix64(seed ^ 0x082EFA98EC4E6C89) - independent of the occlusion step's, new
 * per camera sample and pass, independent of bands, tiles, clones, lanes and order.  Like gloss and occlusion, the term is
 * always sampled.
 *
 * Counts: each such hit adds `samples` to shadow_calls and to shadow_traced; a hit with diffuse == 0.0 draws nothing and counts
 * nothing; primary and secondary are those of the handle without the table.  The occlusion step and its ka, the miss step
 * and the suns are as they were.  Sky-light rays are a third kind beside occlusion rays and shadow rays: they alone see the
 * sky, where nothing blocks them; like a sun's shadow ray they are not dimmed by fog or absorption.  A hemisphere ray that
 * hits something contributes nothing of that surface's light.
 */
#define RTC_SKY_LIGHT_MAX_SAMPLES 64u
typedef struct rtc_sky_light {
  double gain;      /* the factor on the gathered sky; finite, >= 0; 0: no sky light */
  uint32_t samples; /* hemisphere rays per hit, 1 .. RTC_SKY_LIGHT_MAX_SAMPLES */
  uint64_t seed;
} rtc_sky_light;

/*
 * This handle's sky light for every render entry point.  Validated on the host before any HIP call and before anything
 * changes: RTC_ERR_INVALID_ARGUMENT for a gain that is not finite or is negative, or samples outside
 * 1 .. RTC_SKY_LIGHT_MAX_SAMPLES; the previous table stays in force.  NULL, or a gain of zero, is no sky light.  A clone
 * starts with its source's table; rtc_render's band clones follow.  The order of this setter and rtc_scene_set_environment
 * does not matter: which kernels run is decided at launch - the sky-light kernels (rtc_render_kernel_skyl, _skyl_bigworld)
 * when the handle has a sky light and an environment with a sky; every other handle gets the kernels it got before.
 * librtc_multi renders without it.  rtc_scene_desc, rtc_camera, rtc_stats, rtc_environment and RTC_ABI_VERSION are as they
 * were.
 */
int rtc_scene_set_sky_light(rtc_scene *scene, const rtc_sky_light *sky_light);

/* ---- indirect light: diffuse bounce rays and emissive materials ---- */
/*
 * A handle has one indirect table: a gain (finite, >= 0), bounces (0 .. RTC_MAX_DEPTH = 16), a seed and, optionally, an
 * emission row of three finite doubles >= 0 per material (NULL: no material emits).  c runs over r, g, b.
 *
 * Emission.  At every hit, of a primary or a secondary ray,
 *   s.c = s.c + emission[material].c          after the last light's, sun's and sky-light term, before the ray's weight
 * It needs no gain and no bounces.
 *
 * The diffuse child.  Every ray carries d, the number of diffuse bounces on its lineage; the primary ray has d = 0, a
 * reflected or refracted child its parent's d.  A hit forms the child when gain > 0, material.diffuse != 0.0,
 * cur.remaining > 0 and d < bounces:
 *   origin    = over_point
 *   direction = the occlusion step's direction rule, unchanged (the first accepted of 32 triples, e = ng + u, d = e / m, the
 *               two fall-backs to ng) about ng, the geometric normal after its `inside` flip - not the bumped normal, not
 *               the mirror direction -, with J(axis) = rtc_gloss_jitter(h, (d << 17) | cur.code, axis),
 *               h = rtc_gloss_sample_key(key', p, g), key = rtc_mix64(seed ^ 0x452821E638D01377)
 *   remaining = cur.remaining - 1;  d + 1;  the parent's medium;  path code 2 * cur.code (the reflected child's)
 *   weight.c  = cur.weight.c * ((color.c * material.diffuse) * gain)
 * cur.weight is the weight after the media step, color the pattern colour the lights' loop uses at that hit.  A
 * cosine-weighted direction has density cos / pi, so, as for the sky light, no pi and no cosine appear.  The child is an
 * ordinary ray: traced, shaded, fogged and absorbed like any other, it forms children like any other and counts one
 * `secondary`.  The pixel gets the sum of weight.c * s.c over every ray of its tree, as before.
 *
 * No sky counted twice.  Where the sky-light step ran at the parent hit (the sky light's gain > 0 and the environment has a
 * sky), the miss step of the ray that was formed as a diffuse child adds no sky (the media step's fog term stays).  A miss
 * of its reflected or refracted descendants adds the sky as before.
 *
 * Decorrelation.  At a ray with d > 0 the gloss, occlusion, sky-light and indirect draws use
 *   key' = key ^ ((uint64_t)d * RTC_INDIRECT_DECORR)
 * in place of their table's key; with d == 0 this is the key itself, and every draw of a handle without the table keeps its
 * bits.  Two rays of one pixel's tree that share both path code and d share their draws: that correlates the two branches
 * and does not bias the mean, because along one lineage the codes differ.
 *
 * Counts: primary as before; secondary grows by one per child; shadow_calls and shadow_traced grow by what the child's own
 * hits count.  Only + - * / sqrt and comparisons are added, each correctly rounded, in the order written.
 */
#define RTC_INDIRECT_DECORR 0xBE5466CF34E90C6Dull /* odd */
typedef struct rtc_indirect {
  double gain;            /* the factor on a diffuse child's weight; finite, >= 0; 0: no child */
  uint32_t bounces;       /* the most diffuse bounces on one lineage, 0 .. RTC_MAX_DEPTH; 0: no child */
  uint64_t seed;
  const double *emission; /* [n_materials][3], finite, >= 0; NULL: no material emits */
  uint32_t n_materials;   /* with emission: the scene's material count */
} rtc_indirect;

/*
 * This handle's indirect light for every render entry point.  Validated on the host before any HIP call and before anything
 * changes: RTC_ERR_INVALID_ARGUMENT for a gain that is not finite or is negative, bounces above RTC_MAX_DEPTH, a non-NULL
 * emission whose n_materials is not the scene's, or an emission entry that is not finite or is negative; the previous table
 * stays in force.  NULL is no table.  The rows are copied.  A clone starts with its source's table; rtc_render's band clones
 * follow.  The order of this setter and the others does not matter: which kernels run is decided at launch - the indirect
 * kernels (rtc_render_kernel_indir, _indir_bigworld) when the table has gain > 0 and bounces > 0 or an emission entry that
 * is not zero; every other handle gets the kernels it got before.  librtc_multi renders without it.  rtc_scene_desc,
 * rtc_camera, rtc_stats and RTC_ABI_VERSION are as they were.
 */
int rtc_scene_set_indirect(rtc_scene *scene, const rtc_indirect *indirect);

/* ---- emitter sampling: emissive surfaces sampled directly at diffuse hits ---- */
/*
 * A handle has one emitter table: samples (1 .. RTC_EMITTER_MAX_SAMPLES) and a seed.  The list of emitters is not passed in:
 * it is derived from the handle's own tables, in doubles, whenever rtc_scene_set_emitters, rtc_scene_set_indirect or
 * rtc_scene_set_shadow_filters runs.  c runs over r, g, b.
 *
 * Emitters.  A leaf is an emitter when its material's emission row E of the indirect table is not (0, 0, 0); it is a triangle,
 * a smooth triangle or a cube; no node above it is a csg node; its casts_shadow is set; and its material's shadow-filter row,
 * if the handle has a filter table, is (0, 0, 0) - a shadow ray towards a cube's far face must be stopped by its near face.
 * Leaves are taken in depth-first order (roots[] / children[]).  With I the leaf's inverse (xf_inv, rows 0 .. 2: A its
 * 3 x 3 part, b its last column), the forward map is
 *   c00 = a11 a22 - a12 a21   c01 = a12 a20 - a10 a22   c02 = a10 a21 - a11 a20
 *   c10 = a02 a21 - a01 a22   c11 = a00 a22 - a02 a20   c12 = a01 a20 - a00 a21
 *   c20 = a01 a12 - a02 a11   c21 = a02 a10 - a00 a12   c22 = a00 a11 - a01 a10
 *   det = (a00 c00 + a01 c01) + a02 c02;   L[i][j] = c[j][i] / det;   t_i = -((L[i][0] b0 + L[i][1] b1) + L[i][2] b2)
 *   point(p)_i = ((L[i][0] px + L[i][1] py) + L[i][2] pz) + t_i;   vector(v)_i = (L[i][0] vx + L[i][1] vy) + L[i][2] vz
 * A triangle is one entry: origin = point(p1), eu = vector(e1), ev = vector(e2), half = 1.  A cube is six, its faces in the
 * order +x, -x, +y, -y, +z, -z: for the face of axis a and sign s, with b = (a + 1) mod 3 and c = (a + 2) mod 3,
 * origin = point(o), o_a = s, o_b = o_c = -1;  eu = vector(2 e_b);  ev = vector(2 e_c);  half = 0.  For every entry
 *   m = eu x ev (each component x1 y2 - x2 y1 in the cross product's cyclic order);  len = sqrt((mx mx + my my) + mz mz)
 *   n = m / len;   A = len, and len / 2 where half = 1;   w = A * ((E.r + E.g) + E.b)
 * An entry whose w is not finite or not above zero is left out.  cdf[k] = cdf[k - 1] + w_k in list order (cdf[-1] = 0); W is
 * the last; every entry stores q = W / ((E.r + E.g) + E.b).  More than RTC_MAX_EMITTERS entries: RTC_ERR_UNSUPPORTED.
 * Spheres, cylinders, cones, tori, planes and the leaves of a csg are not listed: they light what a bounce ray finds.
 *
 * Where a sample is drawn.  At a hit that forms the diffuse child of rtc_scene_set_indirect - gain > 0, material.diffuse !=
 * 0.0, cur.remaining > 0, d < bounces - when the list is not empty.  After the sky-light step, for j = 0 .. samples - 1:
 *   J(axis) = rtc_gloss_jitter(h, (j << 17) | cur.code, axis),  h = rtc_gloss_sample_key(key', p, g),
 *   key = rtc_mix64(seed ^ 0xC0AC29B7C97C50DD), key' as the indirect table's decorrelation has it
 *   u0 = J(0);  k = the first entry with cdf[k] > u0 * W, the last entry where there is none
 *   u = J(1), v = J(2);  where half = 1 and u + v > 1.0:  u = 1.0 - u, v = 1.0 - v
 *   Y_i = (origin_i + u * eu_i) + v * ev_i
 *   v = Y - over_point;  r2 = (vx vx + vy vy) + vz vz;  r = sqrt(r2);  w = v / r
 *   cos_x = (ng.x wx + ng.y wy) + ng.z wz     ng: the geometric normal after its `inside` flip, not the bumped normal
 *   cos_e = |(n.x wx + n.y wy) + n.z wz|      an emitter emits on both sides, as a hit on either side adds its row
 *   where cos_x <= 0, cos_e == 0 or r <= 2e-4 the sample is zero, no walk is made and nothing is counted;
 *   otherwise one shadow walk from over_point along w: the product F of the shadow-filter rows of every entry with
 *   0 <= t < r - 1e-4 on a casts_shadow leaf (all zero: blocked, the sample is zero); it counts one shadow_calls and one
 *   shadow_traced
 *   term.c = (((E.c * q) * ((cos_x * cos_e) / (RTC_PI * r2))) * F.c),  with media times T.c, the transmittance of
 *   rtc_scene_set_media for a segment of length r in the current ray's medium (sigma.c == 0: the term as it is; else
 *   times exp(-(sigma.c * r))); the fog's own colour does not enter
 *   sum.c = sum.c + term.c
 * and then, before the emission row,
 *   s.c = s.c + (color.c * material.diffuse) * (gain * (sum.c / samples))
 *
 * Nothing counted twice.  The ray that was formed as a diffuse child adds no emission row at a hit on a leaf of the list:
 * its parent's samples counted that light.  Its reflected and refracted descendants, and every other ray, add emission as
 * before.  The image's expectation is the one without the table.
 *
 * Only + - * / sqrt, exp (media) and comparisons are added, each correctly rounded, in the order written.
 */
#define RTC_PI 3.14159265358979323846
#define RTC_MAX_EMITTERS 4096u
#define RTC_EMITTER_MAX_SAMPLES 16u
typedef struct rtc_emitters {
  uint32_t samples; /* samples per hit, 1 .. RTC_EMITTER_MAX_SAMPLES; their mean is taken */
  uint64_t seed;
} rtc_emitters;

/*
 * This handle's emitter sampling for every render entry point.  Validated on the host before any HIP call and before anything
 * changes: RTC_ERR_INVALID_ARGUMENT for samples outside 1 .. RTC_EMITTER_MAX_SAMPLES; RTC_ERR_UNSUPPORTED for a list of more
 * than RTC_MAX_EMITTERS entries and for a listed leaf below a root that rtc_scene_set_motion moves - rtc_scene_set_motion,
 * rtc_scene_set_indirect and rtc_scene_set_shadow_filters refuse in the same way what would make the list of a handle with
 * the table too long or move one of its leaves, whichever call comes second; the previous state stays in force.  NULL is no
 * table.  A clone starts with its source's table; rtc_render's band clones follow.  The order of this setter and the
 * others does not matter: the list is derived again whenever one of the three runs, and which kernels run is decided at
 * launch - the emitter kernels (rtc_render_kernel_emit, _emit_bigworld) when the derived list is not empty; every other
 * handle gets the kernels it got before.  librtc_multi renders without it.  rtc_scene_desc, rtc_camera, rtc_stats and
 * RTC_ABI_VERSION are as they were.
 */
int rtc_scene_set_emitters(rtc_scene *scene, const rtc_emitters *emitters);

/* ---- multiple importance sampling of emitter samples and bounce rays ---- */
/*
 * At a hit that draws emitter samples two strategies find the light of a listed emitter: the `samples` emitter samples and
 * the one cosine-weighted diffuse child.  With mode 0 they are combined by a switch - the samples take all of it, the child
 * adds nothing where it meets a listed leaf (above).  With mode 1 each is weighted by the balance heuristic (Veach and Guibas
 * 1995): the expectation stays, and what one pass returns is bounded.  Notation as above: n = samples as a double; q the
 * entry's W / ((E.r + E.g) + E.b) - the area density of a point of any entry of that material is 1 / q -; for one direction
 *   a = q * (cos_s * cos_e);   b = n * (RTC_PI * r2);   w_e = b / (b + a);   w_b = a / (b + a)
 * with cos_s the cosine at the shaded point.  This is n / (n + rho) and rho / (n + rho) with rho = a / (RTC_PI * r2) =
 * p_bounce / p_emitter in solid angle, in a form that divides by no vanishing r2 and forms no rho; the skip rules below keep
 * r2 > 4e-8, so b > 0 and b + a > 0.  Both weights divide by the one sum b + a: w_e + w_b = 1 within a rounding of each.
 *
 * Emitter sample (mode 1, list not empty).  cos_s = cos_x, cos_e and r2 as in the sample step; the skip rules - cos_x <= 0,
 * cos_e == 0, r <= 2e-4 -, the walk, the filters, the media factor and the counters are as they were;
 *   term.c = ((((E.c * q) * ((cos_x * cos_e) / (RTC_PI * r2))) * w_e) * F.c),  with media times T.c as before.
 *
 * Diffuse child.  Where the child is formed, cos_b = (dir.x ng.x + dir.y ng.y) + dir.z ng.z, its direction against the normal
 * it was drawn about; the value travels with the ray.  At that ray's hit - a ray that was formed as a diffuse child, not its
 * descendants - on a leaf of the list (mode 1), at parameter t along dir:
 *   the face: a triangle's, plain or smooth, is its one entry.  A cube's is the reference's rule for cube normals on the
 *     object-space hit point lp = I * (origin + dir * t): m = max(|lp.x|, max(|lp.y|, |lp.z|)); the x faces where m == |lp.x|,
 *     else the y faces where m == |lp.y|, else the z faces; of the pair, the negative face where that coordinate < 0.
 *   n_face, q: the unit normal n and the q that the list stores for that face's entry - the flat geometric normal, not a
 *     smooth triangle's interpolated one.  A face the list leaves out (w not finite or not above zero) is not sampled: w_b = 1.
 *   cos_e' = |(n_face.x dir.x + n_face.y dir.y) + n_face.z dir.z|;   r2 = t * t;   cos_s = cos_b
 *   where cos_b <= 0, cos_e' == 0 or t <= 2e-4 - where the sample step returns zero for this direction - w_b = 1
 *   s.c = s.c + E.c * w_b                      in the place of the emission row
 * Unlisted emissive leaves - spheres, cylinders, cones, tori, planes, csg leaves, filtered leaves - add their whole row, and
 * every other ray - primary, reflected, refracted - adds emission as before.
 *
 * The bound.  With mode 1 the light one hit takes from listed emitters - the mean of its samples plus its child's weighted
 * emission - is at most (n + 1) * max_c E.c, times color.c * material.diffuse * gain:  per sample
 * E.c * q * (cos_x cos_e / (pi r2)) * w_e = E.c * rho * n / (n + rho) <= n * E.c, so the mean of n is at most n * E.c;  the
 * child adds E.c * w_b <= E.c;  every filter and transmittance is <= 1.  With mode 0 there is no bound as r -> 0.
 *
 * Only + - * / and comparisons are added, each correctly rounded, in the order written, with no fused multiply-add.
 */
/*
 * This handle's combination of emitter samples and diffuse children: 0 - the switch, the default: every render is what it was,
 * bit for bit -, 1 - the balance heuristic.  Any other value: RTC_ERR_INVALID_ARGUMENT, refused before any HIP call, the
 * previous mode stays.  The mode has an effect only while the derived emitter list is not empty, whatever the order of this
 * setter, rtc_scene_set_emitters, rtc_scene_set_indirect and rtc_scene_set_shadow_filters; then the MIS kernels run
 * (rtc_render_kernel_mis, _mis_bigworld).  A clone starts with its source's mode; rtc_render's band clones follow.
 * librtc_multi renders without it.  rtc_scene_desc, rtc_camera, rtc_stats, rtc_emitters and RTC_ABI_VERSION are as they were.
 */
int rtc_scene_set_emitter_mis(rtc_scene *scene, uint32_t mode);

/* ---- adaptive sampling: progressive passes only for tiles still noisy ---- */
#define RTC_ADAPTIVE_MAX_TILE 1024u

/*
 * The image is cut into tile_w x tile_h tiles, numbered row-major as rtc_render_tile_list_device numbers them; edge tiles
 * hold only their pixels inside the image (n_t of them).  Round R = 0, 1, ... renders the active tiles at sample pass R
 * (rtc_scene_set_sample_pass's keying) and adds them into whole-image sums; P_t counts tile t's passes.  After a round tile
 * t stays active iff P_t < min_passes, or P_t < max_passes and noise_t > threshold, with
 *   noise_t = sqrt((1/n_t) * sum over its pixels of max(0, sumsq - P_t * |mean|^2) / (3 (P_t - 1) P_t))
 * (rtc_accum's noise restricted to the tile; +inf while P_t < 2).  A tile that stops is never touched again, so its
 * passes are exactly 0 .. P_t - 1: tile t of an adaptive run is the progressive image after P_t passes, to the bit.
 */
typedef struct rtc_adaptive {
  uint32_t tile_w, tile_h;  /* 1 .. RTC_ADAPTIVE_MAX_TILE                                               */
  uint32_t min_passes;      /* >= 2 (the noise needs two passes)                                         */
  uint32_t max_passes;      /* >= min_passes; max_passes * grid * grid <= RTC_SAMPLING_INDEX_LIMIT      */
  double threshold;         /* finite, >= 0: absolute, in the units of rtc_accum's noise                */
} rtc_adaptive;

/*
 * Caller-owned state of a run, device memory on the handle's device (N = hsize * vsize pixels, T tiles).  sum, sumsq,
 * mean and rgba are as rtc_accum's, per tile at P_t passes (read and written only for tiles being accumulated).  `active`
 * holds the n_active tiles still active, in ascending order; max_noise is the largest noise_t over all T tiles.
 */
typedef struct rtc_adaptive_state {
  double *sum;            /* [N][3], required                                     */
  double *sumsq;          /* [N], required                                        */
  double *mean;           /* [N][3] or NULL                                       */
  uint32_t *rgba;         /* [N] or NULL                                          */
  uint32_t *tile_passes;  /* [T], required: P_t                                   */
  double *tile_noise;     /* [T], required: noise_t                               */
  uint32_t *active;       /* [T], required                                        */
  uint32_t *n_active;     /* one, required                                        */
  double *max_noise;      /* one or NULL                                          */
  uint32_t round;         /* HOST field: the next round's R (begin: 0, step: + 1) */
} rtc_adaptive_state;

/* Zeroes every P_t, sets every noise_t (and max_noise) to +inf and makes every tile active; state->round = 0.
 * Asynchronous on `hip_stream` (NULL: the handle's own stream) like rtc_scene_accumulate_device. */
int rtc_scene_adaptive_begin_device(rtc_scene *scene, uint32_t hsize, uint32_t vsize, const rtc_adaptive *setting,
                                    rtc_adaptive_state *state, void *hip_stream);

/*
 * No rendering: adds the compact tile frame d_frame[n_tiles][tile_h][tile_w][3] (as rtc_render_tile_list_device leaves
 * it: region k is tile d_tiles[k]; d_tiles is device memory and holds distinct tiles) into the state's sums, one
 * work-group per tile, with P_t = P_t + 1 (1: overwrite); writes noise_t in a fixed order, then
 * applies the stopping rule to all T tiles and rebuilds `active`, n_active and max_noise by a scan.  The same inputs give
 * the same bits; no atomics.  Asynchronous, ordered as rtc_scene_accumulate_device.
 */
int rtc_scene_adaptive_accumulate_device(rtc_scene *scene, uint32_t hsize, uint32_t vsize, const rtc_adaptive *setting,
                                         const rtc_adaptive_state *state, const double *d_frame, const uint32_t *d_tiles,
                                         uint32_t n_tiles, void *hip_stream);

/*
 * One round: reads back n_active and the active list (a small synchronising copy), renders that list at sample pass
 * state->round into a frame buffer of the handle's (the handle's own sample pass is left as it is; its sampling, light
 * jitter and motion apply), accumulates it and writes the new n_active to *n_active_out (0: the run is over, nothing
 * was rendered).  Synchronous.
 */
int rtc_scene_adaptive_step(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth, const rtc_adaptive *setting,
                            rtc_adaptive_state *state, uint32_t *n_active_out, void *hip_stream);

/*
 * A whole run with buffers of its own: begin, then rounds until no tile is active.  rgb_out [vsize][hsize][3] (host) gets
 * the mean; tile_passes_out [T] (host, or NULL) every P_t.  Synchronous.
 */
int rtc_render_adaptive(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth, const rtc_adaptive *setting,
                        double *rgb_out, uint32_t *tile_passes_out);
/* (Every adaptive entry point checks all its arguments before the device is touched: RTC_ERR_INVALID_ARGUMENT, with
 * nothing changed, otherwise.) */

/* ---- denoising: variance-guided non-local means over an accumulated image ---- */
#define RTC_DENOISE_MAX_RADIUS 10u
#define RTC_DENOISE_MAX_PATCH 3u
#define RTC_DENOISE_EPS 1e-10
/*
 * An image-space filter guided only by what the accumulation already holds: the mean u ([vsize][hsize][3]) and the sum of
 * squares s ([vsize][hsize], rtc_accum's or rtc_adaptive_state's sumsq), from which every pixel has an estimate of its own
 * variance.  It is the variance-cancelling non-local means of Rousselle, Knaus and Zwicker (2012) on a single buffer.  No
 * render kernel is involved and no scene is needed.  Every operation is an IEEE double operation in the order written (no
 * fused multiply-add); max(0, x) is x > 0 ? x : 0 and min(x, y) is y < x ? y : x (so a NaN is dropped by max and kept
 * from x by min).
 *
 * P(x, y) is `passes`, or with tile_passes tile_passes[(y / tile_h) * ceil(hsize / tile_w) + x / tile_w] (the tiles of an
 * adaptive run, numbered as there).  k2 = strength * strength and c3 = 3.0 * cancel.  A pixel's variance is
 *     v(x, y) = P < 2 ? 0.0 : max(0, s - P * ((u.r * u.r + u.g * u.g) + u.b * u.b)) / (3.0 * ((P - 1.0) * P))
 * - the quantity under rtc_accum's noise sum, formed as there.  A pixel with P < 2 has variance 0.
 *
 * For a pixel p, W = 0 and A = (0, 0, 0); then for dy = -radius .. radius and, inside it, dx = -radius .. radius, both
 * ascending, with q = p + (dx, dy) inside the image:
 *     S = 0, n = 0
 *     for oy = -patch .. patch, inside it ox = -patch .. patch, ascending, with a = p + (ox, oy) and b = q + (ox, oy)
 *     both inside the image:
 *         D.c = u.c(a) - u.c(b)
 *         t   = ((D.r * D.r + D.g * D.g) + D.b * D.b) - c3 * (v(a) + min(v(a), v(b)))
 *         S   = S + t / (RTC_DENOISE_EPS + k2 * (v(a) + v(b)));   n = n + 1
 *     w = exp(-max(0, S / (3.0 * n)));   W = W + w;   A.c = A.c + w * u.c(q)
 * and out.c(p) = A.c / W.  q = p always gives w = 1, so W >= 1; radius 0 returns the mean to the bit.  Where v(a) and v(b)
 * are both 0 a term is the squared difference over RTC_DENOISE_EPS: such a patch matches only patches equal to it, so a
 * tile that has taken one pass (P_t = 1) keeps its values unless another patch repeats them.  exp is the device library's:
 * results agree with a host restatement to 1e-12 * max(1, |value|).  Non-finite inputs propagate.
 *
 * rgba, where given, is the clamp of out: the bits of rtc_rgba8_device(out).
 */
typedef struct rtc_denoise_setting {
  uint32_t radius, patch; /* the search window is (2 radius + 1)^2 pixels, a patch (2 patch + 1)^2: at most the maxima above */
  double strength, cancel; /* k > 0: larger smooths more; the share of the variance taken out of a distance, >= 0 */
} rtc_denoise_setting;
/* (the defaults the scene loader and the Python binding use: radius 7, patch 2, strength 0.45, cancel 1.0) */
typedef struct rtc_denoise {
  const double *mean;          /* [vsize][hsize][3], required                                            */
  const double *sumsq;         /* [vsize][hsize], required: rtc_accum's / the adaptive state's           */
  uint32_t hsize, vsize;       /* >= 1; hsize * vsize <= 2^40 as rtc_rgba8_device                        */
  uint32_t passes;             /* the passes behind every pixel; read when tile_passes is NULL: >= 2     */
  const uint32_t *tile_passes; /* or NULL; [T] device: an adaptive run's P_t, tiles numbered as there    */
  uint32_t tile_w, tile_h;     /* with tile_passes: 1 .. RTC_ADAPTIVE_MAX_TILE                           */
  rtc_denoise_setting setting;
  double *out;                 /* [vsize][hsize][3], required, must not overlap mean                     */
  uint32_t *rgba;              /* [vsize][hsize] or NULL: the clamp of out, rtc_rgba8_device's bits      */
} rtc_denoise;
/*
 * Enqueues the filter on `hip_stream` (not NULL; every pointer a device pointer of that stream's device).  Asynchronous;
 * the caller orders it after whatever wrote mean and sumsq.  RTC_ERR_INVALID_ARGUMENT before any HIP call, with nothing
 * launched, for: a NULL among d, mean, sumsq, out and the stream; a size of 0 or above 2^40 pixels; radius or patch above
 * its maximum; strength not finite or <= 0; cancel not finite or < 0; passes < 2 without tile_passes; a tile size outside
 * 1 .. RTC_ADAPTIVE_MAX_TILE with tile_passes; out overlapping mean.
 */
int rtc_denoise_device(const rtc_denoise *d, void *hip_stream);
/*
 * A denoised render with buffers of its own.  Synchronous, on the handle's own stream.  Without `adaptive`: sample passes
 * 0 .. passes - 1 (passes >= 2), each through rtc_scene_set_sample_pass, rtc_render_device and
 * rtc_scene_accumulate_device, and the handle's own sample pass is put back afterwards whatever happens.  With `adaptive`:
 * a run as rtc_render_adaptive's, with max_passes taken from the setting; `passes` is ignored.  Then rtc_denoise_device
 * (`setting` NULL: the defaults above) over the mean, the sums of squares and the passes (the run's P_t).  rgb_out
 * [vsize][hsize][3] (host) gets the filtered image, noisy_out (host, or NULL) the mean.  Every argument is checked before
 * the device is touched.  librtc_multi renders without it.
 */
int rtc_render_denoised(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth, uint32_t passes,
                        const rtc_adaptive *adaptive, const rtc_denoise_setting *setting, double *rgb_out, double *noisy_out);

/* ---- the film stage: exposure, bloom, tone curve, transfer and the 8-bit clamp over an image ---- */
#define RTC_FILM_MAX_RADIUS 32u
#define RTC_FILM_EPS 1e-10
#define RTC_FILM_CURVE_LINEAR 0
#define RTC_FILM_CURVE_REINHARD 1
#define RTC_FILM_CURVE_ACES 2
#define RTC_FILM_CURVE_HABLE 3
#define RTC_FILM_TRANSFER_LINEAR 0
#define RTC_FILM_TRANSFER_SRGB 1
#define RTC_FILM_TRANSFER_GAMMA 2
/*
 * An image-space output stage, the last link of render -> accumulate -> (denoise) -> film -> RGBA8: it takes a scene-referred
 * image `in` ([vsize][hsize][3], linear radiance, values above 1.0 expected) to display values.  No render kernel is involved
 * and no scene is needed.  Every operation is an IEEE double operation in the order written (no fused multiply-add);
 * max(0, x) is x > 0 ? x : 0.  Y(c) = (0.2126 * c.r + 0.7152 * c.g) + 0.0722 * c.b.  For a pixel p, with n = hsize * vsize:
 *
 * 1. Exposure E.  With auto_key == 0, E = exposure.  Otherwise E = (exposure * auto_key) / exp(T / n), where T is the sum
 *    over all n pixels q of log(RTC_FILM_EPS + max(0, Y(in(q)))).  The order of that one sum is the implementation's: it
 *    is a function of n alone, so the bits are the same on every run and every device, and it uses no floating-point atomics.
 *    exp and log are the device library's.  E stays on the device: no host synchronisation happens inside the call.
 * 2. The exposed image: x(p).c = E * in(p).c.
 * 3. Bloom, only where bloom_radius >= 1 and bloom_intensity > 0, with R = bloom_radius:
 *        y = Y(x(p));  w = max(0, y - bloom_threshold) / (y > RTC_FILM_EPS ? y : RTC_FILM_EPS);  b(p).c = x(p).c * w
 *    The weights are formed on the host in doubles and handed to the kernels by value:
 *        raw[i] = exp(-(double)(i * i) / (2.0 * sigma * sigma)) for i = 0 .. R
 *        norm = raw[0], then norm = norm + 2.0 * raw[i] for i ascending;  g[i] = raw[i] / norm
 *    Rows: H(x, y).c = the sum, from 0.0, over i = -R .. R ascending of g[|i|] * b(x + i, y).c; terms whose column lies
 *    outside the image are left out.  Columns: B(x, y).c = the sum likewise over j of g[|j|] * H(x, y + j).c.  Light that
 *    leaves the frame is lost: there is no renormalisation.  (An implementation may add +0.0 where a term is left out: only
 *    the sign of a zero can differ, and no comparison here tells the two apart.)
 * 4. Combine: c = x(p).c + bloom_intensity * B(p).c; without bloom c = x(p).c.
 * 5. Curve, per channel.  LINEAR: t = c.  REINHARD: t = (c * (1.0 + c / (white * white))) / (1.0 + c).
 *    ACES (Narkowicz's fit): t = (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14).
 *    HABLE: f(v) = ((v * (0.15 * v + 0.05) + 0.004) / (v * (0.15 * v + 0.5) + 0.06)) - 0.02 / 0.3 and t = f(c) / f(white);
 *    f(white) is formed on the host.
 * 6. Transfer, per channel.  LINEAR: o = t.  SRGB: o = t <= 0.0031308 ? 12.92 * t : 1.055 * pow(t, 1.0 / 2.4) - 0.055.
 *    GAMMA: o = t > 0 ? pow(t, 1.0 / gamma) : 0.0.
 * 7. out(p).c = o; rgba(p), where wanted, is the clamp of out: the bits of rtc_rgba8_device(out).
 *
 * Non-finite inputs propagate (but GAMMA's t > 0 test takes a NaN to 0.0).  The setting {1, 0, no bloom, LINEAR, ., LINEAR, .}
 * returns `in` to the bit.  With manual
 * exposure and a LINEAR transfer no library function is involved: every kernel form and a host restatement give the same
 * bits.  With pow, or with the automatic exposure, results agree with a host restatement to 1e-12 * max(1, |value|).
 */
typedef struct rtc_film_setting {
  double exposure;        /* finite, > 0: a linear multiplier                                   */
  double auto_key;        /* finite, >= 0; 0 is off: the log-average luminance is taken to it   */
  uint32_t bloom_radius;  /* 0 .. RTC_FILM_MAX_RADIUS; 0 is no bloom                            */
  double bloom_sigma;     /* finite, > 0 where bloom_radius > 0                                 */
  double bloom_threshold; /* finite, >= 0                                                       */
  double bloom_intensity; /* finite, >= 0; 0 is no bloom                                        */
  uint32_t curve;         /* RTC_FILM_CURVE_*                                                   */
  double white;           /* finite, > 0; read by REINHARD and HABLE                            */
  uint32_t transfer;      /* RTC_FILM_TRANSFER_*                                                */
  double gamma;           /* finite, > 0; read by GAMMA                                         */
} rtc_film_setting;
/* (the defaults the scene loader and the Python binding use: exposure 1, auto_key 0, no bloom, curve ACES, white 4.0,
 * transfer SRGB, gamma 2.2; "bloom": true is radius 12, sigma 4.0, threshold 1.0, intensity 0.15) */
typedef struct rtc_film {
  const double *in;         /* [vsize][hsize][3], required                                                   */
  uint32_t hsize, vsize;    /* >= 1; hsize * vsize <= 2^40 as rtc_rgba8_device                               */
  rtc_film_setting setting;
  void *scratch;            /* rtc_film_scratch_bytes() bytes of device memory; may be NULL where that is 0  */
  double *out;              /* [vsize][hsize][3], required, must not overlap in                              */
  uint32_t *rgba;           /* [vsize][hsize] or NULL: the clamp of out, rtc_rgba8_device's bits             */
  double *scale_out;        /* device, or NULL: where E is written                                           */
} rtc_film;
/*
 * The bytes `scratch` must hold for a size and a setting: H, the partials of T and E.  0 where the setting needs none
 * (manual exposure without bloom); 0 with rtc_last_error set for a size or a setting the contract refuses.
 */
size_t rtc_film_scratch_bytes(uint32_t hsize, uint32_t vsize, const rtc_film_setting *s);
/*
 * Enqueues the film stage on `hip_stream` (not NULL; every pointer a device pointer of that stream's device).  Asynchronous;
 * the caller orders it after whatever wrote `in`; it makes no allocation.  RTC_ERR_INVALID_ARGUMENT before any HIP call,
 * with nothing launched, for: a NULL among f, in, out and the stream; a NULL scratch where bytes are needed; a size of 0 or
 * above 2^40 pixels; every out-of-range or non-finite field above; an unknown curve or transfer; out overlapping in.
 */
int rtc_film_device(const rtc_film *f, void *hip_stream);
/*
 * A filmed render with buffers of its own: the whole path on the handle's own stream, synchronous.  The accumulation
 * (passes >= 1) or the adaptive run is exactly rtc_render_denoised's, and the handle's own sample pass is put back
 * afterwards whatever happens.  Then rtc_denoise_device where `denoise` is not NULL (it needs passes >= 2 or `adaptive`),
 * then rtc_film_device (`film` NULL: the defaults above) over its result.  rgb_out [vsize][hsize][3] (host) gets the
 * film's out, rgba_out ([vsize][hsize][4] bytes, host) its clamp, linear_out (host) the image the film read; each may be
 * NULL, but not both rgb_out and rgba_out.  Every argument is checked before the device is touched.  librtc_multi renders
 * without it.
 */
int rtc_render_filmed(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth, uint32_t passes, const rtc_adaptive *adaptive,
                      const rtc_denoise_setting *denoise, const rtc_film_setting *film, double *rgb_out, uint8_t *rgba_out,
                      double *linear_out);

/* ---- robust accumulation: the Gini-weighted median of means over bucket sums ---- */
#define RTC_ROBUST_MAX_BUCKETS 15u
/*
 * An estimator for the accumulation that tells a firefly - one pass that returns 40 where the others return 0.5 - from signal:
 * the Gini-weighted median of means (GMoN) of Buisine, Delepoulle and Renaud (2021, "Firefly removal in Monte Carlo rendering
 * with adaptive Median of meaNs"), taken on luminance so that a pixel keeps its hue.  The passes of a run go round-robin into
 * M bucket sums; the resolve ranks the M bucket means of a pixel and keeps the central ones, more of them where the pixel is
 * calm and fewer where it is not.  No render kernel is involved and the resolve needs no scene.  Every operation is an IEEE
 * double operation in the order written (no fused multiply-add), and no library function is involved: every kernel form and
 * a host restatement give the same bits.
 *
 * Bucket sums.  `sums` is [M][n][3] doubles on the device, M = setting.buckets.  Pass p (0-based) of a run goes to bucket
 * p % M.  This needs no kernel of its own: it is rtc_scene_accumulate_device with sum = sums + (p % M) * n * 3,
 * passes = p / M + 1 (so a bucket's first pass overwrites it) and sumsq, mean, rgba and noise all NULL.  After P >= M passes
 * bucket j holds n_j = P / M + (j < P % M ? 1 : 0) frames.
 *
 * Resolve, per pixel, with h = (M - 1) / 2 and P = `passes`:
 * 1. Bucket means and keys: m_j.c = sums[j].c / (double)n_j;  y_j = (0.2126 * m_j.r + 0.7152 * m_j.g) + 0.0722 * m_j.b;
 *    k_j = (y_j - y_j == 0) ? (y_j > 0 ? y_j : 0.0) : +infinity.  A NaN or infinite bucket therefore sorts last.
 * 2. Rank: rank_j = the number of i != j with k_i < k_j || (k_i == k_j && i < j) - a permutation of 0 .. M - 1; ties go
 *    by bucket index.
 * 3. The Gini coefficient of the keys; every sum runs over j ascending from 0.0:
 *        T = sum k_j;   A = sum (double)(rank_j + 1) * k_j
 *        G0 = (T > 0 && T < infinity) ? (2.0 * A) / ((double)M * T) - (double)(M + 1) / (double)M : (T > 0 ? 1.0 : 0.0)
 *        g = gain * G0;   G = g > 0 ? (g < 1 ? g : 1.0) : 0.0
 * 4. The kept half-width: c = min(h, (uint32_t)floor((1.0 - G) * (double)h + 0.5)) and k = 2 c + 1; bucket j is kept where
 *    h - c <= rank_j <= h + c.
 * 5. mean_out.c = (the sum over kept j ascending, from 0.0, of m_j.c) / (double)k;  rejected_out = M - k.
 * 6. The variance of that mean, for the denoiser: cv = c > 1 ? c : 1 and kv = 2 cv + 1; D = the sum over j ascending with
 *    h - cv <= rank_j <= h + cv, from 0.0, of ((d.r * d.r + d.g * d.g) + d.b * d.b) where d.c = m_j.c - mean_out.c;
 *        v = D / (3.0 * ((double)(kv - 1) * (double)kv))
 *        sumsq_out = P * ((u.r * u.r + u.g * u.g) + u.b * u.b) + (3.0 * ((P - 1.0) * P)) * v,   u = mean_out, P = (double)passes
 *    - the sum of squares a P-pass accumulation with this mean and this variance of the mean would hold: rtc_denoise_device
 *    called with mean_out, sumsq_out and passes = P recovers v up to rounding.
 * 7. rgba, where wanted, is the clamp of mean_out: the bits of rtc_rgba8_device(mean_out).
 *
 * What follows: non-finite passes in fewer than half of the buckets do not reach mean_out (with gain >= 1: T is infinite,
 * G0 is 1 and the median alone is kept).  With gain 0 every bucket is kept
 * and, with P a multiple of M, the result is the plain mean up to rounding; with P not a multiple of M the bucket means have
 * unequal weights and gain 0 is NOT the plain mean.  A large gain is the plain median of the bucket means.
 */
typedef struct rtc_robust_setting {
  uint32_t buckets; /* M: odd, 3 .. RTC_ROBUST_MAX_BUCKETS                                  */
  double gain;      /* finite, >= 0: 0 keeps every bucket, a large gain is the plain median */
} rtc_robust_setting;
/* (the defaults the scene loader and the Python binding use: buckets 5, gain 1.0) */
typedef struct rtc_robust {
  const double *sums;     /* [M][n][3], required: the bucket sums                                          */
  size_t n_pixels;        /* n: 1 .. 2^40                                                                   */
  uint32_t passes;        /* P >= M: the passes of the run, dealt to the buckets as above                   */
  rtc_robust_setting setting;
  double *mean_out;       /* [n][3], required, not inside sums                                              */
  double *sumsq_out;      /* [n] or NULL, not inside sums: what rtc_denoise_device takes as sumsq           */
  uint32_t *rejected_out; /* [n] or NULL: M - k, the buckets left out of a pixel                            */
  uint32_t *rgba;         /* [n] or NULL: the clamp of mean_out, rtc_rgba8_device's bits                    */
} rtc_robust;
/*
 * Enqueues the resolve on `hip_stream` (not NULL; every pointer a device pointer of that stream's device).  Asynchronous;
 * the caller orders it after whatever wrote sums; it makes no allocation.  Every output is written once and not read back.
 * RTC_ERR_INVALID_ARGUMENT before any HIP call, with nothing launched, for: a NULL among r, sums, mean_out and the stream;
 * n_pixels of 0 or above 2^40; buckets even or outside 3 .. RTC_ROBUST_MAX_BUCKETS; passes < buckets; gain not finite or
 * < 0; mean_out or sumsq_out lying inside sums.
 */
int rtc_robust_device(const rtc_robust *r, void *hip_stream);
/*
 * A robust render with buffers of its own: the whole path on the handle's own stream with one allocation, synchronous.
 * Sample passes 0 .. passes - 1 (passes >= the buckets; there is no adaptive run: tiles at different pass counts would need
 * buckets per tile) each go through rtc_scene_set_sample_pass, rtc_render_device, the ordinary
 * rtc_scene_accumulate_device (sum, sumsq and mean, as rtc_render_denoised's) and a second rtc_scene_accumulate_device into
 * the pass's bucket; the handle's own sample pass is put back afterwards whatever happens.  Then rtc_robust_device (`robust`
 * NULL: the defaults above); then, where `denoise` is not NULL, rtc_denoise_device over mean_out, sumsq_out and passes; then,
 * where `film` is not NULL, rtc_film_device over that - here NULL means NO film stage, unlike rtc_render_filmed, where it
 * means the defaults.  rgb_out [vsize][hsize][3] (host) gets the last stage's image, rgba_out ([vsize][hsize][4] bytes, host)
 * its clamp, robust_out (host) the robust mean, plain_out (host) the ordinary mean, rejected_out ([vsize][hsize] uint32_t,
 * host) the map of rejected buckets; each may be NULL, but not both rgb_out and rgba_out.  Every argument is checked before
 * the device is touched.  librtc_multi renders without it.
 */
int rtc_render_robust(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth, uint32_t passes,
                      const rtc_robust_setting *robust, const rtc_denoise_setting *denoise, const rtc_film_setting *film,
                      double *rgb_out, uint8_t *rgba_out, double *robust_out, double *plain_out, uint32_t *rejected_out);
void rtc_scene_destroy(rtc_scene *scene);

/*
 * A second handle on the SAME scene: shares the source's device copy of the scene (no upload, no BVH build; freed
 * with the last handle that uses it) and has a stream, launch counters, schedule and measurements of its own.  A
 * handle runs one frame at a time; independent frames - an orbit's, an animation's, a rank's share of a split frame,
 * which is too short to fill a GPU by itself - go to a handle and its clones in turn, each on a stream of its own,
 * and the work-groups of a frame start on the CUs the frame before has left (bench.py --inflight, rtc_multi.h's
 * RTC_MULTI_FRAMES).  Same device as the source (made current here); either may be destroyed first.
 */
int rtc_scene_clone(const rtc_scene *source, rtc_scene **out);

/*
 * Replaces Camera.render (camera.zig:80-125) for the tile [x0,x0+w) x [y0,y0+h):
 * rgb_out[(y-y0)*w + (x-x0)][0..2] = colorAt(rayForPixel(x,y), max_depth).
 * The reference value of max_depth is 5 (camera.zig:118).  `rgb_out` is host
 * memory, [h][w][3] doubles.  Synchronous, and without side effects on the
 * caller's memory: the frame is copied into `rgb_out`, nothing is remembered
 * about the pointer.  (Into pageable memory that copy runs at a fifth of the
 * link's rate; see rtc_canvas_register.)  The copy of a frame takes as long as
 * its render or longer, so a large frame (from 400 000 pixels) is rendered in
 * two or four horizontal bands one after the other, each copied while the next
 * renders (1080p into a registered canvas: 1.1 ms instead of 1.45; the lower
 * bands run on clones of the handle, made on first use; rtc_get_stats sums the
 * bands; option "host_bands" forces the count).
 */
int rtc_render(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth,
               uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, double *rgb_out);

/*
 * Optional, for a host that renders frame after frame into ONE canvas (the interactive seam, lib.zig:135-190): pins
 * the caller's buffer for the HIP runtime (hipHostRegister), so that rtc_render's / rtc_multi_render's copy into it
 * runs at link speed (1080p: 1.1 ms per call instead of 3.8-5.6).  Explicit on purpose: the registration belongs to the
 * MEMORY, not to a scene handle, and the caller - who knows when the canvas is freed - drops it with
 * rtc_canvas_unregister BEFORE freeing or reallocating the buffer.  Both are process-wide and need no scene.
 */
int rtc_canvas_register(void *canvas, size_t bytes);
int rtc_canvas_unregister(void *canvas);

/*
 * The same frame as the RGBA8 framebuffer of the reference's interactive seam (Renderer, src/lib.zig:135-164):
 * rgba_out[((y-y0)*w + (x-x0))*4 + 0..2] = clamp(channel) of src/raytracer/color.zig:61-71 (@round of
 * channel * 255, clamped to 0..255), [+3] = 255.  Clamped on the device: 4 bytes per pixel cross the link
 * instead of 24.  `rgba_out` is host memory, [h][w][4] bytes.  Synchronous.
 */
int rtc_render_rgba8(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth,
                     uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint8_t *rgba_out);

/* The clamp alone, device to device: d_rgba[i] = R | G << 8 | B << 16 | 255 << 24 of pixel i of an [n_pixels][3] f64
 * canvas on the current device; asynchronous on `hip_stream` (not NULL).  Needs no scene. */
int rtc_rgba8_device(const double *d_canvas, size_t n_pixels, uint32_t *d_rgba, void *hip_stream);

/*
 * Same, but `d_rgb_out` is device memory on the scene's device and the work is
 * enqueued on `hip_stream` (a hipStream_t; NULL = the handle's own stream, which
 * is made at the first call that needs it: a host that always passes its streams
 * keeps the device's few hardware queues for them - INTEGRATION.md, "Streams and
 * hardware queues") without synchronising.  This is the entry point the multi-GPU driver uses
 * with device buffers owned by its RCCL communicator.
 */
int rtc_render_device(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth,
                      uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                      double *d_rgb_out, void *hip_stream);

/*
 * Multi-GPU tile partition: the image is cut into tile_w x tile_h tiles
 * numbered row-major; this call renders tiles first_tile, first_tile+stride,
 * ... (n_my_tiles of them) into the compact buffer
 * d_rgb_out[k][tile_h][tile_w][3]; pixels of edge tiles that fall outside the
 * image are NOT written (the library never clears the caller's buffer: zero it
 * once if the padding is read, e.g. by a gather).  Asynchronous on `hip_stream`
 * like rtc_render_device.
 */
int rtc_render_tiles_device(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth,
                            uint32_t tile_w, uint32_t tile_h, uint32_t first_tile,
                            uint32_t tile_stride, uint32_t n_my_tiles,
                            double *d_rgb_out, void *hip_stream);

/*
 * The same with an explicit list of tiles (host memory, copied): region k of d_rgb_out is tile tiles[k].  This is
 * what a cost-balanced split uses (rtc_assign_tiles below); a handle keeps the last list on the device, so
 * rendering the same list again copies nothing.
 */
int rtc_render_tile_list_device(rtc_scene *scene, const rtc_camera *cam, uint32_t max_depth,
                                uint32_t tile_w, uint32_t tile_h, const uint32_t *tiles,
                                uint32_t n_my_tiles, double *d_rgb_out, void *hip_stream);

/*
 * What the regions (tiles) of the most recent MEASURING tile-mode render on this handle took, in the library's
 * wave-time units (only ratios mean anything): cost_out[k] for region k.  A render measures when its schedule
 * was not measured on its own view, i.e. the first frame of a tile list and every frame of a moving camera.
 * Synchronises.  RTC_ERR_INVALID_ARGUMENT if there is no such measurement of n_regions regions.
 */
int rtc_get_tile_costs(rtc_scene *scene, double *cost_out, uint32_t n_regions);

/*
 * Cost-balanced split of the image's tiles over `world` ranks (host only, deterministic: every rank that calls it
 * with the same costs gets the same table): longest tile first onto the least-loaded rank that still has a free
 * slot, every rank holding at most padded = ceil(n_tiles / world) tiles so that one equal-count gather moves
 * them.  rank_of_tile[t] = the rank that renders tile t; slot_of_tile[t] = rank * padded + k, the tile's place in
 * the gathered buffer [world][padded][tile_h][tile_w][3] (a rank renders its tiles in increasing tile order).
 */
int rtc_assign_tiles(const double *tile_cost, uint32_t n_tiles, uint32_t world,
                     uint32_t *rank_of_tile, uint32_t *slot_of_tile);

/* rtc_assemble_tiles_device for such a split: d_slot_of_tile is rtc_assign_tiles' table in device memory. */
int rtc_assemble_tile_list_device(const double *d_gathered, const uint32_t *d_slot_of_tile,
                                  uint32_t tile_w, uint32_t tile_h, uint32_t hsize, uint32_t vsize,
                                  double *d_canvas, void *hip_stream);

/* The same for shares that were clamped before they were gathered (rtc_rgba8_device on a rank's tile buffer: 4 bytes
 * per pixel cross the links instead of 24 - an 8-GPU host of lib.zig's RGBA8 framebuffer is otherwise bound by the gather,
 * not the render): d_gathered_rgba[world][padded][tile_h][tile_w] -> d_rgba[vsize][hsize]. */
int rtc_assemble_tile_list_rgba8_device(const uint32_t *d_gathered_rgba, const uint32_t *d_slot_of_tile,
                                        uint32_t tile_w, uint32_t tile_h, uint32_t hsize, uint32_t vsize,
                                        uint32_t *d_rgba, void *hip_stream);

/*
 * Rank 0 of the tile partition, after the gather: copies the ranks' compact tile
 * buffers d_gathered[world][padded_tiles][tile_h][tile_w][3] (rank r's k-th tile
 * is tile r + k * world of the row-major tiling) into the row-major canvas
 * d_canvas[vsize][hsize][3].  Device to device on the current device,
 * asynchronous on `hip_stream` (which must not be NULL).  Needs no scene.
 * Replaces the row-major Canvas the reference fills in place (camera.zig:121).
 */
int rtc_assemble_tiles_device(const double *d_gathered, uint32_t world, uint32_t padded_tiles,
                              uint32_t tile_w, uint32_t tile_h, uint32_t hsize, uint32_t vsize,
                              double *d_canvas, void *hip_stream);

/*
 * A rank's compact tiles (as rtc_render_tile_list_device leaves them: d_tiles[k] is tile d_tile_list[k]) written
 * straight to their places in a row-major canvas [vsize][hsize][3] - `canvas` being any memory the current device can
 * write: device memory, or the caller's host canvas after rtc_canvas_register (pinned and mapped).  With a registered
 * host canvas every GPU of a split frame sends its own share over its own host link; nothing funnels through rank 0
 * (rtc_multi.h does this for its host forms).  Pixels of edge tiles outside the image are skipped.  The _rgba8 form
 * clamps on the way (color.zig:61-71) into [vsize][hsize] RGBA8.  d_tile_list is device memory.  Asynchronous on
 * `hip_stream` (not NULL), on the current device.  Needs no scene.  Replaces Canvas writes of camera.zig:119-121.
 */
int rtc_scatter_tile_list_device(const double *d_tiles, const uint32_t *d_tile_list, uint32_t n_tiles, uint32_t tile_w,
                                 uint32_t tile_h, uint32_t hsize, uint32_t vsize, double *canvas, void *hip_stream);
int rtc_scatter_tile_list_rgba8_device(const double *d_tiles, const uint32_t *d_tile_list, uint32_t n_tiles,
                                       uint32_t tile_w, uint32_t tile_h, uint32_t hsize, uint32_t vsize, uint32_t *rgba,
                                       void *hip_stream);

/* Waits for the work enqueued on the handle's own stream (nothing to wait for if it has never used one). */
int rtc_scene_synchronize(rtc_scene *scene);

/* Counters of the last render that was enqueued on this handle (synchronises). */
int rtc_get_stats(rtc_scene *scene, rtc_stats *out);

/*
 * For callers of the asynchronous entry points, after a frame whose rtc_stats::overflow is not 0 on a scene with csg
 * nodes (Csg.filterIntersections' list, csg.zig:51-95, is of any length in the reference; a lane's list here is a
 * buffer): waits for the handle's last launch and, if what ran out was a csg intersection list, sizes the handle's lists
 * for what that frame needed (in one step, up to 1024 entries).  RTC_OK: the lists are longer now (or nothing had
 * overflowed) - render the frame again; RTC_ERR_OVERFLOW: the overflow was not a csg list's, or the lists are at their
 * maximum; RTC_ERR_OUT_OF_MEMORY (at the next render): the longer lists do not fit, the handle keeps the old ones.
 * rtc_render and rtc_render_rgba8 do this by themselves.
 */
int rtc_grow_csg_lists(rtc_scene *scene);

/* (Diagnostics and tuning - rtc_set_option, rtc_get_schedule, rtc_get_chunk_times, rtc_last_kernel_name - are declared in
 * rtc_diag.h: a host that binds the render path does not need them.) */

/* Thread-local, static storage; "" when the last call on this thread succeeded. */
const char *rtc_last_error(void);
/* "NotInvertible", "OutOfMemory", ... (Zig error-name style, cf. lib.zig:226-227). */
const char *rtc_status_name(int status);

#ifdef __cplusplus
}
#endif
#endif /* RTC_H */
