// rtc_kernels.hip — the per-pixel hot path of SinclaM/ray-tracer-challenge as ONE
// hand-written FP64 megakernel for gfx950 (MI355X, wave64).
//
// Replaces, per pixel (all file:line citations are into /root/reference/src/raytracer):
//   Camera.rayForPixel                      camera.zig:64-76
//   World.colorAt                           world.zig:111-121
//   World.intersect + sort + hit            world.zig:71-83, shapes/shape.zig:64-80
//   Shape.intersect (per-leaf ray xform)    shapes/shape.zig:313-335
//   Sphere/Plane/Cube/Cylinder/Cone/Triangle/SmoothTriangle.localIntersect
//   Group.localIntersect + BoundingBox      shapes/group.zig:39-62, bounding_box.zig:112-165
//   PreComputations.new / schlick           world.zig:212-289
//   World.shadeHit / isShadowed             world.zig:86-154
//   Material.lighting, Pattern.patternAt    material.zig:40-74, patterns/*.zig
//   World.reflectedColor / refractedColor   world.zig:157-189
//
//   Csg.localIntersect / filterIntersections shapes/csg.zig:51-95      (the *_ext kernels)
//   Perturb + noise, TextureMap / UvPattern  patterns/perturb.zig, noise.zig, patterns/texture_map.zig
//
// Design (MI355X-first, not a translation of the reference's control flow):
//   * persistent waves pull PACKETS of pixels from an atomic counter and deal them to idle lanes; one ray per
//     lane per iteration; the reflection/refraction recursion is an explicit per-lane stack of
//     (ray, weight, remaining) entries in a line-per-entry buffer, colour accumulated top-down; idle lanes take
//     the oldest pending ray of busy neighbours through an LDS mailbox;
//   * the reference builds, sorts and scans a heap-allocated list of ALL intersections for
//     every ray (and again for every shadow ray).  Here the three things that list is used
//     for are computed by streaming reductions over exactly the same candidate set:
//       - the hit   = min over entries with t >= 0 of (t, depth-first leaf index),
//       - shadowed  = exists entry with 0 <= t < distance on a shadow-casting leaf,
//       - n1 / n2   = refractive index of the "open" leaf whose last entry before the hit
//                     comes latest (see BehindVisitor), which is what the containers walk
//                     of world.zig:229-255 evaluates to;
//   * top-level World.objects: tables staged in LDS, an FP32 pass over all of them (world boxes, or bounding spheres in the
//     kernels of worlds that are mostly spheres), then each
//     lane runs the exact FP64 test on its own survivors; groups: a candidate BVH (FP32, world space) proposes
//     leaves, and a proposed leaf counts only if the ray passes the reference's own box test of every Group
//     above it (chain_ok), so the entries that reach the reductions are exactly the reference's;
//   * arithmetic is FP64 in the reference's evaluation order and this file is compiled with
//     -ffp-contract=off (the reference's Zig float mode is strict: no FMA contraction), so
//     every t, point and normal is bit-identical to the CPU restatement; pow() (specular, schlick)
//     follows Zig's std.math.pow algorithm (zig_pow below).  No MFMA: nothing here is a dense contraction.
#include "rtc_device.h"

#include <type_traits>

// Diagnostic build only (-DRTC_PROFILE): wave time per section of the main loop, from s_memtime stamps,
// summed into DevStats::prof.  Never defined in the shipped library; numbers from such a build are
// shares, not run times (MI355X guide, "In-kernel stamps").
// -DRTC_PROFILE -DRTC_PROFILE_LITE: only the per-wave log (lifetime, packets, time of the last fetch - DevStats::prof_log)
// and the walk counters' bounds checks; no section stamps, so the frame runs at nearly its product speed.
#if defined(RTC_PROFILE) && defined(RTC_PROFILE_LITE)
#define RTC_STAMP(sec)                                                     \
  do {                                                                     \
    if ((sec) == 7) prof_t = __builtin_amdgcn_s_memtime();                 \
    (void)prof_sec;                                                        \
  } while (0)
#define RTC_COUNT(slot) do { } while (0)
#define RTC_HIST_BEGIN() do { } while (0)
#define RTC_HIST_END(kind) do { } while (0)
#elif defined(RTC_PROFILE)
#define RTC_STAMP(sec)                                                     \
  do {                                                                     \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();          \
    prof_acc[prof_sec] += now_ - prof_t;                                   \
    prof_t = now_;                                                         \
    prof_sec = (sec);                                                      \
  } while (0)
#define RTC_COUNT(slot)                                                                 \
  do {                                                                                  \
    prof2[slot] += 1ull;                                                                \
    prof2[(slot) + 1] += static_cast<unsigned long long>(__builtin_popcountll(__ballot(true))); \
  } while (0)
// wave cycles spent in traces, by how many lanes had a ray: [kind 0 closest / 1 shadow / 2 behind][1-2, 3-4, 5-8, 9-16, 17-32, 33-48, 49-64]
#define RTC_HIST_BEGIN()                                                                      \
  const unsigned hist_n_ = static_cast<unsigned>(__builtin_popcountll(__ballot(true)));        \
  const unsigned long long hist_t_ = __builtin_amdgcn_s_memtime()
#define RTC_HIST_END(kind)                                                                                          \
  prof3[(kind) * 7 + (hist_n_ <= 2 ? 0 : hist_n_ <= 4 ? 1 : hist_n_ <= 8 ? 2 : hist_n_ <= 16 ? 3 : hist_n_ <= 32 ? 4 : hist_n_ <= 48 ? 5 : 6)] += \
      __builtin_amdgcn_s_memtime() - hist_t_
#else
#define RTC_STAMP(sec) do { } while (0)
#define RTC_COUNT(slot) do { } while (0)
#define RTC_HIST_BEGIN() do { } while (0)
#define RTC_HIST_END(kind) do { } while (0)
#endif

#if defined(RTC_PROFILE) && defined(RTC_PROFILE_LITE)
__shared__ DevStats* rtc_prof_stats;
#define RTC_WALK_ADD(slot, n) do { (void)(n); } while (0)
#define RTC_AUX_ADD(slot, n) do { (void)(n); } while (0)
#define RTC_KIND_ADD(slot, n) do { (void)(n); } while (0)
#define RTC_CUBE_ADD(slot, n) do { (void)(n); } while (0)
#elif defined(RTC_PROFILE)
__shared__ DevStats* rtc_prof_stats;
// (diagnostic builds: the walks' counts and cycles - DevStats::prof4, prof5, prof6 - are summed per wave in LDS
// by the first active lane and added to the launch's counters when the wave ends: with an atomic per count and walk on
// eight words of memory the diagnostic frame was eleven times the product's)
__shared__ unsigned long long rtc_prof_counts[4][58];
#define RTC_PROF_ADD_(slot, n)                                                                                        \
  do {                                                                                                                 \
    const unsigned long long n_ = static_cast<unsigned long long>(n);                                                  \
    if (__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(__ballot(true) >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(__ballot(true)), 0u)) == 0u) \
      rtc_prof_counts[threadIdx.x >> 6][slot] += n_;                                                                   \
  } while (0)
#define RTC_WALK_ADD(slot, n) RTC_PROF_ADD_(slot, n)
#define RTC_AUX_ADD(slot, n) RTC_PROF_ADD_(8 + (slot), n)
#define RTC_KIND_ADD(slot, n) RTC_PROF_ADD_(16 + (slot), n)
#define RTC_CUBE_ADD(slot, n) RTC_PROF_ADD_(40 + (slot), n)
#else
#define RTC_WALK_ADD(slot, n) do { } while (0)
#define RTC_AUX_ADD(slot, n) do { } while (0)
#define RTC_KIND_ADD(slot, n) do { } while (0)
#define RTC_CUBE_ADD(slot, n) do { } while (0)
#endif

// Diagnostic builds (-DRTC_PROFILE) also check what the render kernels index against what was allocated for it: an
// access outside is counted in DevStats::oob by kind (RTC_OOB_*, printed by rtc_get_stats) and not made - the index
// becomes 0 or the access is skipped.  A check never traps.  In the product build RTC_IN_BOUNDS is `true` and
// RTC_CHECK_INDEX the index itself.
#ifdef RTC_PROFILE
// what the launch's root loop and shading may index: root records, sphere pairs, box pairs, materials, patterns, light
// words - the tables in memory as allocated, or what the staging copies put into LDS
__shared__ uint32_t rtc_oob_avail[6];
__device__ __forceinline__ bool rtc_in_bounds(uint32_t kind, bool ok) {
  if (!ok) atomicAdd(&rtc_prof_stats->oob[kind], 1ull);
  return ok;
}
#define RTC_IN_BOUNDS(kind, ok) rtc_in_bounds(kind, ok)
#define RTC_CHECK_INDEX(kind, i, n) (rtc_in_bounds(kind, (i) < (n)) ? (i) : 0u)
#define RTC_AVAIL(k) rtc_oob_avail[k]
#else
#define RTC_IN_BOUNDS(kind, ok) true
#define RTC_CHECK_INDEX(kind, i, n) (i)
#endif

// Bound experiments (WRONG images, right dependency chains; never set in the product): bit 0: no shadow ray is traced;
// bit 1: the walks of shadow rays visit no leaf (what their node phase alone costs); bit 2: triangles are tested in FP32
// (what VERDICT r04 item 2's pre-test could save at the very most: every exact test replaced, not a survivor left).
#ifndef RTC_EXPERIMENT
#define RTC_EXPERIMENT 0
#endif

// ---- round 5's build switches: 1 = as shipped, 0 = the kernels without it (A/B builds: tools/variants.py "x=-DRTC_...=0") ----
#ifndef RTC_ROOT_NODE_IN_REC
#define RTC_ROOT_NODE_IN_REC 1  // a group's World.objects record carries a copy of the root node of its candidate BVH (traverse_bvh8)
#endif
#ifndef RTC_ALL_SOLID_FORM
#define RTC_ALL_SOLID_FORM 1    // a world of solid colours takes a hit's colour from its material (render_body, SOLID_PATH)
#endif
#ifndef RTC_CULL_HALF_STEP
#define RTC_CULL_HALF_STEP 1    // phase 1 of the root loop: a remainder of one or two roots is one record's work (trace())
#endif
#ifndef RTC_PLANE_EARLY_OUT
#define RTC_PLANE_EARLY_OUT 1   // a plane test decides 0 <= t < limit without its quotient where that is exact (trace(), leaf_of_kind)
#endif
#ifndef RTC_ROOM_EARLY_OUT
#define RTC_ROOM_EARLY_OUT 1    // shadow rays inside a cube that contains every light (segment_stays_inside_cube)
#endif
#ifndef RTC_CUBE_BEHIND_EARLY_OUT
#define RTC_CUBE_BEHIND_EARLY_OUT 1  // shadow traces of the simple kernels that cull by boxes skip a cube behind the ray's origin (cube_entirely_behind)
#endif
#ifndef RTC_SPECULAR_SKIP
#define RTC_SPECULAR_SKIP 1          // the simple kernels skip the specular power of a point light in a wave none of whose lanes' materials has a specular term (render_body, kSpecularSkip)
#endif
#ifndef RTC_ROOTS32
#define RTC_ROOTS32 1                // rtc_render_kernel_simple3_b, whose worlds have at most RTC_LDS3_ROOTS roots: its closest-hit and shadow traces run one block of the root loop with a 32-bit survivor mask, phase 1's bits shifted in as they are formed (trace(), MAX_ROOTS; render_body, ROOTS)
#endif
#ifndef RTC_CONTAINERS_SOLIDS
#define RTC_CONTAINERS_SOLIDS 1      // simple worlds: the containers pass drops a solid whose bound lies behind the origin and a plane whose entry cannot be negative (trace(), kSolids)
#endif
#ifndef RTC_CONTAINERS_OWN_ROOT
#define RTC_CONTAINERS_OWN_ROOT 1    // rtc_render_kernel_simple_b and _simple3_b: a wave all of whose transparent hits lie on roots that are alone (RTC_ROOT_ALONE) takes n1 / n2 from each hit root's own two entries instead of the whole containers pass (render_body, kOwnRoot; trace(), OWN)
#endif
#ifndef RTC_SHARED_NORMALIZE
#define RTC_SHARED_NORMALIZE 1       // rtc_render_kernel_simple, _simple_b and _simple3_b divide a vector's three components by its magnitude with one refined reciprocal where a whole wave's operands allow it (shared_normalize; render_body, kSharedNormalize)
#endif
// Wave priority by phase of the iteration (s_setprio, round 5; profiles/r05/wave_priority.md).  The three waves of a SIMD
// are at different places of the same loop; which of them issues when more than one could is the arbiter's choice, and
// with equal priorities it serves them alike.  Here a wave says what it is doing: fetching work (RTC_PRIO_DEAL: popping its
// stacks, the LDS mailbox, claiming and reading the next packet - short, serial, and what every lane of the wave waits
// for) goes first; the two phases that are FP32 arithmetic on data that is being waited for (phase 1 of the root loop,
// RTC_PRIO_CULL; the node steps of a BVH walk, RTC_PRIO_NODE) go last; the exact FP64 tests and the shading in between
// (RTC_PRIO_WORK).  Only the order matters (levels 1 / 2 / 3 for the middle measured the same); a fixed priority per
// work-group instead starves waves (cover + 16 %).  cover - 3.1 %, reflection_and_refraction - 4.7 %, cubes - 3.5 %,
// dragons 4K - 2.5 %, teapot - 3.8 %, nefertiti - 5.5 %.  -DRTC_SETPRIO=0 builds the kernels without it.
#ifndef RTC_SETPRIO
#define RTC_SETPRIO 1
#endif
#ifndef RTC_PRIO_DEAL
#define RTC_PRIO_DEAL 3
#endif
#ifndef RTC_PRIO_WORK
#define RTC_PRIO_WORK 1
#endif
#ifndef RTC_PRIO_CULL
#define RTC_PRIO_CULL 0
#endif
#ifndef RTC_PRIO_NODE
#define RTC_PRIO_NODE 0
#endif
#ifndef RTC_PRIO_CULL_SPHERES
#define RTC_PRIO_CULL_SPHERES 3  // (the simple kernels that cull by spheres: reflection_and_refraction's handles settle 1.36-1.38 ms
#endif                         //  instead of 1.37-1.43 with the phase at 0; the other worlds on these kernels +- 0.5 %)
#if RTC_SETPRIO
#define RTC_PRIO_PHASE(x) __builtin_amdgcn_s_setprio(x)
#else
#define RTC_PRIO_PHASE(x) ((void)0)
#endif
#ifndef RTC_LB2
#define RTC_LB2 2  // minimum waves per SIMD the register allocator must leave room for
#endif

namespace {

constexpr double kInf = __builtin_huge_val();

struct Ray {
  double ox, oy, oz, dx, dy, dz;
};

// Zig @max/@min return the non-NaN operand (IEEE maxNum/minNum) == v_max_f64/v_min_f64.
__device__ __forceinline__ double zmax(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ double zmin(double a, double b) { return __builtin_fmin(a, b); }

// Matrix.tupleMul (matrix.zig:124-140) on rows 0..2 of an affine matrix: a row dot is
// ((m0*x + m1*y) + m2*z) + m3*w; w == 1 for points (m3*1 is exact) and w == 0 for vectors
// (the term is an exact +0 and is dropped).
__device__ __forceinline__ double row_pt(const double* __restrict__ m, double x, double y, double z) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}
__device__ __forceinline__ double row_vec(const double* __restrict__ m, double x, double y, double z) {
  return (m[0] * x + m[1] * y) + m[2] * z;
}

// Ray.transform (ray.zig:30-32)
__device__ __forceinline__ Ray xform_ray(const double* __restrict__ m, const Ray& r) {
  Ray o;
  o.ox = row_pt(m + 0, r.ox, r.oy, r.oz);
  o.oy = row_pt(m + 4, r.ox, r.oy, r.oz);
  o.oz = row_pt(m + 8, r.ox, r.oy, r.oz);
  o.dx = row_vec(m + 0, r.dx, r.dy, r.dz);
  o.dy = row_vec(m + 4, r.dx, r.dy, r.dz);
  o.dz = row_vec(m + 8, r.dx, r.dy, r.dz);
  return o;
}

// cube.zig:24-47 / bounding_box.zig:112-137
__device__ __forceinline__ void check_axis(double origin, double direction, double mn, double mx, double& tmin,
                                           double& tmax) {
  const double tmin_numerator = mn - origin;
  const double tmax_numerator = mx - origin;
  if (__builtin_fabs(direction) >= 1e-5) {
    tmin = tmin_numerator / direction;
    tmax = tmax_numerator / direction;
  } else {
    tmin = tmin_numerator * kInf;
    tmax = tmax_numerator * kInf;
  }
  if (tmin > tmax) {
    const double save = tmax;
    tmax = tmin;
    tmin = save;
  }
}

// cube.zig:49-79 / bounding_box.zig:139-165; returns false on a miss (tmin > tmax).
__device__ __forceinline__ bool slab(const Ray& r, double mnx, double mny, double mnz, double mxx, double mxy,
                                     double mxz, double& tmin, double& tmax) {
  double xtmin, xtmax, ytmin, ytmax, ztmin, ztmax;
  check_axis(r.ox, r.dx, mnx, mxx, xtmin, xtmax);
  check_axis(r.oy, r.dy, mny, mxy, ytmin, ytmax);
  check_axis(r.oz, r.dz, mnz, mxz, ztmin, ztmax);
  tmin = zmax(xtmin, zmax(ytmin, ztmin));
  tmax = zmin(xtmax, zmin(ytmax, ztmax));
  return !(tmin > tmax);
}

// Two quotients by the same divisor, as a cube axis needs them (cube.zig:28-33: tmin_numerator / direction and
// tmax_numerator / direction).  The compiler expands x / d into v_div_scale x2, v_rcp_f64, four v_fma refining the
// reciprocal, v_mul, v_fma, v_div_fmas, v_div_fixup: eleven instructions, seven of which depend on d alone.  Where
// neither v_div_scale rescales its operands nor v_div_fixup overrides the result - |d| in [1e-5, 2^200], x == 0 or
// |x| in [2^-53, 2^201]: far inside the hardware's conditions (quotient exponent within +-768, nothing denormal) - the
// sequence below IS that expansion with the d-only part computed once, so both quotients are bit-identical to x / d
// (checked against the plain division on 2^28 random and edge-case operand pairs: tests/hip/shared_divisor_check.hip).
__device__ __forceinline__ double refined_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(r, e, r);
}
__device__ __forceinline__ double quotient(double x, double d, double r) {
  const double q = x * r;
  return __builtin_fma(__builtin_fma(-d, q, x), r, q);
}

// Three quotients by one positive divisor, as Tuple.normalized needs them (tuple.zig:109-116: x / m, y / m, z / m with m
// the vector's magnitude, sqrt((x*x + y*y) + z*z), and m != 0 tested first).  The compiler expands the three divisions
// one by one, three v_rcp_f64 and 33 instructions; here the m-only part of the expansion is computed once, as above.
// Operand range - shared_normalize_ok() - in which neither v_div_scale rescales and v_div_fixup passes the result through
// except for the sign of a zero: m a normal number in [2^-200, 2^201) (its biased exponent within 1023 +- 200: an infinity
// or a NaN fails, and with it every vector that has an infinite or NaN component or a square that overflows), every
// numerator zero or at least 2^-801 in magnitude (v_frexp_exp yields 0 for a zero and less than -1022 for a denormal).
// No numerator exceeds m by more than a rounding, m being the magnitude: a quotient's exponent lies in [-1002, 1], far
// inside the hardware's conditions (numerator exponent above -969, quotient normal and below 2^768).
// v_div_fixup is also what gives a zero quotient its sign, and a cube's world normal does carry -0 components (a zero
// times a negative matrix entry): m > 0, so the numerator's sign IS the quotient's - copied on (v_bfi_b32), a no-op for
// every non-zero numerator.
// Checked against the plain divisions on 2^28 vectors, inside and outside the range: tests/hip/shared_normalize_check.hip,
// which carries a copy of these two functions - a change to one is a change to both.
__device__ __forceinline__ bool shared_normalize_ok(double x, double y, double z, double m) {
  const int lowest = min(min(__builtin_amdgcn_frexp_exp(x), __builtin_amdgcn_frexp_exp(y)), __builtin_amdgcn_frexp_exp(z));
  const uint32_t m_exponent = static_cast<uint32_t>(__builtin_bit_cast(uint64_t, m) >> 52);  // (a sign bit set: out of the band)
  return (lowest >= -800) & (m_exponent - (1023u - 200u) <= 400u);
}
__device__ __forceinline__ void shared_normalize(double& x, double& y, double& z, double m) {
  const double rcp = refined_rcp(m);
  x = __builtin_copysign(quotient(x, m, rcp), x);
  y = __builtin_copysign(quotient(y, m, rcp), y);
  z = __builtin_copysign(quotient(z, m, rcp), z);
}

// Cube.localIntersect's three checkAxis calls (cube.zig:24-47) for the unit cube.  The numerators are -1 - o and 1 - o:
// zero, or at least 2^-53 in magnitude; with every component of the ray below 2^200 the shared-divisor quotients above
// are exact.  A ray outside that range (or with a NaN) takes the plain divisions of slab().
__device__ __forceinline__ bool cube_slab(const Ray& r, double& tmin, double& tmax) {
  const double big = 0x1p200;
  const bool tame = (__builtin_fabs(r.ox) <= big) & (__builtin_fabs(r.oy) <= big) & (__builtin_fabs(r.oz) <= big) &
                    (__builtin_fabs(r.dx) <= big) & (__builtin_fabs(r.dy) <= big) & (__builtin_fabs(r.dz) <= big);
  if (!tame) return slab(r, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, tmin, tmax);
  auto axis = [&](double origin, double direction, double& lo, double& hi) {
    const double tmin_numerator = -1.0 - origin;
    const double tmax_numerator = 1.0 - origin;
    const double rcp = refined_rcp(direction);
    lo = quotient(tmin_numerator, direction, rcp);
    hi = quotient(tmax_numerator, direction, rcp);
    if (!(__builtin_fabs(direction) >= 1e-5)) {
      lo = tmin_numerator * kInf;
      hi = tmax_numerator * kInf;
    }
    if (lo > hi) {
      const double save = hi;
      hi = lo;
      lo = save;
    }
  };
  double xtmin, xtmax, ytmin, ytmax, ztmin, ztmax;
  axis(r.ox, r.dx, xtmin, xtmax);
  axis(r.oy, r.dy, ytmin, ytmax);
  axis(r.oz, r.dz, ztmin, ztmax);
  tmin = zmax(xtmin, zmax(ytmin, ztmin));
  tmax = zmin(xtmax, zmin(ytmax, ztmax));
  return !(tmin > tmax);
}

// A shadow ray that starts inside a cube and whose light is nearer than every face ahead of it: both of the cube's
// entries are irrelevant to it - tmin < 0, tmax > the light's distance - and both can be known WITHOUT the six quotients
// of cube_slab, exactly: the origin inside by 1e-9 (object space) puts a face behind it on every axis that is not
// "parallel" (each of those quotients is negative and no smaller than 1e-9 / 2^200: it cannot round to -0), and
// 1 -+ o > limit x |d| x (1 + 1e-12) puts the face ahead beyond the limit after rounding (see the plane's early-out); an
// axis the reference treats as parallel (|d| < 1e-5, or a NaN: cube.zig:28-35) gives -inf / +inf and constrains nothing.
// Run for the cubes rtc_scene_create marks as rooms (every light inside: teapot.json, nefertiti.json): for any other
// cube the three compares of `inside` would be paid by every test and fail.
__device__ __forceinline__ bool segment_stays_inside_cube(const Ray& r, double limit) {
  const double in = 1.0 - 1e-9;
  const bool inside = (__builtin_fabs(r.ox) <= in) & (__builtin_fabs(r.oy) <= in) & (__builtin_fabs(r.oz) <= in);
  auto clear = [&](double o, double d) {
    const double ad = __builtin_fabs(d);
    const double ahead = d > 0.0 ? 1.0 - o : 1.0 + o;  // to the face the ray travels towards
    return !(ad >= 1e-5) | (ahead > (limit * ad) * (1.0 + 1e-12));
  };
  return inside & clear(r.ox, r.dx) & clear(r.oy, r.dy) & clear(r.oz, r.dz);
}

// A ray that starts beyond one of a cube's faces and does not travel back towards it: the cube is behind it, and both of
// its entries - if it has any - are negative, which a closest-hit and a shadow trace ignore (V::kFrontOnly); known
// WITHOUT xform_ray's successors, the six quotients of cube_slab, exactly, by the reference's own arithmetic (cube.zig
// checkAxis, cube_slab above).  On an axis with o > 1:
//   * both numerators, -1 - o and 1 - o, are negative, and their signs are exact: o >= 1 + 2^-52, so 1 - o <= -2^-52
//     (a difference of neighbours is exact) and -1 - o <= -2;
//   * d >= 1e-5: both quotients are negative - and, with d <= 1e10, at least 2^-52 / 1e10 > 1e-26 in magnitude, far
//     from a quotient that underflows to -0, which `t >= 0` would let through (an infinite d gives exactly that);
//   * |d| < 1e-5, either sign (the reference's "parallel" rule): both are numerator x inf = -inf;
//   * so the axis's far parameter is negative, the cube's tmax - a minimum over the axes that ignores NaNs - is negative,
//     and tmin <= tmax or there is no entry at all.
// On an axis with o < -1 both numerators are positive (1 - o >= 2, -1 - o >= 2^-52), and only a direction that is not
// "parallel", d <= -1e-5, makes the quotients negative: the parallel rule multiplies by +inf whatever the sign of d, and
// a cube whose three axes all give +inf has both entries at t = +inf, which ClosestVisitor::entry's tie rule looks at.
// An infinite o gives -inf / d = -inf: nothing to guard.  A NaN in o or d compares false and the full test runs.
// The ray that leaves a cube's face at over_point - two shadow rays and a reflected ray per hit on cover.json's cubes -
// has that cube 1e-5 behind it, inside phase 1's FP32 margin: each of those traces ran the whole test on the cube it
// stands on.  The containers pass wants negative entries and never asks; a refracted ray starts inside the cube
// (under_point) and fails `|o| > 1` by itself.
// (The conditions are restated, not called, by the checks that hold them to the reference's arithmetic: `_predicate` in
// tests/test_cube_behind_cpu.py and `behind` in tests/cpp/cube_behind_check.cpp.  A change here is a change in all three.)
__device__ __forceinline__ bool cube_entirely_behind(const Ray& lr) {
  auto behind = [](double o, double d) {
    const double ad = __builtin_fabs(d);
    const bool above = (o > 1.0) & ((d >= 0.0) | (ad < 1e-5)), below = (o < -1.0) & (d <= -1e-5);
    return (above | below) & (ad <= 1e10);
  };
  return behind(lr.ox, lr.dx) | behind(lr.oy, lr.dy) | behind(lr.oz, lr.dz);
}

#ifdef RTC_TORUS_TU
// ------------------------------------------------------------------------------------------
// RTC_TORUS (rtc.h): the real roots of the ray's quartic by the derivative chain - the roots of
// q''/2 (closed form, one sqrt) split the search interval into pieces on which the cubic q' is monotone, its roots into
// pieces on which q is monotone.  + - * / sqrt and comparisons only, each correctly rounded, in the order rtc.h writes
// them: the CPU checker takes the same path, exit for exit.  Compiled into the torus kernels' translation unit only.
// The roots travel by value - five registers' worth of doubles and a count -, never through an array: a runtime-indexed
// array would live in scratch.
// ------------------------------------------------------------------------------------------
struct TorusRoots {
  double s0, s1, s2, s3;
  uint32_t n;
};
// appends x if the list has room and x is above its last entry (the list stays strictly ascending)
__device__ __forceinline__ void torus_push(TorusRoots& o, uint32_t cap, double x) {
  const double last = o.n == 1u ? o.s0 : (o.n == 2u ? o.s1 : (o.n == 3u ? o.s2 : o.s3));
  if (o.n >= cap || (o.n != 0u && !(x > last))) return;
  if (o.n == 0u) o.s0 = x;
  else if (o.n == 1u) o.s1 = x;
  else if (o.n == 2u) o.s2 = x;
  else o.s3 = x;
  ++o.n;
}
// One copy in the code object (as perlin_noise): not inlined, and both stages of the chain run the same loop body - a
// cubic is a quartic whose leading coefficient is 0.0 (0.0 * x + a3 is a3).
__device__ __noinline__ TorusRoots torus_quartic(double c4, double c3, double c2, double c1, double c0, double lo, double hi) {
  TorusRoots k{0.0, 0.0, 0.0, 0.0, 0u};
  if (!(lo < hi) || !(hi - lo < kInf)) return k;  // an empty or unbounded interval (or a NaN): no entries
  double a4 = 0.0, a3 = 4.0 * c4, a2 = 3.0 * c3, a1 = 2.0 * c2, a0 = c1;  // q'
  {
    const double q0 = 3.0 * a3, q1 = 2.0 * a2, q2 = a1;  // q''
    const double disc = q1 * q1 - (4.0 * q0) * q2;
    if (disc >= 0.0) {
      const double sq = __builtin_sqrt(disc);
      const double k0 = (-q1 - sq) / (2.0 * q0), k1 = (-q1 + sq) / (2.0 * q0);
      k.s0 = k1 < k0 ? k1 : k0;
      k.s1 = k1 < k0 ? k0 : k1;
      k.n = 2u;
    }
  }
#pragma unroll 1
  for (uint32_t stage = 0u; stage < 2u; ++stage) {
    const double b3 = 4.0 * a4, b2 = 3.0 * a3, b1 = 2.0 * a2, b0 = a1;
    auto P = [&](double x) { return (((a4 * x + a3) * x + a2) * x + a1) * x + a0; };
    auto D = [&](double x) { return ((b3 * x + b2) * x + b1) * x + b0; };
    TorusRoots out{0.0, 0.0, 0.0, 0.0, 0u};
    const uint32_t cap = 3u + stage;
    double a = lo, fa = P(lo);
#pragma unroll 1
    for (uint32_t i = 0u; i <= k.n; ++i) {
      const double b = i == k.n ? hi : (i == 0u ? k.s0 : (i == 1u ? k.s1 : (i == 2u ? k.s2 : k.s3)));
      if (i < k.n && !(b > a && b < hi)) continue;  // a critical point outside the interval, or not above the last one
      const double fb = P(b);
      if (fa == 0.0) {
        torus_push(out, cap, a);
      } else if ((fa < 0.0) != (fb < 0.0) && fb != 0.0) {
        // a sign change on a monotone piece: Newton, safeguarded by bisection, at most 80 steps
        double l = a, h = b;
        double x = 0.5 * (l + h);
#pragma unroll 1
        for (uint32_t it = 0u; it < 80u; ++it) {
          const double fx = P(x);
          if (fx == 0.0) break;
          if ((fx < 0.0) == (fa < 0.0)) l = x;
          else h = x;
          const double d = D(x);
          double xn = d != 0.0 ? x - fx / d : l;
          if (!(xn > l && xn < h)) xn = 0.5 * (l + h);
          const double mid = 0.5 * (l + h);
          const bool stop = xn == x || !(l < h) || mid == l || mid == h;
          x = xn;
          if (stop) break;
        }
        torus_push(out, cap, x);
      }
      a = b;
      fa = fb;
    }
    if (fa == 0.0) torus_push(out, cap, a);
    k = out;
    a4 = c4;
    a3 = c3;
    a2 = c2;
    a1 = c1;
    a0 = c0;
  }
  return k;
}
#endif  // RTC_TORUS_TU

// Emits the entries a leaf's localIntersect appends, in the reference's order, as f(t, u, v).
// `r` is the ray in the leaf's object space.
struct CylParams {
  double ymin, ymax;
  bool closed;
};

#ifdef RTC_TORUS_TU
// Torus.localIntersect, steps 1 to 5 of rtc.h: the roots as ray parameters t, ascending.  cy.ymin is the major radius R,
// cy.ymax the minor radius r (the cyl_* rows).
__device__ __forceinline__ TorusRoots torus_roots(const CylParams& cy, const Ray& r) {
  TorusRoots k{0.0, 0.0, 0.0, 0.0, 0u};
  const double R = cy.ymin, rm = cy.ymax;
  const double alpha = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;
  const double t0 = -((r.ox * r.dx + r.oy * r.dy) + r.oz * r.dz) / alpha;  // step 1: the point nearest the centre
  const double bxz = (R + rm) * (1.0 + 1e-9), by = rm * (1.0 + 1e-9);      // step 2: the padded object box
  double tmin, tmax;
  if (!slab(r, -bxz, -by, -bxz, bxz, by, bxz, tmin, tmax)) return k;
  const double px = r.ox + t0 * r.dx, py = r.oy + t0 * r.dy, pz = r.oz + t0 * r.dz;
  const double beta = 2.0 * ((px * r.dx + py * r.dy) + pz * r.dz);  // step 3
  const double gamma = (((px * px + py * py) + pz * pz) + R * R) - rm * rm;
  const double f = 4.0 * (R * R);
  const double c4 = alpha * alpha;
  const double c3 = (2.0 * alpha) * beta;
  const double c2 = (beta * beta + (2.0 * alpha) * gamma) - f * (r.dx * r.dx + r.dz * r.dz);
  const double c1 = (2.0 * beta) * gamma - (2.0 * f) * (px * r.dx + pz * r.dz);
  const double c0 = gamma * gamma - f * (px * px + pz * pz);
  k = torus_quartic(c4, c3, c2, c1, c0, tmin - t0, tmax - t0);  // step 4
  k.s0 = t0 + k.s0;                                            // step 5
  k.s1 = t0 + k.s1;
  k.s2 = t0 + k.s2;
  k.s3 = t0 + k.s3;
  return k;
}
template <class F>
__device__ __forceinline__ void torus_emit(const TorusRoots& k, F&& f) {
  if (k.n > 0u) f(k.s0, 0.0, 0.0);
  if (k.n > 1u) f(k.s1, 0.0, 0.0);
  if (k.n > 2u) f(k.s2, 0.0, 0.0);
  if (k.n > 3u) f(k.s3, 0.0, 0.0);
}
#define RTC_HAS_CYL_ROW(kind) ((kind) == 3u || (kind) == 6u || (kind) == 7u)
#else
#define RTC_HAS_CYL_ROW(kind) ((kind) == 3u || (kind) == 6u)
#endif

// SIMPLE: the world has only spheres, planes and cubes (the `simple` kernel variant); the other kinds are not compiled.
template <bool SIMPLE = false, class F>
__device__ __forceinline__ void leaf_entries(uint32_t kind, const CylParams& cy, const double* __restrict__ T,
                                             const Ray& r, F&& f) {
  if (SIMPLE && kind > 2u) return;
  switch (kind) {
    case 0: {  // sphere.zig:24-46
      const double a = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;
      const double b = 2.0 * ((r.ox * r.dx + r.oy * r.dy) + r.oz * r.dz);
      const double c = ((r.ox * r.ox + r.oy * r.oy) + r.oz * r.oz) - 1.0;
      const double discriminant = b * b - 4.0 * a * c;
      if (discriminant >= 0.0) {
        const double sq = __builtin_sqrt(discriminant);
        double t1 = (-b - sq) / (2.0 * a);
        double t2 = (-b + sq) / (2.0 * a);
        if (t2 < t1) {  // sortIntersections on two entries
          const double s = t1;
          t1 = t2;
          t2 = s;
        }
        f(t1, 0.0, 0.0);
        f(t2, 0.0, 0.0);
      }
      break;
    }
    case 1: {  // plane.zig:25-36
      if (__builtin_fabs(r.dy) > 1e-5) f(-r.oy / r.dy, 0.0, 0.0);
      break;
    }
    case 2: {  // cube.zig:49-79
      double tmin, tmax;
      if (cube_slab(r, tmin, tmax)) {
        f(tmin, 0.0, 0.0);
        f(tmax, 0.0, 0.0);
      }
      break;
    }
    case 3: {  // cylinder.zig:53-98
      if constexpr (SIMPLE) break;
      const double a = r.dx * r.dx + r.dz * r.dz;
      bool walls_done = false, caps = true;
      if (__builtin_fabs(a) < 1e-5) {
        walls_done = true;  // parallel to the axis: caps only
      }
      if (!walls_done) {
        const double b = 2.0 * r.ox * r.dx + 2.0 * r.oz * r.dz;
        const double c = (r.ox * r.ox + r.oz * r.oz) - 1.0;
        const double discriminant = b * b - 4.0 * a * c;
        if (discriminant < 0.0) {
          caps = false;  // early return before intersectCaps
        } else {
          const double sq = __builtin_sqrt(discriminant);
          double t0 = (-b - sq) / (2.0 * a);
          double t1 = (-b + sq) / (2.0 * a);
          if (t0 > t1) {
            const double s = t0;
            t0 = t1;
            t1 = s;
          }
          const double y0 = r.oy + t0 * r.dy;
          if (cy.ymin < y0 && y0 < cy.ymax) f(t0, 0.0, 0.0);
          const double y1 = r.oy + t1 * r.dy;
          if (cy.ymin < y1 && y1 < cy.ymax) f(t1, 0.0, 0.0);
        }
      }
      if (caps && cy.closed && !(__builtin_fabs(r.dy) < 1e-5)) {  // cylinder.zig:37-51
        double t = (cy.ymin - r.oy) / r.dy;
        double x = r.ox + t * r.dx, z = r.oz + t * r.dz;
        if (x * x + z * z <= 1.0) f(t, 0.0, 0.0);
        t = (cy.ymax - r.oy) / r.dy;
        x = r.ox + t * r.dx;
        z = r.oz + t * r.dz;
        if (x * x + z * z <= 1.0) f(t, 0.0, 0.0);
      }
      break;
    }
    case 6: {  // cone.zig:52-113
      const double tol = 1e-4;
      const double a = (r.dx * r.dx - r.dy * r.dy) + r.dz * r.dz;
      const double b = (2.0 * r.ox * r.dx - 2.0 * r.oy * r.dy) + 2.0 * r.oz * r.dz;
      bool caps = true;
      if (__builtin_fabs(a) < tol && __builtin_fabs(b) < tol) {
        // misses the surface; caps only
      } else {
        const double c = (r.ox * r.ox - r.oy * r.oy) + r.oz * r.oz;
        if (__builtin_fabs(a) < tol) {
          f(-c / (2.0 * b), 0.0, 0.0);
        } else {
          const double discriminant = b * b - 4.0 * a * c;
          if (discriminant < 0.0) {
            caps = false;
          } else {
            const double sq = __builtin_sqrt(discriminant);
            double t0 = (-b - sq) / (2.0 * a);
            double t1 = (-b + sq) / (2.0 * a);
            if (t0 > t1) {
              const double s = t0;
              t0 = t1;
              t1 = s;
            }
            const double y0 = r.oy + t0 * r.dy;
            if (cy.ymin < y0 && y0 < cy.ymax) f(t0, 0.0, 0.0);
            const double y1 = r.oy + t1 * r.dy;
            if (cy.ymin < y1 && y1 < cy.ymax) f(t1, 0.0, 0.0);
          }
        }
      }
      if (caps && cy.closed && !(__builtin_fabs(r.dy) < tol)) {  // cone.zig:36-50
        double t = (cy.ymin - r.oy) / r.dy;
        double x = r.ox + t * r.dx, z = r.oz + t * r.dz;
        if (x * x + z * z <= cy.ymin * cy.ymin) f(t, 0.0, 0.0);
        t = (cy.ymax - r.oy) / r.dy;
        x = r.ox + t * r.dx;
        z = r.oz + t * r.dz;
        if (x * x + z * z <= cy.ymax * cy.ymax) f(t, 0.0, 0.0);
      }
      break;
    }
#ifdef RTC_TORUS_TU
    case 7: {  // RTC_TORUS: up to four entries, ascending
      if constexpr (SIMPLE) break;
      torus_emit(torus_roots(cy, r), f);
      break;
    }
#endif
    default: {  // 4 triangle.zig:29-63, 5 triangle.zig:225-259 (Moller-Trumbore, left-handed cross)
      if constexpr (SIMPLE) break;
      if constexpr ((RTC_EXPERIMENT & 4) != 0) {  // (bound experiment: what an FP32 triangle test in place of the exact one would buy at most)
        const float p1x = static_cast<float>(T[0]), p1y = static_cast<float>(T[1]), p1z = static_cast<float>(T[2]);
        const float e1x = static_cast<float>(T[3]), e1y = static_cast<float>(T[4]), e1z = static_cast<float>(T[5]);
        const float e2x = static_cast<float>(T[6]), e2y = static_cast<float>(T[7]), e2z = static_cast<float>(T[8]);
        const float dx = static_cast<float>(r.dx), dy = static_cast<float>(r.dy), dz = static_cast<float>(r.dz);
        const float cx = dy * e2z - dz * e2y, cy_ = dz * e2x - dx * e2z, cz = dx * e2y - dy * e2x;
        const float det = (e1x * cx + e1y * cy_) + e1z * cz;
        if (__builtin_fabsf(det) < 1e-5f) break;
        const float ff = 1.0f / det;
        const float qx = static_cast<float>(r.ox) - p1x, qy = static_cast<float>(r.oy) - p1y, qz = static_cast<float>(r.oz) - p1z;
        const float u = ff * ((qx * cx + qy * cy_) + qz * cz);
        if (u < 0.0f || u > 1.0f) break;
        const float ox = qy * e1z - qz * e1y, oy = qz * e1x - qx * e1z, oz = qx * e1y - qy * e1x;
        const float v = ff * ((dx * ox + dy * oy) + dz * oz);
        if (v < 0.0f || (u + v) > 1.0f) break;
        f(static_cast<double>(ff * ((e2x * ox + e2y * oy) + e2z * oz)), static_cast<double>(u), static_cast<double>(v));
        break;
      }
      const double p1x = T[0], p1y = T[1], p1z = T[2];
      const double e1x = T[3], e1y = T[4], e1z = T[5];
      const double e2x = T[6], e2y = T[7], e2z = T[8];
      // dir_cross_e2 = direction.cross(e2)  (tuple.zig:128)
      const double cx = r.dy * e2z - r.dz * e2y;
      const double cy = r.dz * e2x - r.dx * e2z;
      const double cz = r.dx * e2y - r.dy * e2x;
      const double det = (e1x * cx + e1y * cy) + e1z * cz;
      if (__builtin_fabs(det) < 1e-5) break;
      const double ff = 1.0 / det;
      const double qx = r.ox - p1x, qy = r.oy - p1y, qz = r.oz - p1z;  // p1_to_origin
      const double u = ff * ((qx * cx + qy * cy) + qz * cz);
      if (u < 0.0 || u > 1.0) break;
      // p1_to_origin.cross(e1)
      const double ox = qy * e1z - qz * e1y;
      const double oy = qz * e1x - qx * e1z;
      const double oz = qx * e1y - qy * e1x;
      const double v = ff * ((r.dx * ox + r.dy * oy) + r.dz * oz);
      if (v < 0.0 || (u + v) > 1.0) break;
      const double t = ff * ((e2x * ox + e2y * oy) + e2z * oz);
      f(t, u, v);
      break;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Candidate enumeration: World.intersect (world.zig:71-83) + Group.localIntersect
// (group.zig:39-62) without materialising the list.  The visitor sees every entry the
// reference would have appended: vis.entry(leaf, meta, t, u, v); vis.cull(tmin, tmax) may
// skip a group whose box interval cannot contribute; vis.done() stops early.
// Box-interval culling is conservative by kBoxSlack: a box's [tmin,tmax] and a leaf's t are
// computed by different roundings, so "entirely behind / beyond" is only trusted with slack.
// ------------------------------------------------------------------------------------------

// The reference only records a leaf's entries if the ray's LINE passes the box of every Group above it
// (Group.localIntersect, group.zig:46-50).  The kernel finds candidates through its own BVH, so before a
// leaf may influence a visitor this chain of reference box tests is replayed, bottom-up, on the
// reference's boxes.  Shortcut: if the candidate point o + t*d lies inside a box by a margin far above
// rounding, the line passes through that box and every slab comparison of the reference test holds with
// room to spare - unless a direction component is below the reference's 1e-5 "parallel" threshold, where
// the reference test ignores the direction (bounding_box.zig:124-127); then the exact test is run.
__device__ __forceinline__ bool chain_ok(const DevScene& S, uint32_t first_parent, const Ray& ray, double t, bool degenerate) {
  const double px = ray.ox + ray.dx * t, py = ray.oy + ray.dy * t, pz = ray.oz + ray.dz * t;
  const double scale = zmax(zmax(__builtin_fabs(px), __builtin_fabs(py)), __builtin_fabs(pz)) +
                       zmax(zmax(__builtin_fabs(ray.ox), __builtin_fabs(ray.oy)), __builtin_fabs(ray.oz));
  const double m = 1e-9 * (1.0 + scale);
  uint32_t n = first_parent;  // leaf_parent[] of the leaf
  while (n != RTC_NO_LEAF) {
    const double* __restrict__ B = S.node_box + 6ull * n;
    const double b0 = B[0], b1 = B[1], b2 = B[2], b3 = B[3], b4 = B[4], b5 = B[5];
    const bool inside = !degenerate & (b0 + m <= px) & (px <= b3 - m) & (b1 + m <= py) & (py <= b4 - m) &
                        (b2 + m <= pz) & (pz <= b5 - m);
    if (!inside) {
      double tmin, tmax;
      if (!slab(ray, b0, b1, b2, b3, b4, b5, tmin, tmax)) return false;
    }
    // Nested boxes: every bound of an outer box is at least as wide, the reference's slab arithmetic is monotone in
    // the bounds (subtract the origin, divide by - or multiply infinity with - the same direction component), so
    // the outer tests pass as well.  (Ten levels of dependent fetches on dragons.json otherwise.)
    if (S.chain_nested) return true;
    n = S.node_parent[n];
  }
  return true;
}

// A leaf proposed by the BVH: run the exact reference test; if one of its entries could change the
// visitor's state, replay the reference box chain, then hand the entries over.
template <class V>
__device__ __forceinline__ void visit_leaf(const DevScene& S, const BvhLeafRec& Lm, const Ray& ray, bool degenerate,
                                           uint32_t& cur_xf, Ray& lr, V& vis) {
  // The whole 104-byte record in one go - header AND triangle -, so that the walk waits for memory once per leaf: read
  // field by field the triangle's loads were issued behind the wait for the header (the kind decides whether it is
  // needed), a second round trip per leaf.
  // (dragons 4K 2.30 -> 2.25 ms, nefertiti 0.565 -> 0.550; groups.json, whose leaves are cones and cylinders, pays 5 % for
  // triangle words it does not use)
  const BvhLeafRec L = Lm;
  // isShadowed (world.zig:136-147) counts an entry only if its shape casts a shadow: a leaf that does not - a glass display
  // case around a mesh - has nothing a shadow trace could use, whatever its test would say.
  if (V::kShadowOnly && ((L.kind_flags >> 8) & 1u) == 0u) return;
  const uint32_t leaf = L.leaf;
  const uint4 meta{L.kind_flags, L.xform, L.material, L.geom};
  if (meta.y != cur_xf) {  // Shape.intersect: ray.transform(_inverse_transform), shape.zig:314-318
    lr = xform_ray(S.xf + 12ull * meta.y, ray);
    cur_xf = meta.y;
  }
  const uint32_t kind = meta.x & 0xFFu;
  CylParams cy{0.0, 0.0, false};
  if (RTC_HAS_CYL_ROW(kind)) {
    const DevCyl c = S.cyl[meta.w];
    cy = {c.ymin, c.ymax, c.closed != 0u};
  }
  const uint32_t shadow = (meta.x >> 8) & 1u;
  if (kind == 4u || kind == 5u) {  // a triangle has at most one entry: evaluate it once
    bool hit = false;
    double ht = 0.0, hu = 0.0, hv = 0.0;
    leaf_entries(kind, cy, L.tri, lr, [&](double t, double u, double v) {
      hit = true;
      ht = t;
      hu = u;
      hv = v;
    });
    if (!hit || !vis.relevant(leaf, shadow, ht)) return;
    if (!chain_ok(S, L.parent, ray, ht, degenerate)) return;
    vis.entry(leaf, shadow, meta.z, ht, hu, hv);
    return;
  }
#ifdef RTC_TORUS_TU
  if (kind == 7u) {  // a torus: the quartic is solved once, for the relevance pass and for the entries
    const TorusRoots k = torus_roots(cy, lr);
    bool rel = false;
    double t_first = 0.0;
    torus_emit(k, [&](double t, double, double) {
      if (!rel && vis.relevant(leaf, shadow, t)) {
        rel = true;
        t_first = t;
      }
    });
    if (!rel) return;
    if (!chain_ok(S, L.parent, ray, t_first, degenerate)) return;
    torus_emit(k, [&](double t, double u, double v) { vis.entry(leaf, shadow, meta.z, t, u, v); });
    return;
  }
#endif
  bool relevant = false;
  double t_rel = 0.0;
  leaf_entries(kind, cy, L.tri, lr, [&](double t, double, double) {
    if (!relevant && vis.relevant(leaf, shadow, t)) {
      relevant = true;
      t_rel = t;
    }
  });
  if (!relevant) return;
  if (!chain_ok(S, L.parent, ray, t_rel, degenerate)) return;
  leaf_entries(kind, cy, L.tri, lr,
               [&](double t, double u, double v) { vis.entry(leaf, shadow, meta.z, t, u, v); });
}

// ------------------------------------------------------------------------------------------
// CSG (shapes/csg.zig).  A csg UNIT (a csg node whose parent is not a csg) is evaluated as a whole:
//   1. every leaf below it appends its entries - if the ray's line passes the box of every Group and Csg
//      above the leaf (csg.zig:79-83 tests the csg's own, never re-boxed, _bbox like a group does);
//   2. the list is sorted by t, stably: ties keep depth-first leaf order, which is what the reference's
//      nested (left ++ right, stable sort) produces at every level (csg.zig:85-93, group.zig:52-60);
//   3. one pass in that order applies filterIntersections (csg.zig:51-72) of EVERY csg node of the unit at
//      once: an entry climbs from its leaf towards the unit; at each csg node it is tested against that
//      node's (inl, inr), toggles one of them, and stops climbing where it is filtered out - exactly the
//      entries the inner csg would have passed up are the ones that reach (and toggle) the outer one.
// The survivors are what Csg.localIntersect returns; the caller hands them to its visitor.
// Not inlined: scenes without csg never run it and its registers stay out of the main loop's budget.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool csg_rule(uint32_t op, bool lhit, bool inl, bool inr) {  // csg.zig:112-118
  if (op == 1u) return (lhit && !inr) || !(lhit || inl);
  if (op == 2u) return (lhit && inr) || (!lhit && inl);
  return (lhit && !inr) || (!lhit && inl);
}

__device__ __noinline__ uint32_t csg_collect(const DevScene& S, uint32_t unit, const Ray& ray, unsigned& overflow) {
  CsgRec* const buf = S.csg_buf + (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) * S.csg_entries * 64u +
                      (threadIdx.x & 63u);
  const bool degenerate = (__builtin_fabs(ray.dx) < 1e-5) | (__builtin_fabs(ray.dy) < 1e-5) | (__builtin_fabs(ray.dz) < 1e-5);
  const uint2 range = S.node_range[unit];
  uint32_t n = 0, dropped = 0;
  uint32_t cur_xf = 0xFFFFFFFFu;
  Ray lr = ray;
  for (uint32_t leaf = range.x; leaf < range.x + range.y; ++leaf) {
    const uint4 meta = S.leaf_meta[leaf];
    if (meta.y != cur_xf) {
      lr = xform_ray(S.xf + 12ull * meta.y, ray);
      cur_xf = meta.y;
    }
    const uint32_t kind = meta.x & 0xFFu;
    CylParams cy{0.0, 0.0, false};
    if (RTC_HAS_CYL_ROW(kind)) {
      const DevCyl c = S.cyl[meta.w];
      cy = {c.ymin, c.ymax, c.closed != 0u};
    }
    bool any = false, boxes = false;
    leaf_entries(kind, cy, S.tri + 9ull * meta.w, lr, [&](double t, double u, double v) {
      if (!any) {
        any = true;
        boxes = chain_ok(S, S.leaf_parent[leaf], ray, t, degenerate);
      }
      if (!boxes) return;
      if (n >= S.csg_entries) {  // the list is full: keep counting what it would have needed (the host sizes it by that)
        ++dropped;
        return;
      }
      // insertion sort by t, stable (equal t: the later entry stays behind)
      uint32_t i = n;
      while (i > 0u && buf[static_cast<size_t>(i - 1u) * 64u].t > t) {
        buf[static_cast<size_t>(i) * 64u] = buf[static_cast<size_t>(i - 1u) * 64u];
        --i;
      }
      CsgRec rec;
      rec.t = t;
      rec.u = u;
      rec.v = v;
      rec.leaf = leaf;
      rec.flags = 0u;
      buf[static_cast<size_t>(i) * 64u] = rec;
      ++n;
    });
  }
  // (the lane's overflow word: bit 0 = a per-lane stack ran out; bits 8 and up = entries a csg list needed, OR-ed over the
  // lists that ran out: an upper bound of the longest, within a factor of two)
  if (dropped != 0u) overflow |= (n + dropped) << 8;
  unsigned long long inl = 0ull, inr = 0ull;  // one bit per csg node of the unit (node_info slot, < 64)
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t leaf = buf[static_cast<size_t>(i) * 64u].leaf;
    uint32_t side = (S.leaf_meta[leaf].x >> 10) & 1u;
    uint32_t cur = S.leaf_parent[leaf];
    bool survives = true;
    for (int guard = 0; guard < 4096; ++guard) {
      const uint32_t info = S.node_info[cur];
      const uint32_t op = info & 3u;
      if (op != 0u) {
        const unsigned long long bit = 1ull << ((info >> 8) & 63u);
        const bool lhit = side == 0u;
        const bool allowed = csg_rule(op, lhit, (inl & bit) != 0u, (inr & bit) != 0u);
        if (lhit) {
          inl ^= bit;
        } else {
          inr ^= bit;
        }
        if (!allowed) {
          survives = false;
          break;
        }
      }
      if (cur == unit) break;
      side = (info >> 16) & 1u;
      cur = S.node_parent[cur];
    }
    buf[static_cast<size_t>(i) * 64u].flags = survives ? 1u : 0u;
  }
  return n;
}

// Hands the surviving entries of a csg unit to a visitor.  The closest-hit and shadow reductions take
// them in list order; the containers walk (BehindVisitor) needs the entries of one leaf together.
template <class V>
__device__ __forceinline__ void visit_csg(const DevScene& S, uint32_t unit, const Ray& ray, V& vis, unsigned& overflow) {
  const uint32_t n = csg_collect(S, unit, ray, overflow);
  CsgRec* const buf = S.csg_buf + (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) * S.csg_entries * 64u +
                      (threadIdx.x & 63u);
  for (uint32_t i = 0; i < n; ++i) {
    const CsgRec a = buf[static_cast<size_t>(i) * 64u];
    if (a.flags != 1u) continue;
    const uint4 meta = S.leaf_meta[a.leaf];
    vis.entry(a.leaf, (meta.x >> 8) & 1u, meta.z, a.t, a.u, a.v);
    if (V::kBehindOnly) {  // the leaf's remaining survivors right away
      for (uint32_t j = i + 1u; j < n; ++j) {
        const CsgRec b = buf[static_cast<size_t>(j) * 64u];
        if (b.flags == 1u && b.leaf == a.leaf) {
          vis.entry(b.leaf, (meta.x >> 8) & 1u, meta.z, b.t, b.u, b.v);
          buf[static_cast<size_t>(j) * 64u].flags = 3u;
        }
      }
    }
  }
}

// Walks the candidate BVH of one group (BvhNode, rtc_device.h) with an FP32 copy of the ray.  The boxes
// were rounded outward at upload; `delta` adds what the FP32 ray and slab arithmetic can be off by
// (5e-7 * (|o| + largest box coordinate)), so a leaf whose exact test would produce an entry is never
// skipped; visitors prune by t-interval with their own slack.
template <bool CSG, class V>
__device__ __forceinline__ void traverse_bvh(const DevScene& S, uint32_t root, const Ray& ray, V& vis,
                                             unsigned& overflow, uint32_t* lds_stack) {
  const float ox = static_cast<float>(ray.ox), oy = static_cast<float>(ray.oy), oz = static_cast<float>(ray.oz);
  const float dx = static_cast<float>(ray.dx), dy = static_cast<float>(ray.dy), dz = static_cast<float>(ray.dz);
  const float delta = 5e-7f * (fmaxf(fmaxf(__builtin_fabsf(ox), __builtin_fabsf(oy)), __builtin_fabsf(oz)) + S.bvh_mag);
  const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
  const bool px = dx >= 0.0f, py = dy >= 0.0f, pz = dz >= 0.0f;
  // Which of a node's two planes per axis the ray meets first is the ray's business, not the node's: the lane fetches
  // "near x" and "far x" ... from the byte offsets its direction signs pick (lo[axis] at 16 * axis, hi[axis] at 48 + 16 *
  // axis) - six 32-bit adds per node instead of twenty-four selects on the fetched boxes.
  const uint32_t off_nx = px ? 0u : 48u, off_fx = px ? 48u : 0u;
  const uint32_t off_ny = py ? 16u : 64u, off_fy = py ? 64u : 16u;
  const uint32_t off_nz = pz ? 32u : 80u, off_fz = pz ? 80u : 32u;
  // origin shifted against / along the direction: (near - on) and (far - of) grow the box by delta
  const float onx = px ? ox + delta : ox - delta, ofx = px ? ox - delta : ox + delta;
  const float ony = py ? oy + delta : oy - delta, ofy = py ? oy - delta : oy + delta;
  const float onz = pz ? oz + delta : oz - delta, ofz = pz ? oz - delta : oz + delta;
  const bool degenerate = (__builtin_fabs(ray.dx) < 1e-5) | (__builtin_fabs(ray.dy) < 1e-5) | (__builtin_fabs(ray.dz) < 1e-5);
  uint32_t cur_xf = 0xFFFFFFFFu;
  Ray lr = ray;
  // "while-while" traversal: every lane first walks inner nodes until it holds a leaf (cheap FP32 box tests, one
  // 64-byte fetch per step), then all lanes that hold one run the expensive exact FP64 leaf test TOGETHER.  With
  // one loop that does either per iteration, lanes at leaves and lanes at nodes take turns (33 % of lanes active
  // on dragons.json).
  // The first RTC_LDS_TRAV entries of the stack live in LDS ([entry][lane]: conflict-free), the rest in scratch: a pop
  // sits between two dependent fetches, and LDS answers sooner than the vector memory path.
  // (The LDS part goes through an LDS-typed pointer: with two generic pointers the compiler merged a pop's two loads
  // into one FLAT load from a selected address, which waits for both the LDS and the vector-memory counters.)
  typedef __attribute__((address_space(3))) uint32_t LdsWord;
  LdsWord* const lds_top = (LdsWord*)lds_stack;
  uint32_t stack[RTC_TRAV_STACK - RTC_LDS_TRAV];
  int sp = 0;
  auto push = [&](uint32_t v) {
    if (sp < RTC_LDS_TRAV) {
      lds_top[sp * 64] = v;
    } else {
      stack[sp - RTC_LDS_TRAV] = v;
    }
    ++sp;
  };
  auto pop = [&]() {
    --sp;
    uint32_t v;
    if (sp < RTC_LDS_TRAV) {
      v = lds_top[sp * 64];
    } else {
      v = stack[sp - RTC_LDS_TRAV];
    }
    return v;
  };
  uint32_t next = root;  // the node to visit next stays in a register: the stack (scratch memory) is one more dependent fetch
#ifdef RTC_PROFILE
  unsigned long long pw_nodes = 0, pw_leaves = 0, pw_node_lanes = 0, pw_leaf_lanes = 0;
  const unsigned long long pw_lanes = __builtin_popcountll(__ballot(true));
#endif
  for (;;) {
    uint32_t leaf_ref = RTC_NO_LEAF;
    while ((next != RTC_NO_LEAF || sp > 0) && !vis.done()) {
#ifdef RTC_PROFILE
      pw_nodes += 1ull;
      pw_node_lanes += __builtin_popcountll(__ballot(true));
#endif
      uint32_t ref = next;
      next = RTC_NO_LEAF;
      if (ref == RTC_NO_LEAF) ref = pop();
      if (ref & RTC_NODE_BIT) {  // a range of 1..8 leaves
        leaf_ref = ref;
        break;
      }
      // One 128-byte node: four child boxes, component by component.
      typedef float Float4 __attribute__((ext_vector_type(4)));
      const char* const table = reinterpret_cast<const char*>(S.bvh);  // (wave-uniform base + a 32-bit offset per lane)
      const uint32_t at = ref * static_cast<uint32_t>(sizeof(Bvh4Node));
      auto plane = [&](uint32_t off) { return *reinterpret_cast<const Float4*>(table + (at + off)); };
      const Float4 nearx = plane(off_nx), neary = plane(off_ny), nearz = plane(off_nz);
      const Float4 farx = plane(off_fx), fary = plane(off_fy), farz = plane(off_fz);
      const uint4 kids = *reinterpret_cast<const uint4*>(table + (at + 96u));
      const Float4 tnx = (nearx - onx) * ix, tfx = (farx - ofx) * ix;
      const Float4 tny = (neary - ony) * iy, tfy = (fary - ofy) * iy;
      const Float4 tnz = (nearz - onz) * iz, tfz = (farz - ofz) * iz;
      // max / min drop the NaN of 0 * inf (ray inside a slab, parallel to it)
      const Float4 tn = __builtin_elementwise_max(__builtin_elementwise_max(tnx, tny), tnz);
      const Float4 tf = __builtin_elementwise_min(__builtin_elementwise_min(tfx, tfy), tfz);
      const uint32_t c4[4] = {kids.x, kids.y, kids.z, kids.w};
      float key[4];
      uint32_t refs[4];
      int entered = 0;
      const float far_limit = vis.far_limit();  // (once per node, not per child)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool h = (c4[k] != RTC_NO_LEAF) & (tn[k] <= tf[k]) & (tn[k] < __builtin_inff()) & !vis.cull_limits(tn[k], tf[k], far_limit);
        key[k] = h ? tn[k] : __builtin_inff();
        refs[k] = c4[k];
        entered += h ? 1 : 0;
      }
      if (entered == 0) continue;
      if (sp + entered > RTC_TRAV_STACK) {
        overflow |= 1u;
        continue;
      }
      // farthest first, so that the nearest child is popped first (children not entered carry +inf and sort to the front)
      auto order = [&](int a, int b) {
        const bool swap = key[a] < key[b];
        const float ka = swap ? key[b] : key[a], kb = swap ? key[a] : key[b];
        const uint32_t ra = swap ? refs[b] : refs[a], rb = swap ? refs[a] : refs[b];
        key[a] = ka;
        key[b] = kb;
        refs[a] = ra;
        refs[b] = rb;
      };
      // (a shadow ray stops at any entry that counts: sorting its children - fully, or only the nearest to the top -
      // cost more than it saved: dragons 4K 4.43 -> 4.25 ms, nefertiti 0.88 -> 0.85 ms, teapot 0.382 -> 0.384 ms without)
      if constexpr (!V::kAnyHit) {
        order(0, 1);
        order(2, 3);
        order(0, 2);
        order(1, 3);
        order(1, 2);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (key[k] < __builtin_inff()) {
          if (next != RTC_NO_LEAF) push(next);  // the last child entered (the nearest, where they are sorted) is not pushed
          next = refs[k];
        }
      }
    }
    if (leaf_ref == RTC_NO_LEAF) break;  // nothing left (or the visitor is done)
    const uint32_t first = (leaf_ref & ~RTC_NODE_BIT) >> 3, count = (leaf_ref & 7u) + 1u;
    for (uint32_t i = 0; i < count; ++i) {
#ifdef RTC_PROFILE
      pw_leaves += 1ull;
      pw_leaf_lanes += __builtin_popcountll(__ballot(true));
#endif
      const BvhLeafRec& L = S.bvh_leaf[first + i];
      if (CSG && (L.leaf & RTC_NODE_BIT)) {  // a csg unit inside the group (only the *_ext kernels have this path)
        if constexpr (CSG) visit_csg(S, L.leaf & ~RTC_NODE_BIT, ray, vis, overflow);
      } else {
        visit_leaf(S, L, ray, degenerate, cur_xf, lr, vis);
      }
    }
  }
#ifdef RTC_PROFILE  // walks of the wave, their lanes, wave steps at nodes / at leaves, lanes at nodes / at leaves (summed over the steps)
  RTC_WALK_ADD(0, 1);
  RTC_WALK_ADD(1, pw_lanes);
  RTC_WALK_ADD(2, pw_nodes);
  RTC_WALK_ADD(3, pw_leaves);
  RTC_WALK_ADD(4, pw_node_lanes);
  RTC_WALK_ADD(5, pw_leaf_lanes);
  if (pw_leaves == 0ull) RTC_WALK_ADD(6, 1);         // walks that reach no leaf at all ...
  if (pw_leaves == 0ull) RTC_WALK_ADD(7, pw_nodes);  // ... and the node steps they took
#endif
}

#if RTC_BVH8
// Walks the EIGHT-wide compressed candidate BVH of one group (Bvh8Node, rtc_device.h) with an FP32 copy of the ray.
// Per node: five 16-byte fetches bring eight child boxes; a child plane is origin + q * step, so its ray parameter is
// q * (step / d) + (origin - o) / d - one conversion and one FMA per plane, the per-node part computed once; the ray's
// direction signs pick which of a child's two planes per axis is the near one; `margin` (see traverse_bvh's delta; the
// FMA form rounds differently from (plane - o) / d, within a few ulps of the same magnitudes, so the margin is doubled)
// widens every interval.  The pending children of a node are ONE stack entry - the first inner child's index, the hit
// mask in front-to-back order (slot XOR direction signs) and the node's inner-child mask - so a node costs at most one
// push, and the stack is as deep as the tree (a handful of entries, all in LDS).  While-while as before: lanes descend
// until they hold leaf ranges, then all lanes that hold some run their exact FP64 leaf tests together.  A visitor for
// which the first entry that counts ends the trace (kAnyHit) takes the children in slot order.
// Leaves no box bounds (planes, cones: RootRec::always_*) are visited first, unconditionally.
__device__ __forceinline__ uint32_t permute_by_octant(uint32_t x, uint32_t oct) {  // bit p of the result = bit (p ^ oct) of x (8 bits)
  const uint32_t s1 = ((x & 0x55u) << 1) | ((x >> 1) & 0x55u);
  x = (oct & 1u) ? s1 : x;
  const uint32_t s2 = ((x & 0x33u) << 2) | ((x >> 2) & 0x33u);
  x = (oct & 2u) ? s2 : x;
  const uint32_t s4 = ((x & 0x0Fu) << 4) | ((x >> 4) & 0x0Fu);
  return (oct & 4u) ? s4 : x;
}

template <bool CSG, class V, int LDS_ENTRIES = RTC_LDS_TRAV>
__device__ __forceinline__ void traverse_bvh8(const DevScene& S, const uint32_t root, const uint32_t always_first,
                                              const uint32_t always_count, const Ray& ray, V& vis, unsigned& overflow,
                                              uint2* lds_stack, const uint4* __restrict__ root_node) {
  const float ox = static_cast<float>(ray.ox), oy = static_cast<float>(ray.oy), oz = static_cast<float>(ray.oz);
  float dx = static_cast<float>(ray.dx), dy = static_cast<float>(ray.dy), dz = static_cast<float>(ray.dz);
  // a direction component of (nearly) zero: 1e-30 instead - every product below stays finite, and over any parameter
  // range that matters the ray does not move by a rounding error's worth along that axis
  dx = __builtin_copysignf(fmaxf(__builtin_fabsf(dx), 1e-30f), dx);
  dy = __builtin_copysignf(fmaxf(__builtin_fabsf(dy), 1e-30f), dy);
  dz = __builtin_copysignf(fmaxf(__builtin_fabsf(dz), 1e-30f), dz);
  // (v_rcp_f32, one ulp: a relative 1.2e-7 on every parameter computed with it, an eighth of the margin below - and one
  // instruction where the IEEE quotient takes ten, three times per walk)
  const float ix = __builtin_amdgcn_rcpf(dx), iy = __builtin_amdgcn_rcpf(dy), iz = __builtin_amdgcn_rcpf(dz);
  const float delta = 1e-6f * (fmaxf(fmaxf(__builtin_fabsf(ox), __builtin_fabsf(oy)), __builtin_fabsf(oz)) + S.bvh_mag);
  const float mx = delta * __builtin_fabsf(ix), my = delta * __builtin_fabsf(iy), mz = delta * __builtin_fabsf(iz);
  const bool negx = dx < 0.0f, negy = dy < 0.0f, negz = dz < 0.0f;
  const uint32_t oct = V::kAnyHit ? 0u : ((negx ? 1u : 0u) | (negy ? 2u : 0u) | (negz ? 4u : 0u));
  const bool degenerate = (__builtin_fabs(ray.dx) < 1e-5) | (__builtin_fabs(ray.dy) < 1e-5) | (__builtin_fabs(ray.dz) < 1e-5);
  uint32_t cur_xf = 0xFFFFFFFFu;
  Ray lr = ray;
  auto visit = [&](uint32_t rec) {
    if ((RTC_EXPERIMENT & 2) && V::kAnyHit) return;
#ifdef RTC_PROFILE  // (diagnostic builds check every reference before it is followed: a wild one is counted and skipped)
    if (rec >= S.n_bvh_leaves) {
      RTC_WALK_ADD(7, 1);
      return;
    }
#endif
    const BvhLeafRec& L = S.bvh_leaf[rec];
    if (CSG && (L.leaf & RTC_NODE_BIT)) {  // a csg unit inside the group (only the *_ext kernels have this path)
      if constexpr (CSG) visit_csg(S, L.leaf & ~RTC_NODE_BIT, ray, vis, overflow);
    } else {
      visit_leaf(S, L, ray, degenerate, cur_xf, lr, vis);
    }
  };
  for (uint32_t i = 0; i < always_count; ++i) visit(always_first + i);
  // the stack: [entry][lane] in LDS (8 bytes per entry), the rest in scratch memory
  typedef uint32_t Pair __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) Pair LdsPair;
  LdsPair* const lds_top = (LdsPair*)lds_stack;
  Pair stack[RTC_TRAV_STACK - LDS_ENTRIES];
  int sp = 0;
  // the group in hand: the root is inner child 0 of a node that is not there
  // bits 0..7: children still to visit, front to back (bit p: slot p ^ oct); bits 8..15: the node's imask (by slot)
  uint32_t g_base = root, g_bits = (1u << oct) | 0x0100u;  // (slot 0 of the node that is not there)
  // Every walk's FIRST node - the group's root - is read from the group's World.objects record (RootRec::inv holds a copy
  // of it: in LDS for every world whose tables fit) instead of from the node table in memory: a walk takes 3.3 node steps
  // on dragons.json, each a gather of five 16-byte loads per lane through the CU's one vector-memory pipe (its data
  // return path is busy in three cycles of four, profiles/r03/pmc_mem_dragons.txt) - the root's no longer is.
  bool at_root = root_node != nullptr;
  uint32_t l_base = 0u, l_hits = 0u, meta_lo = 0u, meta_hi = 0u;
#ifdef RTC_PROFILE
  unsigned long long pw_nodes = 0, pw_leaves = 0, pw_node_lanes = 0, pw_leaf_lanes = 0;
  const unsigned long long pw_lanes = __builtin_popcountll(__ballot(true));
  unsigned long long pw_t = __builtin_amdgcn_s_memtime(), pw_t_nodes = 0, pw_t_leaves = 0;  // wave cycles in the two phases
#endif
  for (;;) {
    RTC_PRIO_PHASE(RTC_PRIO_NODE);
    while (l_hits == 0u && !vis.done()) {
      if ((g_bits & 0xFFu) == 0u) {
        if (sp == 0) break;
        --sp;
        Pair e;
        if (sp < LDS_ENTRIES) {
          e = lds_top[sp * 64];
        } else {
          e = stack[sp - LDS_ENTRIES];
        }
        g_base = e.x;
        g_bits = e.y;
      }
#ifdef RTC_PROFILE
      pw_nodes += 1ull;
      pw_node_lanes += __builtin_popcountll(__ballot(true));
#endif
      const uint32_t p = static_cast<uint32_t>(__builtin_ctz(g_bits));  // (the low byte is not empty)
      g_bits &= g_bits - 1u;
      const uint32_t slot = p ^ oct;
      const uint32_t node = g_base + static_cast<uint32_t>(__builtin_popcount((g_bits >> 8) & ((1u << slot) - 1u)));
      if ((g_bits & 0xFFu) != 0u) {  // its siblings wait
        if (sp < RTC_TRAV_STACK) {
          if (sp < LDS_ENTRIES) {
            lds_top[sp * 64] = Pair{g_base, g_bits};
          } else {
            stack[sp - LDS_ENTRIES] = Pair{g_base, g_bits};
          }
          ++sp;
        } else {
          overflow |= 1u;
        }
      }
#ifdef RTC_PROFILE
      if (node >= S.n_bvh_nodes) {
        RTC_WALK_ADD(7, 1);
        g_bits = 0u;
        continue;
      }
#endif
      uint4 h0, h1, qa, qb, qc;
      if (at_root) {
        at_root = false;
        h0 = root_node[0];
        h1 = root_node[1];
        qa = root_node[2];
        qb = root_node[3];
        qc = root_node[4];
      } else {
        const char* const at = reinterpret_cast<const char*>(S.bvh8) + node * static_cast<uint32_t>(sizeof(Bvh8Node));
        h0 = *reinterpret_cast<const uint4*>(at);
        h1 = *reinterpret_cast<const uint4*>(at + 16);
        qa = *reinterpret_cast<const uint4*>(at + 32);
        qb = *reinterpret_cast<const uint4*>(at + 48);
        qc = *reinterpret_cast<const uint4*>(at + 64);
      }
      // per node: step / d and (origin - o) / d, widened by the margin
      const float sx = __builtin_bit_cast(float, (h0.w & 0xFFu) << 23) * ix;
      const float sy = __builtin_bit_cast(float, ((h0.w >> 8) & 0xFFu) << 23) * iy;
      const float sz = __builtin_bit_cast(float, ((h0.w >> 16) & 0xFFu) << 23) * iz;
      const float bx = (__builtin_bit_cast(float, h0.x) - ox) * ix;
      const float by = (__builtin_bit_cast(float, h0.y) - oy) * iy;
      const float bz = (__builtin_bit_cast(float, h0.z) - oz) * iz;
      const float bnx = bx - mx, bfx = bx + mx, bny = by - my, bfy = by + my, bnz = bz - mz, bfz = bz + mz;
      // q = lo_x lo_y | lo_z hi_x | hi_y hi_z, eight bytes each: the near plane of an axis is the lower one for a ray that
      // travels up that axis
      const uint32_t nx0 = negx ? qb.z : qa.x, nx1 = negx ? qb.w : qa.y, fx0 = negx ? qa.x : qb.z, fx1 = negx ? qa.y : qb.w;
      const uint32_t ny0 = negy ? qc.x : qa.z, ny1 = negy ? qc.y : qa.w, fy0 = negy ? qa.z : qc.x, fy1 = negy ? qa.w : qc.y;
      const uint32_t nz0 = negz ? qc.z : qb.x, nz1 = negz ? qc.w : qb.y, fz0 = negz ? qb.x : qc.z, fz1 = negz ? qb.y : qc.w;
      float lo_c, hi_c;
      vis.box_limits(lo_c, hi_c);  // (once per node, not per child)
      uint32_t hits = 0u;
      // children k and k + 4 are the two halves of packed FP32 FMAs (v_pk_fma_f32: 24 instructions instead of 48)
      typedef float F2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sh = 8 * k;
        auto q2 = [&](uint32_t w0, uint32_t w1) { return F2{static_cast<float>((w0 >> sh) & 0xFFu), static_cast<float>((w1 >> sh) & 0xFFu)}; };
        const F2 tnx = __builtin_elementwise_fma(q2(nx0, nx1), F2(sx), F2(bnx)), tfx = __builtin_elementwise_fma(q2(fx0, fx1), F2(sx), F2(bfx));
        const F2 tny = __builtin_elementwise_fma(q2(ny0, ny1), F2(sy), F2(bny)), tfy = __builtin_elementwise_fma(q2(fy0, fy1), F2(sy), F2(bfy));
        const F2 tnz = __builtin_elementwise_fma(q2(nz0, nz1), F2(sz), F2(bnz)), tfz = __builtin_elementwise_fma(q2(fz0, fz1), F2(sz), F2(bfz));
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float tn = fmaxf(fmaxf(tnx[e], tny[e]), fmaxf(tnz[e], lo_c));
          const float tf = fminf(fminf(tfx[e], tfy[e]), fminf(tfz[e], hi_c));
          hits |= (tn <= tf) ? (1u << (k + 4 * e)) : 0u;
        }
      }
      const uint32_t imask = h0.w >> 24;
      const uint32_t inner = hits & imask;
      g_base = h1.x;
      g_bits = (V::kAnyHit ? inner : permute_by_octant(inner, oct)) | (imask << 8);
      l_hits = hits & (h1.y >> 24);
      if constexpr (V::kShadowOnly) {
        // (a shadow trace does not even fetch the records of a leaf range none of whose shapes casts a shadow: bit 7 of
        // the range's meta byte, set at build time - in dragons.json the display case around every dragon is such a leaf
        // and a child of its group's root node: every shadow walk through a group used to fetch and test it)
        const uint32_t dark_lo = ((((h1.z >> 7) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu;
        const uint32_t dark_hi = ((((h1.w >> 7) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu;
        l_hits &= ~(dark_lo | (dark_hi << 4));
      }
      l_base = h1.y & 0xFFFFFFu;
      meta_lo = h1.z;
      meta_hi = h1.w;
    }
#ifdef RTC_PROFILE
    {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      pw_t_nodes += now - pw_t;
      pw_t = now;
    }
#endif
    if (l_hits == 0u) break;  // nothing left (or the visitor is done)
    RTC_PRIO_PHASE(RTC_PRIO_WORK);
    while (l_hits != 0u) {
      const uint32_t k = static_cast<uint32_t>(__builtin_ctz(l_hits));
      l_hits &= l_hits - 1u;
      const uint32_t m = ((k < 4u ? meta_lo : meta_hi) >> (8u * (k & 3u))) & 0xFFu;
      const uint32_t first = l_base + ((m >> 2) & 31u), count = (m & 3u) + 1u;  // (bit 7: the range casts no shadow)
      for (uint32_t i = 0; i < count; ++i) {
#ifdef RTC_PROFILE
        pw_leaves += 1ull;
        pw_leaf_lanes += __builtin_popcountll(__ballot(true));
#endif
        visit(first + i);
      }
    }
#ifdef RTC_PROFILE
    {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      pw_t_leaves += now - pw_t;
      pw_t = now;
    }
#endif
  }
  RTC_PRIO_PHASE(RTC_PRIO_WORK);  // (a walk ends in its node phase)
#ifdef RTC_PROFILE  // walks of the wave, their lanes, wave steps at nodes / at leaves, lanes at nodes / at leaves (summed over the steps)
  RTC_AUX_ADD(5, pw_t_nodes);
  RTC_AUX_ADD(6, pw_t_leaves);
  {  // the same by kind of trace: closest hit, shadow, containers
    constexpr int K = 8 * (V::kAnyHit ? 1 : (V::kBehindOnly ? 2 : 0));
    RTC_KIND_ADD(K + 0, 1);
    RTC_KIND_ADD(K + 1, pw_lanes);
    RTC_KIND_ADD(K + 2, pw_nodes);
    RTC_KIND_ADD(K + 3, pw_leaves);
    RTC_KIND_ADD(K + 4, pw_node_lanes);
    RTC_KIND_ADD(K + 5, pw_leaf_lanes);
    RTC_KIND_ADD(K + 6, pw_t_nodes);
    RTC_KIND_ADD(K + 7, pw_t_leaves);
  }
  RTC_WALK_ADD(0, 1);
  RTC_WALK_ADD(1, pw_lanes);
  RTC_WALK_ADD(2, pw_nodes);
  RTC_WALK_ADD(3, pw_leaves);
  RTC_WALK_ADD(4, pw_node_lanes);
  RTC_WALK_ADD(5, pw_leaf_lanes);
  if (pw_leaves == 0ull) RTC_WALK_ADD(6, 1);  // walks that reach no leaf at all
#endif
}
#endif  // RTC_BVH8

// Conservative bounding-sphere rejection for one World.objects entry, in FP32.
// Everything under the root lies inside the sphere (radius inflated and rounded up at upload), so if the
// LINE misses the sphere the root contributes no entry at all; the visitor may additionally discard
// roots entirely behind the origin (closest hit, shadows) or entirely in front of it (containers pass).
// FP32 is safe here because the test only ever REMOVES work and every comparison carries a margin T that
// dominates the rounding of its operands: with S = |o| + max|c| the coordinates entering oc = c - o are
// off by <= 1.2e-7 * S each, which perturbs b^2 - a*c and a*(oc^2 - r^2) by less than
// 8e-6 * a * (oc^2 + S^2) = T  (>= 4e-6 * a * (|oc| + S)^2).  Far from the origin T grows and the test
// merely rejects less.  Branch-free on purpose: phase 1 is a straight-line stream of LDS reads and
// FP32 math (half the issue cost of FP64).  r2 == +inf (no finite bound) falls out as "keep", the table
// padding r2 == -inf as "cull", NaNs compare false, i.e. keep.
struct RayF {
  float ox, oy, oz, dx, dy, dz, a, s2, t_scale;
};

__device__ __forceinline__ RayF ray_f32(const Ray& r, float cmax) {
  RayF f;
  f.ox = static_cast<float>(r.ox);
  f.oy = static_cast<float>(r.oy);
  f.oz = static_cast<float>(r.oz);
  f.dx = static_cast<float>(r.dx);
  f.dy = static_cast<float>(r.dy);
  f.dz = static_cast<float>(r.dz);
  f.a = f.dx * f.dx + f.dy * f.dy + f.dz * f.dz;
  const float s = __builtin_sqrtf(f.ox * f.ox + f.oy * f.oy + f.oz * f.oz) + cmax;
  f.s2 = s * s;
  f.t_scale = 8e-6f * f.a;
  return f;
}

typedef float Float2 __attribute__((ext_vector_type(2)));
struct CullTables {  // what phase 1 of the root loop reads (in LDS where the world's tables fit): one of the two
  const RootCullPair* __restrict__ sphere;
  const RootBoxPair* __restrict__ box;
};

// Phase 1 of the root loop for TWO roots: the arithmetic runs as packed FP32 (v_pk_fma_f32 & co: one instruction per
// pair of roots), only the comparisons are per root.  Returns bit 0 / bit 1 = root 0 / 1 of the pair must be tested.
// SOLIDS (the containers pass of a simple world, RTC_CONTAINERS_SOLIDS): every bounded root is a sphere or a cube - two
// entries or none -, so a root whose bound lies entirely behind the origin has an even number of entries there and the
// pass, which uses a root only if that number is odd, has no use for it.  (An open surface - a triangle, an open cylinder -
// can have ONE: the other worlds keep it.)
template <class V, bool GROUPS, bool SOLIDS = false>
__device__ __forceinline__ uint32_t roots_kept(const RootCullPair& R, const RayF ray) {  // by value: by reference, three fields went through scratch memory
  // explicit FMAs: this file is compiled with contraction off for the FP64 path, but nothing here has
  // to round like the reference
  const Float2 ocx = R.cx - ray.ox, ocy = R.cy - ray.oy, ocz = R.cz - ray.oz;
  const Float2 b = __builtin_elementwise_fma(ocx, Float2(ray.dx), __builtin_elementwise_fma(ocy, Float2(ray.dy), ocz * ray.dz));
  const Float2 oc2 = __builtin_elementwise_fma(ocx, ocx, __builtin_elementwise_fma(ocy, ocy, ocz * ocz));
  const Float2 T = (oc2 + ray.s2) * ray.t_scale;       // 8e-6 * a * (oc^2 + S^2)
  const Float2 ac = (oc2 - R.r2) * ray.a;
  const Float2 bb = b * b;
  const Float2 disc = bb - ac;
  uint32_t kept = 0u;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const bool miss = disc[e] < -T[e];                    // the line misses the sphere
    // (lowest bit of r2 set: entries of this root may lie outside its bound - a cone in a group - and only `miss` holds)
    // (a world without groups - the simple kernel - has no such root and does not look)
    const bool line_only = GROUPS && (__builtin_bit_cast(uint32_t, static_cast<float>(R.r2[e])) & 1u) != 0u;
    const bool sided = (ac[e] > T[e]) & (bb[e] > T[e]) & !line_only;  // origin outside, sphere clearly on one side of it
    const bool behind = sided & (b[e] < 0.0f);            // entirely at t < 0
    const bool front = sided & (b[e] > 0.0f);             // entirely at t > 0
    const bool culled = miss | (behind & (V::kFrontOnly | SOLIDS)) | (front & V::kBehindOnly);
    kept |= culled ? 0u : (1u << e);
  }
  return kept;
}

// ---- the same rejection with the roots' WORLD-SPACE BOXES (RootBoxPair, rtc_device.h; trace<BOX>, round 5).  A ray's parameter at a plane x = p is (p - o) / d = p * (1 / d) + (-o / d): one FMA per plane with the
// per-ray part computed once, two roots per packed FMA; which of a box's two planes per axis is the near one is the
// ray's business (its direction signs pick the offsets the planes are read from).  The interval [max of the near
// parameters, min of the far ones] is where the LINE is inside the box: empty - no entry at all; entirely outside the
// range in which an entry can matter to the visitor (behind the origin for the closest hit and for shadows, beyond the
// light for shadows, in front of the origin for the containers pass) - none that matters.  Margins: every near
// parameter is lowered and every far one raised by (delta + par) * |1 / d|, delta = 1e-6 (|o| + largest box coordinate)
// for the FP32 arithmetic (see traverse_bvh8), par for the reference's "parallel" rule (DevScene::cull_par): a cube
// ignores a direction component below 1e-5 in its object space, so one of its entries can lie up to 1e-5 x the ray
// parameter x the cube's scale outside the cube along that axis.  NaNs keep (every comparison is "is it outside").
struct RayB {
  float ix, iy, iz;                       // 1 / d (a component of zero: 1e30 of its sign)
  float cnx, cny, cnz, cfx, cfy, cfz;     // -o / d - margin (near planes), -o / d + margin (far planes)
  uint32_t onx, ony, onz;                 // byte offsets of the near planes' pairs in a RootBoxPair (the far plane of an axis: the next pair)
  float t_lo, t_hi;                       // the parameter range in which an entry can matter to the visitor
};

template <class V>
__device__ __forceinline__ RayB ray_box(const Ray& r, const DevScene& S, const V& vis) {
  RayB b;
  const float ox = static_cast<float>(r.ox), oy = static_cast<float>(r.oy), oz = static_cast<float>(r.oz);
  float dx = static_cast<float>(r.dx), dy = static_cast<float>(r.dy), dz = static_cast<float>(r.dz);
  dx = __builtin_copysignf(fmaxf(__builtin_fabsf(dx), 1e-30f), dx);
  dy = __builtin_copysignf(fmaxf(__builtin_fabsf(dy), 1e-30f), dy);
  dz = __builtin_copysignf(fmaxf(__builtin_fabsf(dz), 1e-30f), dz);
  b.ix = __builtin_amdgcn_rcpf(dx);
  b.iy = __builtin_amdgcn_rcpf(dy);
  b.iz = __builtin_amdgcn_rcpf(dz);
  const float reach = fmaxf(fmaxf(__builtin_fabsf(ox), __builtin_fabsf(oy)), __builtin_fabsf(oz)) + S.cull_bmax;
  const float slack = 1e-6f * reach + S.cull_par * (4.0f * reach);  // (4 x reach: no entry of a bounded root is further along a ray of about unit length)
  const float mx = slack * __builtin_fabsf(b.ix), my = slack * __builtin_fabsf(b.iy), mz = slack * __builtin_fabsf(b.iz);
  const float cx = -ox * b.ix, cy = -oy * b.iy, cz = -oz * b.iz;
  b.cnx = cx - mx;
  b.cny = cy - my;
  b.cnz = cz - mz;
  b.cfx = cx + mx;
  b.cfy = cy + my;
  b.cfz = cz + mz;
  const bool nx = dx < 0.0f, ny = dy < 0.0f, nz = dz < 0.0f;
  b.onx = nx ? 8u : 0u;     // RootBoxPair: [lo][hi][lo] per axis - near, far = lo, hi or hi, lo
  b.ony = ny ? 32u : 24u;
  b.onz = nz ? 56u : 48u;
  vis.box_limits(b.t_lo, b.t_hi);
  return b;
}

// Two roots.  Returns bit 0 / bit 1 = root 0 / 1 of the pair must be tested.  `pair`: the record; ax / ay / az: the record's
// address + the ray's near-plane offsets (RayB::onx ...), formed ONCE per block of records by the caller - from there the
// records of a block are immediate offsets, and phase 1 has no address arithmetic left (it had twelve integer
// instructions per four roots, a fifth of the loop: the loop is a third of cover's vector instructions).
template <class V, bool GROUPS>
__device__ __forceinline__ uint32_t roots_kept_box(const char* __restrict__ pair, const char* __restrict__ ax, const char* __restrict__ ay,
                                                   const char* __restrict__ az, const RayB& rb) {
  const Float2 nx = *reinterpret_cast<const Float2*>(ax), fx = *reinterpret_cast<const Float2*>(ax + 8);
  const Float2 ny = *reinterpret_cast<const Float2*>(ay), fy = *reinterpret_cast<const Float2*>(ay + 8);
  const Float2 nz = *reinterpret_cast<const Float2*>(az), fz = *reinterpret_cast<const Float2*>(az + 8);
  const Float2 tnx = __builtin_elementwise_fma(nx, Float2(rb.ix), Float2(rb.cnx)), tny = __builtin_elementwise_fma(ny, Float2(rb.iy), Float2(rb.cny)),
               tnz = __builtin_elementwise_fma(nz, Float2(rb.iz), Float2(rb.cnz));
  const Float2 tfx = __builtin_elementwise_fma(fx, Float2(rb.ix), Float2(rb.cfx)), tfy = __builtin_elementwise_fma(fy, Float2(rb.iy), Float2(rb.cfy)),
               tfz = __builtin_elementwise_fma(fz, Float2(rb.iz), Float2(rb.cfz));
  uint32_t kept = 0u;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float tn = fmaxf(fmaxf(tnx[e], tny[e]), tnz[e]), tf = fminf(fminf(tfx[e], tfy[e]), tfz[e]);
    bool culled = fmaxf(tn, rb.t_lo) > fminf(tf, rb.t_hi);  // the line misses the box, or meets it only where no entry matters
    if constexpr (GROUPS) {
      // (entries of this root may lie outside its box - a cone in a group: only the line's missing the box holds)
      const float line_only = (*reinterpret_cast<const Float2*>(pair + 72))[e];
      culled = line_only != 0.0f ? tn > tf : culled;
    }
    kept |= culled ? 0u : (1u << e);
  }
  return kept;
}

// Four roots - two neighbouring records -, all twelve plane pairs fetched before any is used (the loads of a record wait
// for nothing but each other: taken one record at a time, every record's arithmetic waited for its own three loads).
template <class V, bool GROUPS>
__device__ __forceinline__ uint32_t roots_kept_box4(const char* __restrict__ pair, const char* __restrict__ ax, const char* __restrict__ ay,
                                                    const char* __restrict__ az, const RayB& rb) {
  constexpr uint32_t NEXT = sizeof(RootBoxPair);
  const Float2 nx[2] = {*reinterpret_cast<const Float2*>(ax), *reinterpret_cast<const Float2*>(ax + NEXT)};
  const Float2 fx[2] = {*reinterpret_cast<const Float2*>(ax + 8), *reinterpret_cast<const Float2*>(ax + NEXT + 8)};
  const Float2 ny[2] = {*reinterpret_cast<const Float2*>(ay), *reinterpret_cast<const Float2*>(ay + NEXT)};
  const Float2 fy[2] = {*reinterpret_cast<const Float2*>(ay + 8), *reinterpret_cast<const Float2*>(ay + NEXT + 8)};
  const Float2 nz[2] = {*reinterpret_cast<const Float2*>(az), *reinterpret_cast<const Float2*>(az + NEXT)};
  const Float2 fz[2] = {*reinterpret_cast<const Float2*>(az + 8), *reinterpret_cast<const Float2*>(az + NEXT + 8)};
  uint32_t kept = 0u;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const Float2 tnx = __builtin_elementwise_fma(nx[r], Float2(rb.ix), Float2(rb.cnx)), tny = __builtin_elementwise_fma(ny[r], Float2(rb.iy), Float2(rb.cny)),
                 tnz = __builtin_elementwise_fma(nz[r], Float2(rb.iz), Float2(rb.cnz));
    const Float2 tfx = __builtin_elementwise_fma(fx[r], Float2(rb.ix), Float2(rb.cfx)), tfy = __builtin_elementwise_fma(fy[r], Float2(rb.iy), Float2(rb.cfy)),
                 tfz = __builtin_elementwise_fma(fz[r], Float2(rb.iz), Float2(rb.cfz));
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float tn = fmaxf(fmaxf(tnx[e], tny[e]), tnz[e]), tf = fminf(fminf(tfx[e], tfy[e]), tfz[e]);
      bool culled = fmaxf(tn, rb.t_lo) > fminf(tf, rb.t_hi);
      if constexpr (GROUPS) {
        const float line_only = (*reinterpret_cast<const Float2*>(pair + r * NEXT + 72))[e];
        culled = line_only != 0.0f ? tn > tf : culled;
      }
      kept |= culled ? 0u : (1u << (2 * r + e));
    }
  }
  return kept;
}

// (RTC_ROOTS32) The same test for RECORDS x 2 roots whose survivor bits are SHIFTED INTO `m` from below, the last root
// first: the caller walks the table from its top record down, so after the walk root r's bit stands at bit r of the one
// 32-bit word.  A root is the same compare as above - `!(max(tn, t_lo) > min(tf, t_hi))`, a NaN keeps - and one add with
// carry, m + m + kept (v_addc_co_u32 with the compare's lane mask as its carry-in): two vector instructions where the
// form above has a compare, a select and an OR per root and the caller a 64-bit shift per step.  The adds are written
// as instructions because the compiler has no other way to them: from `m + m + kept` in the source it makes a select, a
// shift and an OR (twelve instructions per four roots).  The compares stay the compiler's (__builtin_amdgcn_fcmpf), which
// schedules them among the min / max.  (worlds without groups only: no `line_only`)
template <class V, int RECORDS>
__device__ __forceinline__ uint32_t roots_shifted_in_box(uint32_t m, const char* __restrict__ ax, const char* __restrict__ ay,
                                                         const char* __restrict__ az, const RayB& rb) {
  constexpr uint32_t NEXT = sizeof(RootBoxPair);
  static_assert(RECORDS == 1 || RECORDS == 2, "the half step and the step of four roots");
  Float2 nx[RECORDS], fx[RECORDS], ny[RECORDS], fy[RECORDS], nz[RECORDS], fz[RECORDS];
  unsigned long long kept[2 * RECORDS];  // per root: the wave's lanes that keep it
#pragma unroll
  for (int r = 0; r < RECORDS; ++r) {  // (all plane pairs fetched before any is used, as in roots_kept_box4)
    nx[r] = *reinterpret_cast<const Float2*>(ax + r * NEXT);
    fx[r] = *reinterpret_cast<const Float2*>(ax + r * NEXT + 8);
    ny[r] = *reinterpret_cast<const Float2*>(ay + r * NEXT);
    fy[r] = *reinterpret_cast<const Float2*>(ay + r * NEXT + 8);
    nz[r] = *reinterpret_cast<const Float2*>(az + r * NEXT);
    fz[r] = *reinterpret_cast<const Float2*>(az + r * NEXT + 8);
  }
#pragma unroll
  for (int r = RECORDS - 1; r >= 0; --r) {
    const Float2 tnx = __builtin_elementwise_fma(nx[r], Float2(rb.ix), Float2(rb.cnx)), tny = __builtin_elementwise_fma(ny[r], Float2(rb.iy), Float2(rb.cny)),
                 tnz = __builtin_elementwise_fma(nz[r], Float2(rb.iz), Float2(rb.cnz));
    const Float2 tfx = __builtin_elementwise_fma(fx[r], Float2(rb.ix), Float2(rb.cfx)), tfy = __builtin_elementwise_fma(fy[r], Float2(rb.iy), Float2(rb.cfy)),
                 tfz = __builtin_elementwise_fma(fz[r], Float2(rb.iz), Float2(rb.cfz));
#pragma unroll
    for (int e = 1; e >= 0; --e) {
      const float tn = fmaxf(fmaxf(tnx[e], tny[e]), tnz[e]), tf = fminf(fminf(tfx[e], tfy[e]), tfz[e]);
      kept[2 * r + e] = __builtin_amdgcn_fcmpf(fmaxf(tn, rb.t_lo), fminf(tf, rb.t_hi), 13);  // (13: unordered or <=, `!(a > b)`)
    }
  }
  // (s_nop 1: a lane mask written by a vector compare may be read by a vector instruction two wait states later at the
  // earliest, and the compiler pads nothing inside the string - the last compare may stand right in front of it.  Each
  // add writes its carry-out to vcc, which nothing reads.)
  if constexpr (RECORDS == 2) {
    asm("s_nop 1\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %1\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %2\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %3\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %4"
        : "+v"(m) : "s"(kept[3]), "s"(kept[2]), "s"(kept[1]), "s"(kept[0]) : "vcc");
  } else {
    asm("s_nop 1\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %1\n\t"
        "v_addc_co_u32_e64 %0, vcc, %0, %0, %2"
        : "+v"(m) : "s"(kept[1]), "s"(kept[0]) : "vcc");
  }
  return m;
}

// World.intersect's loop over World.objects (world.zig:74), two-phase so that no load depends on a
// previous one and no lane waits for roots only its neighbours need:
//   phase 1 streams the FP32 bounds (world boxes or bounding spheres: BOX) of up to 64 roots (wave-uniform addresses) and
//           leaves one survivor bit per root in a per-lane mask;
//   phase 2 lets every lane walk the set bits of ITS OWN mask and run the exact reference test on
//           the 144-byte-strided root records (per-lane LDS addresses; the stride spreads the banks).
// Rays of one wave are a mix of pixels and bounces after a few iterations, so the union of the lanes'
// survivors is most of the world while each lane's own list is 2-4 roots long.
// WORLD: 0 = anything (groups, csg: the root loop below visits the survivors in table order and walks the candidate BVH
// of a group); 1 = `flat`: no groups at all, every leaf kind; 2 = `simple`: top-level planes, spheres and cubes only.
// The flat and simple kernels carry none of the group traversal and run the exact tests one kind at a time.
// member / stride: a cooperative trace (render_body, COOP; worlds without groups only).  The `stride` lanes of an aligned
// group hold the same ray; lane `member` of the group takes every stride-th batch of four roots through both phases, and
// the group's visitors are merged at the end: what one lane does in five batches and three exact tests in a row, eight
// lanes do in one of each - the instruction stream of a wave with few rays left is what bounds it.  (0, 1): one lane, all.
// (MOTION) which root the trace is in: only the closest-hit visitor of the motion kernels keeps it (MotionClosestVisitor)
template <class V>
__device__ __forceinline__ void motion_root(V&, uint32_t) {}

// MOTION (the motion kernels only; a world with groups, one lane per ray): root r is tested at the lane's shutter time tm
// with the ray's origin shifted by -tm * D_r (DevMotion); phase 1 reads tables whose bounds already cover the motion.
// MAX_ROOTS: how many roots the kernel's world can have.  64: any number, in blocks of 64 (one 64-bit survivor mask per lane
// and block).  32 (RTC_ROOTS32; a three-wave simple kernel, whose worlds rtc_scene_create holds to RTC_LDS3_ROOTS): one
// block at base 0 and a 32-bit mask - no block loop, half the mask and bit-scan instructions, and a box form of phase 1
// that shifts its survivor bits into that one register (roots_shifted_in_box).  Which traces take it: render_body, ROOTS.
template <bool CSG, int WORLD, class V, int TRAV = RTC_LDS_TRAV, bool BOX = true, bool MOTION = false, int MAX_ROOTS = 64, bool OWN = false>
__device__ __forceinline__ void trace(const DevScene& S, const RootRec* __restrict__ recs,
                                      const CullTables& cull, const Ray& ray, V& vis, unsigned& overflow,
                                      uint32_t* lds_stack, const uint32_t member = 0u, const uint32_t stride = 1u,
                                      const double* __restrict__ disp = nullptr, const double tm = 0.0,
                                      const bool own_pass = false, const uint32_t own_root = 0u) {
  constexpr bool SIMPLE = WORLD == 2, FLAT = WORLD >= 1;
  constexpr bool R32 = MAX_ROOTS == 32;
  static_assert(MAX_ROOTS == 64 || (R32 && SIMPLE && RTC_LDS3_ROOTS == 32), "the 32-root form is the three-wave simple kernels'");
  using Mask = std::conditional_t<R32, uint32_t, unsigned long long>;  // one survivor bit per root of a block
  static_assert(!MOTION || WORLD == 0, "the motion kernels walk the general world");
  // Phase 1 rejects a root by its world BOX (BOX: every kernel that walks groups, the flat kernels, and the simple kernels
  // of worlds that are mostly cubes) or by its bounding SPHERE (the simple kernels of worlds that are mostly spheres): a
  // cube's box is the cube where its sphere lets through half of the rays that miss it, a group's box is far tighter than
  // the sphere around it, and a box says whether a root lies beyond a shadow ray's light - but a sphere's bounding sphere
  // is its own outline, which its box is 27 % wider than.  Measured, boxes against spheres: cover 0.497 -> 0.483 ms,
  // cubes 0.803 -> 0.748, groups 0.879 -> 0.745, csg_demo 2.49 -> 2.34, dragons 4K 1.74 -> 1.70, cylinders 0.242 -> 0.230;
  // reflection_and_refraction (seven spheres in a room of planes) 1.664 -> 1.738, skybox_demo 0.261 -> 0.272.  Both tests
  // in one kernel - spheres by spheres, the rest by boxes - lose to either (cover 0.496, reflection_and_refraction 1.785:
  // the three-wave kernel has no registers for two kinds of ray set-up): rtc_scene_create picks the kernel by what the
  // world is made of (profiles/r05/root_cull_boxes.md).
  // (RTC_CONTAINERS_SOLIDS) The containers pass uses a root only if an ODD number of its entries lies at t < 0
  // (BehindVisitor::flush; hit_dups is read only when the hit leaf is such a root).  In a simple world a bounded root is a sphere or
  // a cube - odd exactly when the origin is inside it -, so its bound must REACH the origin: the box interval by the margin of the
  // other two visitors, the sphere by roots_kept's SOLIDS (tests/test_containers_cpu.py).  On cover every one of the pass's
  // 21 813 wave steps of cube tests per frame was a cube behind the origin (profiles/containers/).
  constexpr bool kSolids = SIMPLE && RTC_CONTAINERS_SOLIDS && V::kBehindOnly;
  const auto rf = [&]() {
    if constexpr (BOX) {
      if constexpr (OWN) {
        if (own_pass) return RayB{};  // (no phase 1: no ray set-up)
      }
      RayB b = ray_box(ray, S, vis);
      if constexpr (kSolids) b.t_lo = -1.0002e-4f;
      return b;
    } else {
      if constexpr (OWN) {
        if (own_pass) return RayF{};
      }
      return ray_f32(ray, S.cull_cmax);
    }
  }();
  // (the table is sorted [spheres][cubes][the rest][planes]: a plane has no bound, phase 1 stops where the planes begin)
  const uint32_t n_bounded = S.n_roots - S.n_root_planes;
  // (R32: bits [0, x) of a 32-bit mask, x up to 32 - `(1u << 32) - 1u` is not defined, and 32 roots keep bit 31)
  [[maybe_unused]] const auto below32 = [](uint32_t x) -> uint32_t { return x >= 32u ? ~0u : (1u << x) - 1u; };
  // (R32: the one block, base 0 - the loop is gone once compiled; its `continue` below is why it is still written as one)
  for (uint32_t base = 0; base < (R32 ? 1u : S.n_roots); base += 64u) {
    const uint32_t n = R32 ? S.n_roots : min(64u, S.n_roots - base);
    const uint32_t nc = R32 ? n_bounded : (n_bounded > base ? min(n, n_bounded - base) : 0u);  // roots of this block that phase 1 tests
    Mask mine = 0u;
    RTC_PRIO_PHASE(BOX ? RTC_PRIO_CULL : RTC_PRIO_CULL_SPHERES);
    // the tables are padded with entries no ray keeps: the spheres to a multiple of four roots (r2 = -inf), the boxes to eight (lo > hi)
    if (OWN && own_pass) {  // (the lane's survivors are its hit root, whatever lane of a group it is)
      const uint32_t rel = own_root - base;
      if (rel < 64u) mine = Mask{1u} << rel;
    } else {
    if (BOX && FLAT && stride == 1u) {
      // (the kernels of worlds without groups, but for their cooperative iterations: four roots - two records - per step
      // off three per-lane addresses that move from step to step.  The kernels that walk groups have few top-level
      // objects and no registers for twelve plane pairs in flight: dragons 4K + 0.9 % with this form, so they keep the loop below)
      if constexpr (BOX) {
        // (the block loop itself is NOT unrolled: the simple kernels are 42 KB of code and run without a single
        // instruction-cache miss; unrolled eight times they were 60 KB and cover took twice as long)
        const char* block = reinterpret_cast<const char*>(cull.box + (base >> 1));
        const char* ax = block + rf.onx;
        const char* ay = block + rf.ony;
        const char* az = block + rf.onz;
#if RTC_CULL_HALF_STEP
        const uint32_t whole = (nc & 3u) > 2u ? nc : (nc & ~3u);  // (a remainder of one or two roots: one record, not two)
#else
        const uint32_t whole = nc;
#endif
#ifdef RTC_PROFILE
        // (the pairs this block reads: two per step of four roots, and one for the half step)
        const bool reads_ok = RTC_IN_BOUNDS(RTC_OOB_ROOTS, (base >> 1) + 2u * ((whole + 3u) >> 2) + (whole < nc ? 1u : 0u) <= RTC_AVAIL(2));
#else
        constexpr bool reads_ok = true;
#endif
        if constexpr (R32) {
          // The same records from the TOP down - the half step's one first, then the steps of four -, every root's bit
          // shifted into `mine` as it is formed: when the walk arrives at record 0, root r's bit stands at bit r (at most
          // 32 shifts: the table is padded to eight roots, and there are at most 32).  The three addresses carry the
          // table's base from before the loop and a step moves each by one add.
          const uint32_t steps = (whole + 3u) >> 2;  // steps of four roots
          ax += steps * (2u * static_cast<uint32_t>(sizeof(RootBoxPair)));
          ay += steps * (2u * static_cast<uint32_t>(sizeof(RootBoxPair)));
          az += steps * (2u * static_cast<uint32_t>(sizeof(RootBoxPair)));
#if RTC_CULL_HALF_STEP
          if (reads_ok && whole < nc) mine = roots_shifted_in_box<V, 1>(mine, ax, ay, az, rf);
#endif
#pragma unroll 1
          for (uint32_t step = steps; reads_ok && step != 0u; --step) {
            ax -= 2u * sizeof(RootBoxPair);
            ay -= 2u * sizeof(RootBoxPair);
            az -= 2u * sizeof(RootBoxPair);
            mine = roots_shifted_in_box<V, 2>(mine, ax, ay, az, rf);
          }
        } else {
#pragma unroll 1
          for (uint32_t first = 0; reads_ok && first < whole; first += 4u) {
            const uint32_t k = roots_kept_box4<V, !FLAT>(block, ax, ay, az, rf);
            mine |= static_cast<unsigned long long>(k) << first;
            block += 2u * sizeof(RootBoxPair);
            ax += 2u * sizeof(RootBoxPair);
            ay += 2u * sizeof(RootBoxPair);
            az += 2u * sizeof(RootBoxPair);
          }
#if RTC_CULL_HALF_STEP
          if (reads_ok && whole < nc) mine |= static_cast<unsigned long long>(roots_kept_box<V, !FLAT>(block, ax, ay, az, rf)) << whole;
#endif
        }
      }
    } else {
      for (uint32_t i = 4u * member; i < nc; i += 4u * stride) {
#ifdef RTC_PROFILE
        if (!RTC_IN_BOUNDS(RTC_OOB_ROOTS, ((base + i) >> 1) + ((BOX && !(i + 2u < nc)) ? 1u : 2u) <= RTC_AVAIL(BOX ? 2 : 1))) continue;
#endif
        Mask k;
        if constexpr (BOX) {
          const char* const p0 = reinterpret_cast<const char*>(cull.box + ((base + i) >> 1));
          const char* const p1 = p0 + sizeof(RootBoxPair);
          k = roots_kept_box<V, !FLAT>(p0, p0 + rf.onx, p0 + rf.ony, p0 + rf.onz, rf);
          // (a remainder of one or two roots - teapot.json has two top-level objects, dragons.json six - is one record's work)
          if (i + 2u < nc) k |= roots_kept_box<V, !FLAT>(p1, p1 + rf.onx, p1 + rf.ony, p1 + rf.onz, rf) << 2;
        } else {
          const RootCullPair p0 = cull.sphere[(base + i) >> 1], p1 = cull.sphere[((base + i) >> 1) + 1u];
          k = roots_kept<V, !FLAT, kSolids>(p0, rf) | (roots_kept<V, !FLAT, kSolids>(p1, rf) << 2);
        }
        mine |= k << i;
      }
    }
    if constexpr (R32) {
      mine &= below32(nc);
    } else {
      if (nc < 64u) mine &= (1ull << nc) - 1ull;  // (the padding is never kept; a NaN ray must not reach past the table either)
    }
    if (nc < n) {  // the block's planes: kept as they are (what the bound of a plane, none, always said)
      Mask planes;
      if constexpr (R32) planes = below32(n) & ~below32(nc);  // (bits [nc, n), n up to 32)
      else planes = (n < 64u ? (1ull << n) - 1ull : ~0ull) & ~((1ull << nc) - 1ull);
      if (stride != 1u) {  // (a cooperative trace: root r is lane ((r / 4) % stride)'s, as in the loop above)
        Mask own = Mask{0xFu} << (4u * member);
        if (stride == 4u) own |= own << 16;
        if constexpr (!R32) own |= own << 32;
        planes &= own;
      }
      mine |= planes;
    }
    }  // (not an own_pass)
    RTC_PRIO_PHASE(RTC_PRIO_WORK);
    // Phase 2, one kind at a time.  The table is sorted [spheres][cubes][everything else][planes] (rtc_scene_create), so
    // a kind is a range of bits.  A wave that walks its lanes' survivors in table order runs the plane, the sphere AND
    // the cube code in almost every step (some lane holds one of each); kind by kind it runs each test's code only as
    // often as the lane with the most survivors of that kind needs it, and the compiler drops what a kind does not use
    // (a plane needs one row of the inverse).  Visiting order is free: the reductions do not depend on it.
    auto range = [&](uint32_t lo, uint32_t hi) -> Mask {  // bits of roots [lo, hi) that fall into this block
      if constexpr (R32) {
        return below32(hi) & ~below32(lo);
      } else {
        const uint32_t a = max(lo, base) - base, b = min(max(hi, base), base + 64u) - base;
        const unsigned long long below_b = b >= 64u ? ~0ull : (1ull << b) - 1ull;
        const unsigned long long below_a = a >= 64u ? ~0ull : (1ull << a) - 1ull;
        return below_b & ~below_a;
      }
    };
#if defined(RTC_PROFILE) && !defined(RTC_PROFILE_LITE)
    uint32_t cube_tests = 0u, cube_neg = 0u, cube_pred = 0u;  // this lane's exact cube tests of the block; those with tmax < 0; those cube_entirely_behind names
#endif
    // (cube_entirely_behind stands in the shadow traces of rtc_render_kernel_simple_b / _simple3_b - worlds of cubes - and
    // nowhere else: in closest-hit traces, in the other kernels without groups and in the `while (mine)` path it was
    // measured and lost)
    constexpr bool kCubeBehind = SIMPLE && BOX && V::kAnyHit && V::kFrontOnly && RTC_CUBE_BEHIND_EARLY_OUT;
    auto leaf_of_kind = [&](auto kind_tag, const uint32_t root) {
      constexpr uint32_t KIND = decltype(kind_tag)::value;
      const RootRec& R = recs[RTC_CHECK_INDEX(RTC_OOB_ROOTS, root, RTC_AVAIL(0))];
      const uint32_t kf = R.kind_flags;
      const Ray lr = xform_ray(R.inv, ray);  // Shape.intersect: ray.transform(_inverse_transform)
      const CylParams cy{0.0, 0.0, false};
      const uint32_t leaf = R.index, shadow = (kf >> 8) & 1u, material = R.material;
      vis.set_root(root);
      if constexpr (KIND == 2u && V::kAnyHit && RTC_ROOM_EARLY_OUT) {
        if ((kf & RTC_ROOT_ROOM) && segment_stays_inside_cube(lr, vis.t_limit())) return;
      }
#if defined(RTC_PROFILE) && !defined(RTC_PROFILE_LITE)
      if constexpr (KIND == 2u) {  // (what cube_entirely_behind can save at most, and what it does save: cube_counts below)
        double c_tmin, c_tmax;
        cube_slab(lr, c_tmin, c_tmax);
        const bool neg = c_tmax < 0.0, pred = cube_entirely_behind(lr);
        constexpr uint32_t K = V::kAnyHit ? 6u : (V::kBehindOnly ? 12u : 0u);
        RTC_CUBE_ADD(K + 0u, __builtin_popcountll(__ballot(true)));
        RTC_CUBE_ADD(K + 1u, __builtin_popcountll(__ballot(neg)));
        RTC_CUBE_ADD(K + 2u, __builtin_popcountll(__ballot(pred)));
        RTC_CUBE_ADD(K + 3u, 1);
        cube_neg += neg ? 1u : 0u;
        cube_pred += pred ? 1u : 0u;
        cube_tests += 1u;
      }
#endif
      if constexpr (KIND == 2u && kCubeBehind) {
        if (cube_entirely_behind(lr)) return;
      }
      if constexpr (KIND == 1u && V::kFrontOnly && RTC_PLANE_EARLY_OUT) {
        // A plane's one entry is t = -o.y / d.y (plane.zig:25-36), and the division is 13 of the test's ~35 instructions.
        // A closest-hit or a shadow trace looks at an entry only if 0 <= t and t < (or <=) its limit - the best hit so
        // far, the light's distance - and BOTH can be decided without the quotient, exactly:
        //   * o.y and d.y of one sign: the quotient is negative - and, with |o.y| >= 1e-290 and |d.y| <= 1e10, at least
        //     1e-300 in magnitude, so it cannot round to -0 (which `t >= 0` would let through);
        //   * |o.y| > limit x |d.y| x (1 + 1e-12): the exact quotient exceeds limit x (1 + 0.9997e-12) (two roundings of
        //     2^-53 in the product), so the correctly rounded one exceeds the limit.  An infinite limit or an overflowing
        //     product compares false: the division runs.
        // A light inside a room never has a wall between itself and a point of the room: EVERY plane test of EVERY shadow ray
        // of reflection_and_refraction ends here, for the whole wave.
        if (__builtin_fabs(lr.dy) > 1e-5) {
          const double ao = __builtin_fabs(lr.oy), ad = __builtin_fabs(lr.dy);
          const bool negative = ((lr.oy > 0.0) == (lr.dy > 0.0)) & (ao >= 1e-290) & (ad <= 1e10);
          const bool beyond = ao > (vis.t_limit() * ad) * (1.0 + 1e-12);
          if (!(negative | beyond)) vis.entry(leaf, shadow, material, -lr.oy / lr.dy, 0.0, 0.0);
        }
      } else if constexpr (KIND == 1u && kSolids) {
        // The pass looks at a plane's one entry t = -o.y / d.y only if t < 0 (the plane's own `t == hit_t` counts for hit_dups,
        // which is read only when the hit leaf is open - and the plane that was hit at t >= 0 is not).  o.y and d.y of
        // different signs - `o.y > 0` against `d.y > 0`, a zero or a NaN on the side of the negatives - give a quotient that
        // is positive, a zero of either sign or a NaN: none is < 0, and the division is not made.
        if (__builtin_fabs(lr.dy) > 1e-5 && (lr.oy > 0.0) == (lr.dy > 0.0)) vis.entry(leaf, shadow, material, -lr.oy / lr.dy, 0.0, 0.0);
      } else {
        leaf_entries<SIMPLE>(KIND, cy, nullptr, lr, [&](double t, double u, double v) { vis.entry(leaf, shadow, material, t, u, v); });
      }
    };
    auto leaves_of_kind = [&](auto kind_tag, Mask m) {
      while (m != 0u && !vis.done()) {
        const uint32_t bit = static_cast<uint32_t>(R32 ? __builtin_ctz(static_cast<uint32_t>(m)) : __builtin_ctzll(m));
        m &= m - Mask{1u};
        if constexpr (V::kBehindOnly) RTC_AUX_ADD(4, 1);  // (diagnostic builds: wave steps of the containers pass's exact tests)
        leaf_of_kind(kind_tag, base + bit);
      }
    };
    // (The kernels without group traversal are built this way: reflection_and_refraction depth 8 2.74 -> 2.22 ms,
    // cover 0.730 -> 0.698; in the kernels that also carry the group traversal the three extra loops cost the mesh
    // scenes 1-2 % and their worlds have few top-level objects.)
    if constexpr (FLAT) {
      const uint32_t k1 = S.n_root_spheres, k2 = k1 + S.n_root_cubes;
      if (stride == 1u || (OWN && own_pass)) {
        // Every lane holds every plane of the block (phase 1 has no say about them): the loop over them is the WAVE's -
        // one record address for all lanes, no per-lane bit scan, no integer multiply for a per-lane record address
        // (reflection_and_refraction runs six plane tests in every one of its 45 M traces).
        // (the planes of the block are its roots [base + nc, base + n).  The loop used to start at max(n_bounded, base) -
        // the same iterations in the source - and a world of 63 bounded roots whose planes reach into a second block
        // rendered a dozen pixels off the oracle, with fewer shadow rays, in one-lane traces only: the compiled loop did
        // not do what the source says.  Started at `base` with the bounded roots skipped, or with the planes taken from
        // `mine` as a cooperative trace takes them, it was exact; so is this form.  tests/test_table_limits_gpu.py, bounded63-*)
        const uint32_t p1 = (OWN && own_pass) ? base + nc : base + n;  // (own_pass: the hit root is a sphere or a cube - an empty loop, whatever the stride)
        for (uint32_t root = base + nc; root < p1; ++root) {
          if (__all(vis.done())) break;
          if constexpr (V::kBehindOnly) RTC_AUX_ADD(4, 1);
          if (!vis.done()) leaf_of_kind(std::integral_constant<uint32_t, 1u>{}, root);
        }

      } else {
        leaves_of_kind(std::integral_constant<uint32_t, 1u>{}, mine & range(n_bounded, S.n_roots));
      }
      leaves_of_kind(std::integral_constant<uint32_t, 0u>{}, mine & range(0u, k1));
      leaves_of_kind(std::integral_constant<uint32_t, 2u>{}, mine & range(k1, k2));
#if defined(RTC_PROFILE) && !defined(RTC_PROFILE_LITE)
      {  // the cube loop is as long as its lane with the most tests: the wave-level steps that would remain without the
         // tests whose interval ends behind the origin, and without those the early-out names
        constexpr uint32_t K = V::kAnyHit ? 6u : (V::kBehindOnly ? 12u : 0u);
        uint32_t left_neg = 0u, left_pred = 0u;
        while (__ballot(cube_tests - cube_neg > left_neg) != 0ull) ++left_neg;
        while (__ballot(cube_tests - cube_pred > left_pred) != 0ull) ++left_pred;
        RTC_CUBE_ADD(K + 4u, left_neg);
        RTC_CUBE_ADD(K + 5u, left_pred);
      }
#endif
      if constexpr (SIMPLE) continue;  // (a simple world has nothing else)
      mine &= range(k2, n_bounded);    // the other leaf kinds: cylinders, cones, triangles
    }
    while (mine != 0ull && !vis.done()) {
      const uint32_t bit = static_cast<uint32_t>(__builtin_ctzll(mine));
      mine &= mine - 1ull;
      const RootRec& R = recs[RTC_CHECK_INDEX(RTC_OOB_ROOTS, base + bit, RTC_AVAIL(0))];
      const uint32_t kf = R.kind_flags;
      // (MOTION: this root's ray, the origin shifted by -tm * D - with D = 0 the same bits; every other kernel tests `ray`
      // itself: a copy of it, even an unchanged one, moves their register allocation)
      Ray shifted;
      if constexpr (MOTION) {
        const double* __restrict__ D = disp + 3ull * (base + bit);
        shifted = ray;
        shifted.ox = ray.ox - tm * D[0];
        shifted.oy = ray.oy - tm * D[1];
        shifted.oz = ray.oz - tm * D[2];
        motion_root(vis, base + bit);
      }
      const Ray& root_ray = MOTION ? shifted : ray;
      if (FLAT || !(kf & RTC_ROOT_IS_GROUP)) {
        if (!FLAT && V::kShadowOnly && ((kf >> 8) & 1u) == 0u) continue;  // (a shadow trace: a shape that casts no shadow, see visit_leaf)
        const Ray lr = xform_ray(R.inv, root_ray);  // Shape.intersect: ray.transform(_inverse_transform)
        if constexpr (V::kAnyHit && RTC_ROOM_EARLY_OUT) {
          if ((kf & RTC_ROOT_ROOM) && segment_stays_inside_cube(lr, vis.t_limit())) continue;
        }
        const CylParams cy{R.ymin, R.ymax, ((kf >> 9) & 1u) != 0u};
        const uint32_t leaf = R.index, shadow = (kf >> 8) & 1u, material = R.material;
        vis.set_root(base + bit);
        leaf_entries<SIMPLE>(kf & 0xFFu, cy, S.tri + 9ull * R.geom, lr,
                             [&](double t, double u, double v) { vis.entry(leaf, shadow, material, t, u, v); });
        continue;
      }
      vis.set_root(RTC_NO_LEAF);
      if constexpr (!FLAT) {
        if (CSG && (kf & RTC_ROOT_IS_CSG)) {
          if constexpr (CSG) visit_csg(S, R.index, root_ray, vis, overflow);
        } else {
#if RTC_BVH8
          // (the three-wave kernel only: measured with and without it, dragons 4K 1.884 -> 1.859 ms and groups 0.890 -> 0.875
          // there; the two-wave kernel loses a per cent - teapot 0.256 -> 0.258, nefertiti 0.489 -> 0.495 -
          // profiles/r05/walk_experiments.md)
          traverse_bvh8<CSG, V, TRAV>(S, R.geom, R.always_first, R.always_count, root_ray, vis, overflow, reinterpret_cast<uint2*>(lds_stack),
                                      (RTC_ROOT_NODE_IN_REC && TRAV == 2) ? reinterpret_cast<const uint4*>(R.inv) : nullptr);
#else
          traverse_bvh<CSG>(S, R.geom, root_ray, vis, overflow, lds_stack);
#endif
        }
      }
    }  // while (mine)
  }
  if constexpr (FLAT) {
    if (stride > 1u && !(OWN && own_pass)) vis.merge_group(stride);  // (a cooperative trace: every lane of the group leaves with the group's result)
  }
}

// Butterfly over an aligned group of eight lanes with DPP moves (one VALU instruction per dword and step, no LDS crossbar):
// step 0 swaps neighbours (quad_perm [1,0,3,2]), step 1 pairs (quad_perm [2,3,0,1]), step 2 mirrors the half row
// (lane i <-> 7 - i: after the first two steps the four lanes of a quad agree, so any lane of the other quad will do).
template <int STEP>
__device__ __forceinline__ uint32_t group8_other(uint32_t x) {
  constexpr int ctrl = STEP == 0 ? 0xB1 : (STEP == 1 ? 0x4E : 0x141);
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), ctrl, 0xF, 0xF, false));
}
template <int STEP>
__device__ __forceinline__ double group8_other(double x) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  const unsigned long long o = static_cast<unsigned long long>(group8_other<STEP>(static_cast<uint32_t>(b))) |
                               (static_cast<unsigned long long>(group8_other<STEP>(static_cast<uint32_t>(b >> 32))) << 32);
  return __builtin_bit_cast(double, o);
}

// hit(): first entry with t >= 0 of the stably sorted list (shape.zig:71-80) ==
// lexicographic min of (t, depth-first leaf index) over entries with t >= 0.
struct ClosestVisitor {
  static constexpr bool kAnyHit = false;  // the first entry that counts ends the trace: visiting order is free
  static constexpr bool kShadowOnly = false;  // only entries of leaves that cast a shadow count: the others are not even tested
  double t = kInf;
  uint32_t leaf = RTC_NO_LEAF;
  uint32_t root = RTC_NO_LEAF;      // World.objects index when the hit leaf IS a top-level object
  uint32_t cur_root = RTC_NO_LEAF;
  double u = 0.0, v = 0.0;
  __device__ __forceinline__ void set_root(uint32_t r) { cur_root = r; }
  static constexpr bool kFrontOnly = true;    // entries with t < 0 never matter
  static constexpr bool kBehindOnly = false;
  __device__ __forceinline__ double t_limit() const { return t; }
  __device__ __forceinline__ void entry(uint32_t l, uint32_t, uint32_t, double et, double eu, double ev) {
    if (et >= 0.0 && (et < t || (et == t && l < leaf))) {
      t = et;
      leaf = l;
      root = cur_root;
      u = eu;
      v = ev;
    }
  }
  __device__ __forceinline__ bool relevant(uint32_t l, uint32_t, double et) const {
    return et >= 0.0 && (et < t || (et == t && l < leaf));
  }
  __device__ __forceinline__ bool cullf(float tn, float tf) const {  // FP32 box interval of the candidate BVH
    const float best = static_cast<float>(t);
    return tf < -1e-4f * (1.0f + __builtin_fabsf(tf)) || tn > best + 1e-4f * (1.0f + __builtin_fabsf(tn) + __builtin_fabsf(best));
  }
  // cullf() with the part that does not depend on the box taken out of the per-child code (traverse_bvh computes the
  // limit once per node): tn > best + 1e-4 (1 + |tn| + |best|) is, for best >= 0, tn > (best (1 + 1e-4) + 1e-4) / (1 - 1e-4)
  // - the limit below, rounded up - and tf < -1e-4 (1 + |tf|) is tf < -1e-4 / (1 - 1e-4).
  __device__ __forceinline__ float far_limit() const { return (static_cast<float>(t) * 1.0001f + 1.0001e-4f) * 1.0002f; }
  __device__ __forceinline__ bool cull_limits(float tn, float tf, float limit) const { return (tf < -1.0002e-4f) | (tn > limit); }
  // (the same two rules as an interval a box's [tn, tf] must meet: traverse_bvh8)
  __device__ __forceinline__ void box_limits(float& lo, float& hi) const { lo = -1.0002e-4f; hi = far_limit(); }
  __device__ __forceinline__ bool done() const { return false; }
  // Cooperative trace (render_body, COOP): the eight lanes of an aligned group hold the SAME ray and have each tested a
  // share of World.objects; the lexicographic min of their results - the reduction is symmetric, so after three butterfly
  // steps every lane of the group holds it.
  template <int STEP>
  __device__ __forceinline__ void merge_step() {
    const double ot = group8_other<STEP>(t), ou = group8_other<STEP>(u), ov = group8_other<STEP>(v);
    const uint32_t ol = group8_other<STEP>(leaf), oroot = group8_other<STEP>(root);
    if (ot < t || (ot == t && ol < leaf)) {
      t = ot;
      leaf = ol;
      root = oroot;
      u = ou;
      v = ov;
    }
  }
  __device__ __forceinline__ void merge_group(uint32_t group) {  // group: 8 or 4 lanes (wave-uniform)
    merge_step<0>();
    merge_step<1>();
    if (group > 4u) merge_step<2>();
  }
};

// (MOTION) the closest hit and the root it lies under - a top-level object, a group or a csg unit -: the shading of a
// moving root needs its displacement.  Found by ADL from trace() (unused where only the other kernels are compiled).
struct MotionClosestVisitor : ClosestVisitor {
  uint32_t hit_root = RTC_NO_LEAF, in_root = RTC_NO_LEAF;
  __device__ __forceinline__ void entry(uint32_t l, uint32_t s, uint32_t m, double et, double eu, double ev) {
    if (relevant(l, s, et)) hit_root = in_root;
    ClosestVisitor::entry(l, s, m, et, eu, ev);
  }
};
[[maybe_unused]] __device__ __forceinline__ void motion_root(MotionClosestVisitor& v, uint32_t r) { v.in_root = r; }

// isShadowed (world.zig:126-154): any entry with 0 <= t < distance on a casts_shadow leaf.
struct ShadowVisitor {
  static constexpr bool kAnyHit = true;  // the first entry that counts ends the trace: visiting order is free
  static constexpr bool kShadowOnly = true;
  double distance;
  bool shadowed = false;
  __device__ __forceinline__ void set_root(uint32_t) {}
  static constexpr bool kFrontOnly = true;
  static constexpr bool kBehindOnly = false;
  __device__ __forceinline__ double t_limit() const { return distance; }
  __device__ __forceinline__ void entry(uint32_t, uint32_t casts_shadow, uint32_t, double et, double, double) {
    if (et >= 0.0 && et < distance && casts_shadow) shadowed = true;
  }
  __device__ __forceinline__ bool relevant(uint32_t, uint32_t casts_shadow, double et) const {
    return et >= 0.0 && et < distance && casts_shadow;
  }
  __device__ __forceinline__ bool cullf(float tn, float tf) const {
    const float lim = static_cast<float>(distance);
    return tf < -1e-4f * (1.0f + __builtin_fabsf(tf)) || tn > lim + 1e-4f * (1.0f + __builtin_fabsf(tn) + __builtin_fabsf(lim));
  }
  __device__ __forceinline__ float far_limit() const { return (static_cast<float>(distance) * 1.0001f + 1.0001e-4f) * 1.0002f; }
  __device__ __forceinline__ bool cull_limits(float tn, float tf, float limit) const { return (tf < -1.0002e-4f) | (tn > limit); }
  __device__ __forceinline__ void box_limits(float& lo, float& hi) const { lo = -1.0002e-4f; hi = far_limit(); }
  __device__ __forceinline__ bool done() const { return shadowed; }
  __device__ __forceinline__ void merge_group(uint32_t group) {  // any lane of the aligned group of eight (or four)
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    shadowed = ((__ballot(shadowed) >> (lane & ~(group - 1u))) & ((1ull << group) - 1ull)) != 0ull;
  }
};

// A light's isShadowed with shadow filters (rtc.h's rtc_scene_set_shadow_filters): the product of the
// filter rows of EVERY entry with 0 <= t < distance on a casts_shadow leaf - the entries ShadowVisitor::relevant accepts.
// Not an any-hit walk: the walk hands every entry over exactly once, as it does to the containers pass, which counts them;
// what kAnyHit would select besides - the slot-order descent, the room and cube early-outs that answer for a box without
// enumerating its entries - stays off.  kShadowOnly keeps what holds for every walk that wants casts_shadow entries only:
// leaves and leaf ranges that cast none are not fetched.  The trace may stop once all three channels are zero: a zero
// factor gives exactly zero whatever follows.  The row is read by the lane that found the entry.  Compiled into the
// shadow-filter kernels' translation unit only: no other unit has a use for it.
#ifdef RTC_SFILT_TU
struct FilterVisitor {
  static constexpr bool kAnyHit = false;
  static constexpr bool kShadowOnly = true;
  double distance;
  double tr = 1.0, tg = 1.0, tb = 1.0;  // the transmittance so far
  const double* __restrict__ filter;    // DevShadowFilter::row, [n_materials][3]
  __device__ __forceinline__ void set_root(uint32_t) {}
  static constexpr bool kFrontOnly = true;
  static constexpr bool kBehindOnly = false;
  __device__ __forceinline__ double t_limit() const { return distance; }
  __device__ __forceinline__ void entry(uint32_t, uint32_t casts_shadow, uint32_t material, double et, double, double) {
    if (et >= 0.0 && et < distance && casts_shadow) {
      const double* __restrict__ f = filter + 3ull * material;
      tr = tr * f[0];
      tg = tg * f[1];
      tb = tb * f[2];
    }
  }
  __device__ __forceinline__ bool relevant(uint32_t, uint32_t casts_shadow, double et) const {
    return et >= 0.0 && et < distance && casts_shadow;
  }
  // (the box rules are ShadowVisitor's: an entry counts in the same range)
  __device__ __forceinline__ bool cullf(float tn, float tf) const {
    const float lim = static_cast<float>(distance);
    return tf < -1e-4f * (1.0f + __builtin_fabsf(tf)) || tn > lim + 1e-4f * (1.0f + __builtin_fabsf(tn) + __builtin_fabsf(lim));
  }
  __device__ __forceinline__ float far_limit() const { return (static_cast<float>(distance) * 1.0001f + 1.0001e-4f) * 1.0002f; }
  __device__ __forceinline__ bool cull_limits(float tn, float tf, float limit) const { return (tf < -1.0002e-4f) | (tn > limit); }
  __device__ __forceinline__ void box_limits(float& lo, float& hi) const { lo = -1.0002e-4f; hi = far_limit(); }
  __device__ __forceinline__ bool done() const { return tr == 0.0 && tg == 0.0 && tb == 0.0; }  // blocked
  // (a cooperative trace: every lane of the group multiplied the factors of its own share of the roots; the butterfly's
  // two sides form the same product of two, which commutes exactly, so every lane leaves with the same bits)
  template <int STEP>
  __device__ __forceinline__ void merge_step() {
    tr = tr * group8_other<STEP>(tr);
    tg = tg * group8_other<STEP>(tg);
    tb = tb * group8_other<STEP>(tb);
  }
  __device__ __forceinline__ void merge_group(uint32_t group) {
    merge_step<0>();
    merge_step<1>();
    if (group > 4u) merge_step<2>();
  }
};
#endif

// A sun's isShadowed (rtc.h's rtc_scene_set_environment): FilterVisitor without a far end.  The limit
// is +infinity for every box rule - `tn > inf` is false, and no rule multiplies the limit by a zero or subtracts it from
// itself -, and an entry counts on `et >= 0` alone, not on `et < distance`: a cube whose local direction is shorter than
// the reference's 1e-5 on every axis answers with entries at -inf and +inf (cube.zig's check_axis), and the one at +inf
// is an entry with et >= 0 however far away - `inf < inf` would drop it.  A NaN fails `et >= 0` as it does everywhere.
// Compiled into the environment kernels' translation unit only.
#ifdef RTC_ENV_TU
struct SunVisitor : FilterVisitor {
  __device__ __forceinline__ void entry(uint32_t, uint32_t casts_shadow, uint32_t material, double et, double, double) {
    if (et >= 0.0 && casts_shadow) {
      const double* __restrict__ f = filter + 3ull * material;
      tr = tr * f[0];
      tg = tg * f[1];
      tb = tb * f[2];
    }
  }
  __device__ __forceinline__ bool relevant(uint32_t, uint32_t casts_shadow, double et) const { return et >= 0.0 && casts_shadow; }
};
#endif

// The walk of the emitter unit's suns' loop (rtc.h's rtc_scene_set_emitters): a sun's and a sky-light
// sample's iterations keep SunVisitor's rule - `distance` is +infinity and an entry counts on et >= 0 alone, the +inf entries
// of a degenerate cube included -, an emitter sample's has a far end, the emitter's distance less 1e-4, and an entry
// counts as FilterVisitor's does, on et < distance as well.  `bounded` says which; it is wave-uniform, as the iteration's
// kind is.  Compiled into the emitter kernels' translation unit only.
#ifdef RTC_EMIT_TU
struct EmitVisitor : FilterVisitor {
  bool bounded = false;
  __device__ __forceinline__ void entry(uint32_t, uint32_t casts_shadow, uint32_t material, double et, double, double) {
    if (et >= 0.0 && (!bounded || et < distance) && casts_shadow) {
      const double* __restrict__ f = filter + 3ull * material;
      tr = tr * f[0];
      tg = tg * f[1];
      tb = tb * f[2];
    }
  }
  __device__ __forceinline__ bool relevant(uint32_t, uint32_t casts_shadow, double et) const {
    return et >= 0.0 && (!bounded || et < distance) && casts_shadow;
  }
};
#endif

// The containers walk of PreComputations.new (world.zig:229-255), as a reduction.
// Entries before the hit in the sorted list are exactly those with t < 0.  A leaf with an
// odd number of them is still in `containers` when the hit is reached, at the position of
// its LAST such entry (its final toggle is an append), so
//   n1 = ior of the open leaf whose last t<0 entry is latest in (t, leaf order), else 1;
//   n2 = ior of the hit leaf if it was not open (it gets appended), else ior of the latest
//        open leaf other than the hit leaf, else 1 (or the hit leaf again if it has a second
//        entry at exactly t_hit: the reference does not `break` on an empty list).
// Identity is the leaf index; rtc_scene_create rejects scenes whose leaves share a Shape.id.
// SELECTS (the simple kernels): "is this open leaf the later one" updates its three fields with selects on one condition.
// Written as a branch - the form every other kernel keeps, instruction for instruction - the simple kernels' last flush was
// compiled to code that, on a TIE in t (cur_last == best_t, the larger leaf wins), moved the leaf but kept the earlier
// leaf's material: two glass spheres with one transform and different refractive indices gave n1 of the wrong sphere
// (rtc_render_kernel_simple3: the material's move stood inside the not-greater branch, in front of the tie's decision;
// profiles/containers/flush_tie_isa.txt holds those instructions; tests/test_containers_gpu.py, `ties` and `ties3`).
template <bool SELECTS>
struct BehindVisitorT {
  static constexpr bool kAnyHit = false;  // the first entry that counts ends the trace: visiting order is free
  static constexpr bool kShadowOnly = false;
  uint32_t hit_leaf;
  double hit_t;
  // running state of the leaf currently being visited (entries of one leaf arrive together)
  uint32_t cur = RTC_NO_LEAF;
  uint32_t cur_cnt = 0;
  double cur_last = -kInf;
  uint32_t cur_mat = 0;
  // results
  double best_t = -kInf, best_excl_t = -kInf;
  uint32_t best_leaf = RTC_NO_LEAF, best_excl_leaf = RTC_NO_LEAF;
  uint32_t best_mat = 0, best_excl_mat = 0;
  bool hit_open = false;
  uint32_t hit_dups = 0;
  __device__ __forceinline__ void set_root(uint32_t) {}
  // (SELECTS) is the open leaf (bt, bl) later than (at, al)?  bl is a leaf
  static __device__ __forceinline__ bool later_than(double at, uint32_t al, double bt, uint32_t bl) {
    return (bt > at) | ((bt == at) & ((al == RTC_NO_LEAF) | (bl > al)));
  }

  // LAST: the flush after a leaf's last entry that no other entry follows (render_body's after the trace, merge_group's) - the
  // copy that was compiled wrongly; the flushes between two leaves (entry()) stay branches in every kernel: with selects
  // there as well fresnel lost 3.7 % and reflection_and_refraction 1.9 % (profiles/containers/times_1080p_depth5.txt)
  template <bool LAST = false>
  __device__ __forceinline__ void flush() {
    if constexpr (SELECTS && LAST) {
      const bool open = cur != RTC_NO_LEAF && (cur_cnt & 1u) != 0u;
      const bool is_hit = cur == hit_leaf;
      const bool take = open && later_than(best_t, best_leaf, cur_last, cur);
      const bool take_excl = open && !is_hit && later_than(best_excl_t, best_excl_leaf, cur_last, cur);
      best_t = take ? cur_last : best_t;
      best_leaf = take ? cur : best_leaf;
      best_mat = take ? cur_mat : best_mat;
      best_excl_t = take_excl ? cur_last : best_excl_t;
      best_excl_leaf = take_excl ? cur : best_excl_leaf;
      best_excl_mat = take_excl ? cur_mat : best_excl_mat;
      hit_open = hit_open || (open && is_hit);
    } else if (cur != RTC_NO_LEAF && (cur_cnt & 1u)) {
      if (cur_last > best_t || (cur_last == best_t && (best_leaf == RTC_NO_LEAF || cur > best_leaf))) {
        best_t = cur_last;
        best_leaf = cur;
        best_mat = cur_mat;
      }
      if (cur == hit_leaf) {
        hit_open = true;
      } else if (cur_last > best_excl_t ||
                 (cur_last == best_excl_t && (best_excl_leaf == RTC_NO_LEAF || cur > best_excl_leaf))) {
        best_excl_t = cur_last;
        best_excl_leaf = cur;
        best_excl_mat = cur_mat;
      }
    }
    cur = RTC_NO_LEAF;
    cur_cnt = 0;
    cur_last = -kInf;
  }
  static constexpr bool kFrontOnly = false;
  static constexpr bool kBehindOnly = true;   // only entries with t < 0 (and the hit leaf's own) matter
  __device__ __forceinline__ double t_limit() const { return kInf; }
  __device__ __forceinline__ void entry(uint32_t l, uint32_t, uint32_t material, double et, double, double) {
    if (l != cur) {
      flush();
      cur = l;
      cur_mat = material;
    }
    if (et < 0.0) {
      cur_cnt++;
      cur_last = zmax(cur_last, et);
    } else if (l == hit_leaf && et == hit_t) {
      hit_dups++;
    }
  }
  __device__ __forceinline__ bool relevant(uint32_t l, uint32_t, double et) const {
    return et < 0.0 || (l == hit_leaf && et == hit_t);
  }
  __device__ __forceinline__ bool cullf(float tn, float) const { return tn > 1e-4f * (1.0f + __builtin_fabsf(tn)); }
  __device__ __forceinline__ float far_limit() const { return 0.0f; }
  __device__ __forceinline__ bool cull_limits(float tn, float, float) const { return tn > 1.0002e-4f; }  // tn > 1e-4 / (1 - 1e-4)
  __device__ __forceinline__ void box_limits(float& lo, float& hi) const { lo = -__builtin_inff(); hi = 1.0002e-4f; }
  __device__ __forceinline__ bool done() const { return false; }
  // (every root was tested by ONE lane of the group, so the entries of a leaf did arrive together; what is merged are the
  // lanes' flushed results: the latest open leaf, the latest one other than the hit leaf, the hit leaf's own state)
  __device__ __forceinline__ void merge_group(uint32_t group) {
    flush<true>();
    auto later = [](double at, uint32_t al, double bt, uint32_t bl) {  // is (bt, bl) the later open leaf?
      return bl != RTC_NO_LEAF && (al == RTC_NO_LEAF || bt > at || (bt == at && bl > al));
    };
    auto step = [&](auto tag) {
      constexpr int STEP = decltype(tag)::value;
      const double ot = group8_other<STEP>(best_t), oet = group8_other<STEP>(best_excl_t);
      const uint32_t ol = group8_other<STEP>(best_leaf), om = group8_other<STEP>(best_mat);
      const uint32_t oel = group8_other<STEP>(best_excl_leaf), oem = group8_other<STEP>(best_excl_mat);
      const uint32_t oopen = group8_other<STEP>(hit_open ? 1u : 0u), odups = group8_other<STEP>(hit_dups);
      if constexpr (SELECTS) {
        const bool take = later(best_t, best_leaf, ot, ol), take_excl = later(best_excl_t, best_excl_leaf, oet, oel);
        best_t = take ? ot : best_t;
        best_leaf = take ? ol : best_leaf;
        best_mat = take ? om : best_mat;
        best_excl_t = take_excl ? oet : best_excl_t;
        best_excl_leaf = take_excl ? oel : best_excl_leaf;
        best_excl_mat = take_excl ? oem : best_excl_mat;
      } else {
        if (later(best_t, best_leaf, ot, ol)) {
          best_t = ot;
          best_leaf = ol;
          best_mat = om;
        }
        if (later(best_excl_t, best_excl_leaf, oet, oel)) {
          best_excl_t = oet;
          best_excl_leaf = oel;
          best_excl_mat = oem;
        }
      }
      hit_open = hit_open || oopen != 0u;
      hit_dups += odups;
    };
    step(std::integral_constant<int, 0>{});
    step(std::integral_constant<int, 1>{});
    if (group > 4u) step(std::integral_constant<int, 2>{});
  }
};

// ------------------------------------------------------------------------------------------
// Patterns (patterns/pattern.zig:112-131).  Zig @mod for floats (LLVM backend): r = fmod(x,y);
// x < 0 ? fmod(r + y, y) : r.  With y == 2 fmod is exact: x - 2*trunc(x/2).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double fmod2(double x) { return x - 2.0 * __builtin_trunc(x / 2.0); }
__device__ __forceinline__ double zig_mod2(double x) {
  const double a = fmod2(x);
  return (x < 0.0) ? fmod2(a + 2.0) : a;
}

// the same for a divisor that is a power of two (1 and 2 in texture_map.zig): x / y, trunc and the product are exact
__device__ __forceinline__ double zig_mod(double x, double y) {
  const double a = x - y * __builtin_trunc(x / y);
  return (x < 0.0) ? (a + y) - y * __builtin_trunc((a + y) / y) : a;
}

struct Rgb {
  double r, g, b;
};

// noise.zig: Ken Perlin's improved noise (reference permutation noise.zig:6-23; the doubled table of
// noise.zig:25-33 is p[k & 255]).  Same statement as oracle/rtc_oracle.hpp perlinNoise / octaveNoise.
__constant__ uint8_t kPerlinPermutation[256] = {
    151, 160, 137, 91,  90,  15,  131, 13,  201, 95,  96,  53,  194, 233, 7,   225, 140, 36,  103, 30,  69,  142,
    8,   99,  37,  240, 21,  10,  23,  190, 6,   148, 247, 120, 234, 75,  0,   26,  197, 62,  94,  252, 219, 203,
    117, 35,  11,  32,  57,  177, 33,  88,  237, 149, 56,  87,  174, 20,  125, 136, 171, 168, 68,  175, 74,  165,
    71,  134, 139, 48,  27,  166, 77,  146, 158, 231, 83,  111, 229, 122, 60,  211, 133, 230, 220, 105, 92,  41,
    55,  46,  245, 40,  244, 102, 143, 54,  65,  25,  63,  161, 1,   216, 80,  73,  209, 76,  132, 187, 208, 89,
    18,  169, 200, 196, 135, 130, 116, 188, 159, 86,  164, 100, 109, 198, 173, 186, 3,   64,  52,  217, 226, 250,
    124, 123, 5,   202, 38,  147, 118, 126, 255, 82,  85,  212, 207, 206, 59,  227, 47,  16,  58,  17,  182, 189,
    28,  42,  223, 183, 170, 213, 119, 248, 152, 2,   44,  154, 163, 70,  221, 153, 101, 155, 167, 43,  172, 9,
    129, 22,  39,  253, 19,  98,  108, 110, 79,  113, 224, 232, 178, 185, 112, 104, 218, 246, 97,  228, 251, 34,
    242, 193, 238, 210, 144, 12,  191, 179, 162, 241, 81,  51,  145, 235, 249, 14,  239, 107, 49,  192, 214, 31,
    181, 199, 106, 157, 184, 84,  204, 176, 115, 121, 50,  45,  127, 4,   150, 254, 138, 236, 205, 93,  222, 114,
    67,  29,  24,  72,  243, 141, 128, 195, 78,  66,  215, 61,  156, 180};
__device__ __forceinline__ int perlin_p(int i) { return static_cast<int>(kPerlinPermutation[i & 255]); }
__device__ __forceinline__ double perlin_grad(int hash, double x, double y, double z) {  // noise.zig:90-96
  const int h = hash & 15;
  const double u = h < 8 ? x : y;
  const double v = h < 4 ? y : ((h == 12 || h == 14) ? x : z);
  return ((h & 1) == 0 ? u : -u) + ((h & 2) == 0 ? v : -v);
}
__device__ __forceinline__ double perlin_fade(double t) { return t * t * t * (t * (t * 6.0 - 15.0) + 10.0); }
__device__ __forceinline__ double perlin_lerp(double t, double a, double b) { return a + t * (b - a); }
__device__ __noinline__ double perlin_noise(double x, double y, double z) {  // noise.zig:51-89
  const double fx = __builtin_floor(x), fy = __builtin_floor(y), fz = __builtin_floor(z);
  const int X = static_cast<int>(static_cast<long long>(fx) & 255ll);
  const int Y = static_cast<int>(static_cast<long long>(fy) & 255ll);
  const int Z = static_cast<int>(static_cast<long long>(fz) & 255ll);
  x -= fx;
  y -= fy;
  z -= fz;
  const double u = perlin_fade(x), v = perlin_fade(y), w = perlin_fade(z);
  const int A = perlin_p(X) + Y, AA = perlin_p(A) + Z, AB = perlin_p(A + 1) + Z;
  const int B = perlin_p(X + 1) + Y, BA = perlin_p(B) + Z, BB = perlin_p(B + 1) + Z;
  return perlin_lerp(
      w,
      perlin_lerp(v, perlin_lerp(u, perlin_grad(perlin_p(AA), x, y, z), perlin_grad(perlin_p(BA), x - 1.0, y, z)),
                  perlin_lerp(u, perlin_grad(perlin_p(AB), x, y - 1.0, z), perlin_grad(perlin_p(BB), x - 1.0, y - 1.0, z))),
      perlin_lerp(v,
                  perlin_lerp(u, perlin_grad(perlin_p(AA + 1), x, y, z - 1.0), perlin_grad(perlin_p(BA + 1), x - 1.0, y, z - 1.0)),
                  perlin_lerp(u, perlin_grad(perlin_p(AB + 1), x, y - 1.0, z - 1.0),
                              perlin_grad(perlin_p(BB + 1), x - 1.0, y - 1.0, z - 1.0))));
}
__device__ __forceinline__ double octave_noise(double x, double y, double z, uint32_t octaves, double persistence) {
  double total = 0.0, frequency = 1.0, amplitude = 1.0, max_value = 0.0;  // noise.zig:35-49
  for (uint32_t i = 0; i < octaves; ++i) {
    total += perlin_noise(x * frequency, y * frequency, z * frequency) * amplitude;
    max_value += amplitude;
    amplitude *= persistence;
    frequency *= 2.0;
  }
  return total / max_value;
}
// RTC_BUMP_RIPPLES (rtc.h, rtc_scene_set_bumps): a parabolic wave of period 1 around the field's y axis, along the radial
// direction - + - * / sqrt floor fabs only, each correctly rounded, in the order the header writes them.
__device__ __forceinline__ void bump_ripples(double qx, double qz, double& dx, double& dz) {
  dx = 0.0;
  dz = 0.0;
  const double r = __builtin_sqrt(qx * qx + qz * qz);
  if (r == 0.0) return;
  const double v = 2.0 * (r - __builtin_floor(r)) - 1.0;
  const double h = (4.0 * v) * (1.0 - __builtin_fabs(v));
  dx = h * (qx / r);
  dz = h * (qz / r);
}

#ifdef RTC_MESHUV_TU
// RTC_TEX_MESH (rtc.h): what the pattern evaluation of the meshuv kernels knows of the hit - the
// texture table, the hit triangle's index in it (RTC_NO_LEAF: the hit leaf is no triangle, or the handle has no table: six
// zeros and (0, 0)) and the entry's barycentrics.  Constants of the whole evaluation, passed by value: three scalars and a
// pointer, never an array.  Compiled into the meshuv kernels' translation unit only - in every other unit the two macros
// are empty and the pattern functions have the arguments they had.
struct MeshUvHit {
  const double* rows;
  uint32_t tri;
  double u, v;
};
#define RTC_MESHUV_PARAM , const MeshUvHit mh
#define RTC_MESHUV_ARG , mh
#else
#define RTC_MESHUV_PARAM
#define RTC_MESHUV_ARG
#endif

// TextureMap.patternAt + UvPattern.uvPatternAt (texture_map.zig).  Returns the sub-pattern the uv pattern
// selects (align check, uv checkers), or RTC_NO_LEAF with the colour in `out` (uv test pattern, uv image).
// Out of line: scenes without texture maps never run it.
__device__ __noinline__ uint32_t texture_map_at(const DevScene& S, uint32_t tex, double px, double py, double pz, Rgb& out RTC_MESHUV_PARAM) {
  const DevTexMap tm = S.tex[tex];
  const double kPi = 3.14159265358979323846264338327950288;
  double u, v;
  uint32_t face = 0u;
  if (tm.mapping == 0u) {  // spherical, texture_map.zig:180-195
    const double theta = atan2(px, pz);
    const double radius = __builtin_sqrt((px * px + py * py) + pz * pz);
    const double phi = acos(py / radius);
    const double raw_u = theta / (2.0 * kPi);
    u = 1.0 - (raw_u + 0.5);
    v = 1.0 - phi / kPi;
  } else if (tm.mapping == 1u) {  // planar, :201-205
    u = zig_mod(px, 1.0);
    v = zig_mod(pz, 1.0);
  } else if (tm.mapping == 2u) {  // cylindrical, :210-217
    const double theta = atan2(px, pz);
    const double raw_u = theta / (2.0 * kPi);
    u = 1.0 - (raw_u + 0.5);
    v = zig_mod(py, 1.0);
#ifdef RTC_MESHUV_TU
  } else if (tm.mapping == 4u) {  // RTC_TEX_MESH (rtc.h): the hit triangle's texture row at the entry's barycentrics
    double a1 = 0.0, b1 = 0.0, a2 = 0.0, b2 = 0.0, a3 = 0.0, b3 = 0.0, bu = 0.0, bv = 0.0;
    if (mh.tri != RTC_NO_LEAF) {
      const double* __restrict__ R = mh.rows + static_cast<size_t>(RTC_MESHUV_ROW) * mh.tri;
      a1 = R[0]; b1 = R[1]; a2 = R[2]; b2 = R[3]; a3 = R[4]; b3 = R[5];
      bu = mh.u;
      bv = mh.v;
    }
    const double w = (1.0 - bu) - bv;
    u = (a2 * bu + a3 * bv) + a1 * w;
    v = (b2 * bu + b3 * bv) + b1 * w;
    if (u < 0.0 || u > 1.0) u = u - __builtin_floor(u);  // tiling; 0.0 and 1.0 stay
    if (v < 0.0 || v > 1.0) v = v - __builtin_floor(v);
#endif
  } else {  // cubic, :219-303; faces: front 0, back 1, left 2, right 3, up 4, down 5
    const double coord = zmax(__builtin_fabs(px), zmax(__builtin_fabs(py), __builtin_fabs(pz)));
    face = 1u;
    if (coord == px) face = 3u;
    else if (coord == -px) face = 2u;
    else if (coord == py) face = 4u;
    else if (coord == -py) face = 5u;
    else if (coord == pz) face = 0u;
    switch (face) {
      case 0u: u = zig_mod(px + 1.0, 2.0) / 2.0; v = zig_mod(py + 1.0, 2.0) / 2.0; break;
      case 1u: u = zig_mod(1.0 - px, 2.0) / 2.0; v = zig_mod(py + 1.0, 2.0) / 2.0; break;
      case 2u: u = zig_mod(pz + 1.0, 2.0) / 2.0; v = zig_mod(py + 1.0, 2.0) / 2.0; break;
      case 3u: u = zig_mod(1.0 - pz, 2.0) / 2.0; v = zig_mod(py + 1.0, 2.0) / 2.0; break;
      case 4u: u = zig_mod(px + 1.0, 2.0) / 2.0; v = zig_mod(1.0 - pz, 2.0) / 2.0; break;
      default: u = zig_mod(px + 1.0, 2.0) / 2.0; v = zig_mod(pz + 1.0, 2.0) / 2.0; break;
    }
  }
  const DevUv uv = S.uv[tm.uv[face]];
  if (uv.kind == 0u) {  // align check, :30-39
    uint32_t k = 0u;
    if (v > 0.8) {
      if (u < 0.2) k = 1u;
      else if (u > 0.8) k = 2u;
    } else if (v < 0.2) {
      if (u < 0.2) k = 3u;
      else if (u > 0.8) k = 4u;
    }
    return uv.sub[k];
  }
  if (uv.kind == 1u) {  // uv checkers, :52-60
    const double u_adj = __builtin_floor(u * uv.width), v_adj = __builtin_floor(v * uv.height);
    return (zig_mod(u_adj + v_adj, 2.0) < 1.0) ? uv.sub[0] : uv.sub[1];
  }
  if (uv.kind == 3u) {  // uv test pattern, :13-17
    out = {u, v, 0.0};
    return RTC_NO_LEAF;
  }
  // uv image, :74-103
  const DevImage im = S.img[uv.image];
  const float* __restrict__ rgb = S.img_rgb + 3ull * im.offset;
  auto pixel = [&](double fx, double fy) {  // Canvas.getPixelPointer(@intFromFloat(fx), @intFromFloat(fy)).?.*
    uint32_t x = fx <= 0.0 ? 0u : static_cast<uint32_t>(fx), y = fy <= 0.0 ? 0u : static_cast<uint32_t>(fy);
    x = min(x, im.width - 1u);  // outside the canvas the reference panics; clamped here
    y = min(y, im.height - 1u);
    const float* p = rgb + 3ull * (static_cast<size_t>(y) * im.width + x);
    return Rgb{static_cast<double>(p[0]), static_cast<double>(p[1]), static_cast<double>(p[2])};
  };
  const double v_flip = 1.0 - v;
  const double x = u * static_cast<double>(im.width - 1u);
  const double y = v_flip * static_cast<double>(im.height - 1u);
  if (uv.interp == 0u) {
    out = pixel(round(x), round(y));  // @round: half away from zero
    return RTC_NO_LEAF;
  }
  const double x1 = __builtin_floor(x), x2 = __builtin_ceil(x), y1 = __builtin_floor(y), y2 = __builtin_ceil(y);
  const Rgb c11 = pixel(x1, y1), c21 = pixel(x2, y1), c12 = pixel(x1, y2), c22 = pixel(x2, y2);
  const double wx1 = x2 - x, wx2 = x - x1, wy1 = y2 - y, wy2 = y - y1;  // both 0 on an integer coordinate (as there)
  const Rgb cx1{c11.r * wx1 + c21.r * wx2, c11.g * wx1 + c21.g * wx2, c11.b * wx1 + c21.b * wx2};
  const Rgb cx2{c12.r * wx1 + c22.r * wx2, c12.g * wx1 + c22.g * wx2, c12.b * wx1 + c22.b * wx2};
  out = {cx1.r * wy1 + cx2.r * wy2, cx1.g * wy1 + cx2.g * wy2, cx1.b * wy1 + cx2.b * wy2};
  return RTC_NO_LEAF;
}

// Follows a chain of "selecting" patterns (stripes / checkers / rings) down to a solid or
// test pattern.  Sub-patterns are evaluated at the OBJECT-space point with their own inverse
// (stripes.zig:27-33).  Returns false if the chain ends in a mixing pattern (idx then names it).
// A perturb on the way moves the object point, for everything below it: (ox, oy, oz) is in/out.
template <bool EXT>
__device__ __forceinline__ bool pattern_chain(const DevScene& S, const DevPattern* __restrict__ pat, uint32_t& idx,
                                              double& ox, double& oy, double& oz, Rgb& out RTC_MESHUV_PARAM) {
  for (int guard = 0; guard < 64; ++guard) {
    const DevPattern& P = pat[idx];
    const uint32_t kind = P.kind;
    if (kind == 0) {  // solid.zig:20-24
      out = {P.rgb[0], P.rgb[1], P.rgb[2]};
      return true;
    }
    const double* __restrict__ m = P.inv;
    const double px = row_pt(m + 0, ox, oy, oz);
    const double py = row_pt(m + 4, ox, oy, oz);
    const double pz = row_pt(m + 8, ox, oy, oz);
    const uint2 ab{P.a, P.b};
    if (kind == 9) {  // TestPattern, pattern.zig:144-148
      out = {px, py, pz};
      return true;
    } else if (kind == 1) {  // stripes.zig:27-33
      idx = (zig_mod2(px) < 1.0) ? ab.x : ab.y;
    } else if (kind == 5) {  // checkers.zig:23-29
      idx = (zig_mod2((__builtin_floor(px) + __builtin_floor(py)) + __builtin_floor(pz)) < 1.0) ? ab.x : ab.y;
    } else if (kind == 2) {  // rings.zig:27-33
      idx = (zig_mod2(__builtin_floor(__builtin_sqrt(px * px + pz * pz))) < 1.0) ? ab.x : ab.y;
    } else if (EXT && kind == 8) {  // texture_map.zig: (u, v) from the PATTERN point, then a uv pattern
      if constexpr (EXT) {          // (only the *_ext kernels carry this path)
        Rgb c;
        const uint32_t next = texture_map_at(S, P.a, px, py, pz, c RTC_MESHUV_ARG);
        if (next == RTC_NO_LEAF) {
          out = c;
          return true;
        }
        idx = next;  // align check / uv checkers select a sub-pattern, evaluated at the object point
      }
    } else if (kind == 7) {  // perturb.zig:31-46: the wrapped pattern is looked up at a jittered OBJECT point
      const uint32_t octaves = static_cast<uint32_t>(P.rgb[1]);
      const double persistence = P.rgb[2], scale = P.rgb[0];
      const double n0 = octave_noise(ox, oy, oz, octaves, persistence);
      const double n1 = octave_noise(ox, oy, oz + 1.0, octaves, persistence);
      const double n2 = octave_noise(ox, oy, oz + 2.0, octaves, persistence);
      ox = ox + n0 * scale;
      oy = oy + n1 * scale;
      oz = oz + n2 * scale;
      idx = ab.x;
    } else {
      return false;  // gradient / radial gradient / blend: needs both children
    }
  }
  out = {0.0, 0.0, 0.0};
  return true;
}

// Mixing patterns NESTED in one another (a blend of gradients, a gradient of a blend ...: gradient.zig:19-33 and
// blend.zig:16-27 take arbitrary `*const Pattern` children).  The reference recurses; here the tree of mixing patterns
// below `idx` is walked top-down with an explicit stack, each branch carrying its weight: a blend passes half of its
// weight to either child ((a + b) * 0.5: exact), a gradient 1 - f and f of it (a + (b - a) f), and the solid /
// test-pattern colours at the ends of the select-chains are summed by weight.  The sum differs from the reference's
// nested expression in the last bits (colours need 1e-5; no branch depends on them).  Out of line, *_ext kernels only:
// rtc_scene_create sends a scene with nested mixing patterns there and refuses more than RTC_PATTERN_STACK levels.
template <bool EXT>
__device__ __forceinline__ bool pattern_chain(const DevScene& S, const DevPattern* __restrict__ pat, uint32_t& idx,
                                              double& ox, double& oy, double& oz, Rgb& out RTC_MESHUV_PARAM);
__device__ __noinline__ Rgb pattern_tree(const DevScene& S, const DevPattern* pat, uint32_t idx, double ox, double oy, double oz RTC_MESHUV_PARAM) {
  struct Frame {
    double w, x, y, z;
    uint32_t idx;
  };
  Frame stack[RTC_PATTERN_STACK];
  int n = 0;
  Rgb acc{0.0, 0.0, 0.0};
  double w = 1.0;
  for (int guard = 0; guard < 4096; ++guard) {
    Rgb c;
    if (pattern_chain<true>(S, pat, idx, ox, oy, oz, c RTC_MESHUV_ARG)) {  // a select-chain that ends in a colour
      acc.r += w * c.r;
      acc.g += w * c.g;
      acc.b += w * c.b;
      if (n == 0) break;
      --n;
      idx = stack[n].idx;
      w = stack[n].w;
      ox = stack[n].x;
      oy = stack[n].y;
      oz = stack[n].z;
      continue;
    }
    const DevPattern& P = pat[idx];  // a mixing pattern, looked up at the (possibly perturbed) object point
    double wb = w * 0.5;             // blend.zig:21-24
    if (P.kind != 6u) {
      const double px = row_pt(P.inv + 0, ox, oy, oz), pz = row_pt(P.inv + 8, ox, oy, oz);
      double fpart = px - __builtin_floor(px);  // gradient.zig:27-32
      if (P.kind != 3u) {                       // radial gradient, gradient.zig:49-55
        const double mag = __builtin_sqrt(px * px + pz * pz);
        fpart = mag - __builtin_floor(mag);
      }
      wb = w * fpart;
    }
    if (n < RTC_PATTERN_STACK) {  // (deeper nestings are refused at create)
      stack[n].w = wb;
      stack[n].x = ox;
      stack[n].y = oy;
      stack[n].z = oz;
      stack[n].idx = P.b;
      ++n;
    }
    w = w - wb;
    idx = P.a;
  }
  return acc;
}

// Pattern.patternAt for the whole table.  Mixing patterns (gradient.zig, blend.zig) may sit anywhere in a select-chain;
// when their own children are select-chains - every scene of the reference - the mix is the reference's expression,
// evaluated here; a mixing pattern below a mixing pattern goes to pattern_tree (the *_ext kernels).
template <bool EXT>
__device__ __forceinline__ Rgb pattern_at(const DevScene& S, const DevPattern* __restrict__ pat, uint32_t idx, double ox,
                                          double oy, double oz RTC_MESHUV_PARAM) {
  Rgb out;
  if (pattern_chain<EXT>(S, pat, idx, ox, oy, oz, out RTC_MESHUV_ARG)) return out;
  const DevPattern& P = pat[idx];
  const uint32_t kind = P.kind;
  const double* __restrict__ m = P.inv;
  const double px = row_pt(m + 0, ox, oy, oz);
  const double pz = row_pt(m + 8, ox, oy, oz);
  uint32_t ia = P.a, ib = P.b;
  Rgb ca{0, 0, 0}, cb{0, 0, 0};
  {  // both children start from the mixing pattern's own object point (a perturb below moves its copy only)
    double ax = ox, ay = oy, az = oz, bx = ox, by = oy, bz = oz;
    const bool a_ends = pattern_chain<EXT>(S, pat, ia, ax, ay, az, ca RTC_MESHUV_ARG);
    const bool b_ends = pattern_chain<EXT>(S, pat, ib, bx, by, bz, cb RTC_MESHUV_ARG);
    if constexpr (EXT) {
      if (!(a_ends && b_ends)) return pattern_tree(S, pat, idx, ox, oy, oz RTC_MESHUV_ARG);  // nested mixing patterns
    }
  }
  if (kind == 6) {  // blend.zig:21-24
    return {(ca.r + cb.r) * 0.5, (ca.g + cb.g) * 0.5, (ca.b + cb.b) * 0.5};
  }
  double fpart;
  if (kind == 3) {  // gradient.zig:27-32
    fpart = px - __builtin_floor(px);
  } else {  // radial gradient, gradient.zig:49-55
    const double mag = __builtin_sqrt(px * px + pz * pz);
    fpart = mag - __builtin_floor(mag);
  }
  return {ca.r + (cb.r - ca.r) * fpart, ca.g + (cb.g - ca.g) * fpart, ca.b + (cb.b - ca.b) * fpart};
}

// (ENV) the environment unit evaluates patterns in a second place, at a missed ray's direction.
// pattern_at is forced inline: a second call would put a second copy of the select-chain and mix code into kernels that
// stand at 256 VGPRs.  The miss calls this out-of-line form instead; the hit keeps the inlined call every unit has (with
// the hit's lookup out of line too, through generic pointers where it reads LDS, every hit paid for it: cover + 6 %,
// teapot + 8 % on a handle without an environment).
#ifdef RTC_ENV_TU
__device__ __noinline__ Rgb pattern_at_shared(const DevScene& S, const DevPattern* pat, uint32_t idx, double ox, double oy,
                                              double oz RTC_MESHUV_PARAM) {
  return pattern_at<true>(S, pat, idx, ox, oy, oz RTC_MESHUV_ARG);
}
#endif

// std.math.pow(f64, x, y) as Zig's standard library computes it (lib/std/math/pow.zig, a port of Go's
// math.Pow; the reference calls it at material.zig:69 and world.zig:288): special cases, then
// x^y = x^frac(y) * x^int(y), the integer power by binary exponentiation on the frexp mantissa with the
// exponent carried separately, one scalbn at the end.  Same statement as oracle/rtc_oracle.hpp zig_pow.
// For the scenes' integer shininess this is a dozen multiplications instead of libm's pow().
__device__ __forceinline__ bool is_odd_integer(double v) {
  if (__builtin_fabs(v) >= 9007199254740992.0) return false;
  const double ip = __builtin_trunc(v);
  return v == ip && (static_cast<long long>(ip) & 1ll) == 1ll;
}
__device__ __forceinline__ double zig_pow(double x, double y) {
  const double inf = kInf;
  if (y == 0.0 || x == 1.0) return 1.0;
  if (x != x || y != y) return __builtin_nan("");
  if (y == 1.0) return x;
  if (x == 0.0) {
    if (y < 0.0) return is_odd_integer(y) ? __builtin_copysign(inf, x) : inf;
    return is_odd_integer(y) ? x : 0.0;
  }
  if (__builtin_isinf(y)) {
    if (x == -1.0) return 1.0;
    if ((__builtin_fabs(x) < 1.0) == (y > 0.0)) return 0.0;
    return inf;
  }
  if (__builtin_isinf(x)) {
    if (x < 0.0) {
      if (y < 0.0) return is_odd_integer(y) ? -0.0 : 0.0;
      return is_odd_integer(y) ? -inf : inf;
    }
    return y < 0.0 ? 0.0 : inf;
  }
  if (y == 0.5) return __builtin_sqrt(x);
  if (y == -0.5) return 1.0 / __builtin_sqrt(x);
  const double ay = __builtin_fabs(y);
  double yi = __builtin_trunc(ay);
  double yf = ay - yi;  // modf: exact
  if (yf != 0.0 && x < 0.0) return __builtin_nan("");
  if (yi >= 9223372036854775808.0) return exp(y * log(x));
  double a1 = 1.0;
  int ae = 0;
  if (yf != 0.0) {
    if (yf > 0.5) {
      yf -= 1.0;
      yi += 1.0;
    }
    a1 = exp(yf * log(x));
  }
  int xe;
  double x1 = frexp(x, &xe);
  for (long long i = static_cast<long long>(yi); i != 0; i >>= 1) {
    if (xe < -(1 << 12) || (1 << 12) < xe) {
      ae += xe;
      break;
    }
    if (i & 1ll) {
      a1 *= x1;
      ae += xe;
    }
    x1 *= x1;
    xe <<= 1;
    if (x1 < 0.5) {
      x1 += x1;
      xe -= 1;
    }
  }
  if (y < 0.0) {
    a1 = 1.0 / a1;
    ae = -ae;
  }
  return ldexp(a1, ae);
}

// zig_pow(x, n) for finite x > 0 and an integer 2 <= n <= 2^20: none of the special cases above applies and the
// fractional part is zero, so what is left of std.math.pow is the squaring loop on the frexp mantissa - the same
// operations in the same order, hence the same bits.  (Material.lighting's specular term, material.zig:69: the exponent
// is the material's shininess, an integer in every scene file; rtc_scene_create says so per material.  About a third
// of zig_pow's instructions on this path were tests for cases that cannot occur.)
__device__ __forceinline__ double pow_small_int(double x, uint32_t n) {
  double a1 = 1.0;
  int ae = 0;
  int xe;
  double x1 = frexp(x, &xe);
  for (uint32_t i = n; i != 0u; i >>= 1) {
    if (xe < -(1 << 12) || (1 << 12) < xe) {
      ae += xe;
      break;
    }
    if (i & 1u) {
      a1 *= x1;
      ae += xe;
    }
    x1 *= x1;
    xe <<= 1;
    if (x1 < 0.5) {
      x1 += x1;
      xe -= 1;
    }
  }
  return ldexp(a1, ae);
}

// One pending secondary ray of the colorAt recursion (world.zig:157-189): the colour it
// returns is multiplied by `weight` on its way up to the pixel.
struct Pending {
  Ray ray;
  double weight;
  uint32_t remaining;
#ifdef RTC_GLOSS_TU
  // (GLOSS) the ray's path code in its pixel's ray tree: the primary ray 1, the reflected child of c
  // 2 c, the refracted child 2 c + 1 (below 2^17: max_depth <= RTC_MAX_DEPTH).  In memory and in LDS it rides in the upper
  // half of the word that holds `remaining`: the record stays 64 bytes.  Compiled into the gloss kernels' unit only.
  uint32_t code;
#endif
#ifdef RTC_MEDIA_TU
  // (MEDIA) `weight` is the red channel's; the green and blue weights travel in a fifth 16-byte
  // quarter beside the record (render_body), and the ray's medium - a material index, or RTC_NO_MEDIUM - rides in the upper
  // half of the word that holds `remaining` (8 bits: at most RTC_MAX_DEPTH) and the path code (24 bits: below 2^17): every
  // 32-bit material index fits, and the record itself stays 64 bytes.  Compiled into the media kernels' unit only.
  double weight_g, weight_b;
  uint32_t medium;
#endif
#ifdef RTC_INDIR_TU
  // (INDIRECT) the ray's lineage: d, the diffuse bounces on it (bits 0-4: at most RTC_MAX_DEPTH), and
  // RTC_LIN_DIFFUSE where the ray itself was formed as a diffuse child.  It rides in the seven spare bits of the 24-bit code
  // field, above the path code's 17: the record and its fifth quarter stay.  Compiled into the indirect kernels' unit only.
  uint32_t lin;
#endif
#ifdef RTC_MIS_TU
  // (MIS) cos_b of a ray formed as a diffuse child: the cosine between its direction and the normal it
  // was drawn about.  The record's tail word is full and its fifth quarter holds two weights: while the ray waits the value
  // lies in DevMis::carry, a slot of memory per stack level - the levels in LDS included, whose LDS does not grow
  // (render_body's push_extra / load_extra).  Compiled into the MIS kernels' unit only.
  double cosb;
#endif
};
#ifdef RTC_INDIR_TU
static_assert(RTC_MAX_DEPTH < 32, "a Pending's lineage has five bits for its diffuse bounces");
static_assert(RTC_MAX_DEPTH + 1 <= 17, "the path code stays below 2^17: the lineage rides above it");
#define RTC_LIN_D 31u
#define RTC_LIN_DIFFUSE 32u
#define RTC_PENDING_TAIL(p)                                                                                           \
  (static_cast<unsigned long long>((p).remaining) | (static_cast<unsigned long long>((p).code | ((p).lin << 17)) << 8) | \
   (static_cast<unsigned long long>((p).medium) << 32))
#define RTC_PENDING_REMAINING(word) (static_cast<uint32_t>(word) & 0xFFu)
#define RTC_PENDING_CODE(p, word)                                                                                  \
  (p).code = (static_cast<uint32_t>(word) >> 8) & 0x1FFFFu, (p).lin = (static_cast<uint32_t>(word) >> 25) & 0x7Fu, \
  (p).medium = static_cast<uint32_t>((word) >> 32)
#define RTC_SET_CODE(p, c) (p).code = (c)
#define RTC_SET_LIN(p, v) (p).lin = (v)
// (the draws of a ray with d diffuse bounces on its lineage: key ^ (d * RTC_INDIRECT_DECORR); d == 0: the key itself)
#define RTC_DKEY(k) ((k) ^ (static_cast<unsigned long long>(cur.lin & RTC_LIN_D) * RTC_INDIRECT_DECORR))
#elif defined(RTC_MEDIA_TU)
static_assert(RTC_MAX_DEPTH < 256, "a Pending's `remaining` has eight bits beside the path code and the medium");
#define RTC_PENDING_TAIL(p) \
  (static_cast<unsigned long long>((p).remaining) | (static_cast<unsigned long long>((p).code) << 8) | (static_cast<unsigned long long>((p).medium) << 32))
#define RTC_PENDING_REMAINING(word) (static_cast<uint32_t>(word) & 0xFFu)
#define RTC_PENDING_CODE(p, word) (p).code = (static_cast<uint32_t>(word) >> 8), (p).medium = static_cast<uint32_t>((word) >> 32)
#define RTC_SET_CODE(p, c) (p).code = (c)
#elif defined(RTC_GLOSS_TU)
#define RTC_PENDING_TAIL(p) (static_cast<unsigned long long>((p).remaining) | (static_cast<unsigned long long>((p).code) << 32))
#define RTC_PENDING_REMAINING(word) static_cast<uint32_t>(word)
#define RTC_PENDING_CODE(p, word) (p).code = static_cast<uint32_t>((word) >> 32)
#define RTC_SET_CODE(p, c) (p).code = (c)
#else
#define RTC_PENDING_TAIL(p) (p).remaining
#define RTC_PENDING_REMAINING(word) static_cast<uint32_t>(word)
#define RTC_PENDING_CODE(p, word)
#define RTC_SET_CODE(p, c)
#endif
#ifndef RTC_INDIR_TU
#define RTC_SET_LIN(p, v) (void)0
#define RTC_DKEY(k) (k)
#endif
// (MEDIA) what the media unit adds where a ray is made, weighted or moved; nothing in every other unit
#ifdef RTC_MEDIA_TU
#define RTC_W(p, c) (p).weight_##c
#define RTC_MEDIA_START(p, w) (p).weight_g = (w), (p).weight_b = (w), (p).medium = RTC_NO_MEDIUM
#define RTC_MEDIA_KID(kid, parent, w, m) \
  (kid).weight_g = (parent).weight_g * (w), (kid).weight_b = (parent).weight_b * (w), (kid).medium = (m)
#define RTC_MEDIA_PUSH_EXTRA(level, p) push_extra(level, p)
#define RTC_MEDIA_LOAD_EXTRA(p, level, of_lane) load_extra(p, level, of_lane)
#else
#define RTC_W(p, c) (p).weight
#define RTC_MEDIA_START(p, w) (void)0
#define RTC_MEDIA_KID(kid, parent, w, m) (void)0
#define RTC_MEDIA_PUSH_EXTRA(level, p) (void)0
#define RTC_MEDIA_LOAD_EXTRA(p, level, of_lane) (void)0
#endif

// A Pending as it sits on a lane's stack in memory: one 64-byte line, moved as four 16-byte accesses.
typedef unsigned long long Quad2 __attribute__((ext_vector_type(2)));  // 16 bytes, moved as bits
__device__ __forceinline__ unsigned long long dbits(double x) { return __builtin_bit_cast(unsigned long long, x); }
__device__ __forceinline__ double bitsd(unsigned long long x) { return __builtin_bit_cast(double, x); }
__device__ __forceinline__ void store_pending(PendingRec* dst, const Pending& p) {
  Quad2* d = reinterpret_cast<Quad2*>(dst);
  Quad2 a, b, c, e;
  a.x = dbits(p.ray.ox); a.y = dbits(p.ray.oy);
  b.x = dbits(p.ray.oz); b.y = dbits(p.ray.dx);
  c.x = dbits(p.ray.dy); c.y = dbits(p.ray.dz);
  e.x = dbits(p.weight); e.y = RTC_PENDING_TAIL(p);
  d[0] = a; d[1] = b; d[2] = c; d[3] = e;
}
__device__ __forceinline__ Pending load_pending(const PendingRec* src) {
  const Quad2* d = reinterpret_cast<const Quad2*>(src);
  const Quad2 a = d[0], b = d[1], c = d[2], e = d[3];
  Pending p;
  p.ray = {bitsd(a.x), bitsd(a.y), bitsd(b.x), bitsd(b.y), bitsd(c.x), bitsd(c.y)};
  p.weight = bitsd(e.x);
  p.remaining = RTC_PENDING_REMAINING(e.y);
  RTC_PENDING_CODE(p, e.y);
  return p;
}

// The same record in LDS: the first levels of every lane's stack live there (render_body), four 16-byte quarters with
// the lanes of a wave side by side in each, so that a wave's push or pop is four conflict-free 16-byte accesses.
__device__ __forceinline__ void store_pending_lds(Quad2* dst, const Pending& p) {  // dst: quarter 0 of the lane's slot
  Quad2 a, b, c, e;
  a.x = dbits(p.ray.ox); a.y = dbits(p.ray.oy);
  b.x = dbits(p.ray.oz); b.y = dbits(p.ray.dx);
  c.x = dbits(p.ray.dy); c.y = dbits(p.ray.dz);
  e.x = dbits(p.weight); e.y = RTC_PENDING_TAIL(p);
  dst[0] = a; dst[64] = b; dst[128] = c; dst[192] = e;
}
__device__ __forceinline__ Pending load_pending_lds(const Quad2* src) {
  const Quad2 a = src[0], b = src[64], c = src[128], e = src[192];
  Pending p;
  p.ray = {bitsd(a.x), bitsd(a.y), bitsd(b.x), bitsd(b.y), bitsd(c.x), bitsd(c.y)};
  p.weight = bitsd(e.x);
  p.remaining = RTC_PENDING_REMAINING(e.y);
  RTC_PENDING_CODE(p, e.y);
  return p;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
  unsigned long long s = v;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// (MS) The whole image's pixel of a launch's output index: the rectangle, or the rank's tiles (DevPixelMap).
__device__ __forceinline__ void map_pixel(const DevPixelMap& map, size_t out_index, uint32_t& px, uint32_t& py) {
  if (map.mode == 0u) {
    const uint32_t ry = static_cast<uint32_t>(out_index / map.w);
    px = map.x0 + static_cast<uint32_t>(out_index - static_cast<size_t>(ry) * map.w);
    py = map.y0 + ry;
  } else {
    const size_t per_tile = static_cast<size_t>(map.tile_w) * map.tile_h;
    const uint32_t region = static_cast<uint32_t>(out_index / per_tile);
    const uint32_t r = static_cast<uint32_t>(out_index - static_cast<size_t>(region) * per_tile);
    const uint32_t ry = r / map.tile_w, rx = r - ry * map.tile_w;
    const uint32_t tile = map.mode == 1u ? map.first_tile + region * map.tile_stride : map.tile_list[region];
    const uint32_t ty = tile / map.tiles_x;
    px = (tile - ty * map.tiles_x) * map.tile_w + rx;
    py = ty * map.tile_h + ry;
  }
}

// (MS) The primary ray of camera sample k of pixel (px, py) - DESIGN.md section 12.  Sub-pixel offsets (i + jx) / grid,
// (j + jy) / grid; with grid 1 and no jitter this is Camera.rayForPixel (camera.zig:64-76) to the bit.  With an aperture
// the origin is a point of the lens disc (rejection sampling on the camera hash, no sin / cos) and the ray passes through
// the pixel's point on the focal plane.
__device__ __forceinline__ Ray camera_sample(const DevCamera& cam, const DevSampling& smp, uint32_t px, uint32_t py, uint32_t k) {
  const uint32_t j = k / smp.grid, i = k - j * smp.grid;
  const unsigned long long p = static_cast<unsigned long long>(py) * cam.hsize + px;
  const uint32_t g = smp.sample_base + k;  // the global sample index of the pass (section 13): the hash's, not the stratum's
  double jx = 0.5, jy = 0.5;
  if (smp.jitter) {
    jx = rtc_camera_jitter(smp.key, p, g, 0u);
    jy = rtc_camera_jitter(smp.key, p, g, 1u);
  }
  const double n = static_cast<double>(smp.grid);
  const double ox = (static_cast<double>(i) + jx) / n, oy = (static_cast<double>(j) + jy) / n;
  const double xoffset = (static_cast<double>(px) + ox) * cam.pixel_size;
  const double yoffset = (static_cast<double>(py) + oy) * cam.pixel_size;
  const double world_x = cam.half_width - xoffset;
  const double world_y = cam.half_height - yoffset;
  Ray r;
  double pix_x, pix_y, pix_z;
  if (smp.aperture > 0.0) {
    double lx = 0.0, ly = 0.0;
    for (uint32_t t = 0u; t < 32u; ++t) {
      const double a = 2.0 * rtc_camera_jitter(smp.key, p, g, 2u + 2u * t) - 1.0;
      const double b = 2.0 * rtc_camera_jitter(smp.key, p, g, 3u + 2u * t) - 1.0;
      if ((a * a) + (b * b) <= 1.0) {
        lx = a;
        ly = b;
        break;
      }
    }
    const double f = smp.focal, ax = smp.aperture * lx, ay = smp.aperture * ly;
    const double fx = world_x * f, fy = world_y * f;
    pix_x = row_pt(cam.inv + 0, fx, fy, -f);
    pix_y = row_pt(cam.inv + 4, fx, fy, -f);
    pix_z = row_pt(cam.inv + 8, fx, fy, -f);
    r.ox = row_pt(cam.inv + 0, ax, ay, 0.0);
    r.oy = row_pt(cam.inv + 4, ax, ay, 0.0);
    r.oz = row_pt(cam.inv + 8, ax, ay, 0.0);
  } else {
    pix_x = row_pt(cam.inv + 0, world_x, world_y, -1.0);
    pix_y = row_pt(cam.inv + 4, world_x, world_y, -1.0);
    pix_z = row_pt(cam.inv + 8, world_x, world_y, -1.0);
    r.ox = row_pt(cam.inv + 0, 0.0, 0.0, 0.0);
    r.oy = row_pt(cam.inv + 4, 0.0, 0.0, 0.0);
    r.oz = row_pt(cam.inv + 8, 0.0, 0.0, 0.0);
  }
  double dx = pix_x - r.ox, dy = pix_y - r.oy, dz = pix_z - r.oz;
  const double mag = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);  // Tuple.normalized, tuple.zig:109-116
  if (mag != 0.0) {
    dx = dx / mag;
    dy = dy / mag;
    dz = dz / mag;
  }
  r.dx = dx;
  r.dy = dy;
  r.dz = dz;
  return r;
}
#ifdef RTC_GLOSS_TU
// (GLOSS, rtc.h's rtc_scene_set_gloss) the direction d of a rough material's child ray, scattered:
// s is the first of RTC_GLOSS_DRAWS draws of the ray's own hash (h: its camera sample's, code: its path code) that lies in
// the unit ball - none: (0, 0, 0), the lens sampler's rule -, e = d + s * rough, d' = e / |e| (|e| == 0: d), and d' is
// taken when it lies on the child's side of the geometric normal ng (the reflection's above it, the refraction's below),
// else d stays.  Only + - * / sqrt and comparisons, each correctly rounded, in the order of rtc.h.  The draws are made one
// triple at a time and never kept.  Out of line, by value: a lane whose material is smooth never comes here, and the
// walk's registers are not the sampler's.  Compiled into the gloss kernels' translation unit only.
struct GlossDir {
  double x, y, z;
};
__device__ __noinline__ GlossDir gloss_scatter(unsigned long long h, uint32_t code, double rough, double dx, double dy, double dz,
                                               double ngx, double ngy, double ngz, bool below) {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (uint32_t t = 0u; t < RTC_GLOSS_DRAWS; ++t) {
    const double a = 2.0 * rtc_gloss_jitter(h, code, 3u * t + 0u) - 1.0;
    const double b = 2.0 * rtc_gloss_jitter(h, code, 3u * t + 1u) - 1.0;
    const double c = 2.0 * rtc_gloss_jitter(h, code, 3u * t + 2u) - 1.0;
    if (((a * a) + (b * b)) + (c * c) <= 1.0) {
      sx = a;
      sy = b;
      sz = c;
      break;
    }
  }
  const double ex = dx + sx * rough, ey = dy + sy * rough, ez = dz + sz * rough;
  const double m = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);  // tuple.zig's normalize
  GlossDir r{dx, dy, dz};
  if (m != 0.0) {
    const double ux = ex / m, uy = ey / m, uz = ez / m;
    const double side = (ux * ngx + uy * ngy) + uz * ngz;
    if (below ? side < 0.0 : side > 0.0) r = GlossDir{ux, uy, uz};
  }
  return r;
}
#endif
#ifdef RTC_OCCL_TU
// (OCCL, rtc.h's rtc_scene_set_occlusion) the direction of one occlusion sample at a hit with
// geometric normal ng: u is the first of RTC_GLOSS_DRAWS draws of the sample's own word (h: the camera sample's hash, word:
// (k << 17) | the hit ray's path code) inside the unit ball, normalised; e = ng + u, d = e / |e| - a cosine-weighted
// direction of ng's hemisphere; no draw accepted, a draw at the centre or |e| == 0: ng.  Only + - * / sqrt and comparisons,
// each correctly rounded, in the order of rtc.h.  The draws are made one triple at a time and never kept.  Out of line, by
// value, as gloss_scatter: the walk's registers are not the sampler's, and nothing of it is live across the trace that
// follows.  Compiled into the occlusion kernels' translation unit only.
__device__ __noinline__ GlossDir occl_direction(unsigned long long h, uint32_t word, double ngx, double ngy, double ngz) {
  GlossDir r{ngx, ngy, ngz};
  for (uint32_t t = 0u; t < RTC_GLOSS_DRAWS; ++t) {
    const double a = 2.0 * rtc_gloss_jitter(h, word, 3u * t + 0u) - 1.0;
    const double b = 2.0 * rtc_gloss_jitter(h, word, 3u * t + 1u) - 1.0;
    const double c = 2.0 * rtc_gloss_jitter(h, word, 3u * t + 2u) - 1.0;
    const double q = ((a * a) + (b * b)) + (c * c);
    if (q <= 1.0) {
      if (q != 0.0) {
        const double len = __builtin_sqrt(q);
        const double ex = ngx + a / len, ey = ngy + b / len, ez = ngz + c / len;
        const double m = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);  // tuple.zig's normalize
        if (m != 0.0) r = GlossDir{ex / m, ey / m, ez / m};
      }
      break;
    }
  }
  return r;
}
#define RTC_KA(mat) occl_ka
#else
#define RTC_KA(mat) (mat).ambient
#endif
// (SFILT, rtc.h's rtc_scene_set_shadow_filters) what a light's shadow ray yields.  In the shadow-filter
// kernels' translation unit: the walk is FilterVisitor's, a point or spot light's diffuse and specular terms are multiplied
// by the transmittance per channel, and an area light sums its samples' transmittances per channel, from 0.0 in the loop's
// order.  In every other unit the macros expand to what stood in their place: the any-hit walk, the terms as they are, the
// integer count.
#ifdef RTC_SFILT_TU
#define RTC_LIGHT_VISITOR FilterVisitor
#define RTC_LIGHT_VISITOR_SET(sv) (sv).filter = sfilt.row
#define RTC_LIGHT_BLOCKED(sv) (sv).done()
#define RTC_SF_DECL double sf_r = 1.0, sf_g = 1.0, sf_b = 1.0
#define RTC_SF_TAKE(sv) sf_r = (sv).tr, sf_g = (sv).tg, sf_b = (sv).tb
#define RTC_SF(x, c) ((x) * sf_##c)
#define RTC_LIT_DECL double lit_r = 0.0, lit_g = 0.0, lit_b = 0.0
#define RTC_LIT_ADD(sv) lit_r = lit_r + (sv).tr, lit_g = lit_g + (sv).tg, lit_b = lit_b + (sv).tb
#define RTC_LIT_INTENSITY(samples) const double intensity_r = lit_r / samples, intensity_g = lit_g / samples, intensity_b = lit_b / samples
#define RTC_INTENSITY(c) intensity_##c
#else
#define RTC_LIGHT_VISITOR ShadowVisitor
#define RTC_LIGHT_VISITOR_SET(sv) (void)0
#define RTC_LIGHT_BLOCKED(sv) (sv).shadowed
#define RTC_SF_DECL (void)0
#define RTC_SF_TAKE(sv) (void)0
#define RTC_SF(x, c) x
#define RTC_LIT_DECL uint32_t lit = 0u
#define RTC_LIT_ADD(sv) lit += (sv).shadowed ? 0u : 1u
#define RTC_LIT_INTENSITY(samples) const double intensity = static_cast<double>(lit) / samples
#define RTC_INTENSITY(c) intensity
#endif

// (MS) a lane's sample word: the sample index, and whether the lane owns the pixel (deals its samples, step 1)
#define RTC_SAMPLE_MASK 0xFFFFu
#define RTC_SAMPLE_OWNER 0x10000u

}  // namespace

// ------------------------------------------------------------------------------------------
// The megakernel: persistent waves.  The launch has only as many work-groups as the chip holds;
// every wave pulls 8x8-pixel chunks from one atomic counter and deals their pixels to whichever of
// its lanes have run out of rays, so a lane that finishes a cheap pixel (one plane hit) immediately
// starts another while its neighbours are still inside a glass sphere's ray tree.  Per iteration
// each lane handles ONE ray: closest-hit trace, shading with its shadow traces, spawn of the
// reflection / refraction children (one continues in registers, the other goes to the lane's stack).
// Exit: the counter runs past n_chunks (`drained`) and no lane holds a ray; every wave reaches it.
// ------------------------------------------------------------------------------------------
// (AREA: World.lights may hold area lights - DevAreaLights, the area kernels' extra argument; compiled into those kernels only)
// (MS: several camera samples per pixel - DevSampling, the sampling kernels' extra argument; compiled into those kernels only)
// (MOTION: top-level objects that move while the shutter is open - DevMotion, the motion kernels' extra argument; with MS
// and AREA, compiled into those kernels only)
// (SPOT: point lights that shine into a cone - DevSpots, the spot kernels' extra argument; with MOTION, MS and AREA,
// compiled into those kernels only)
// (BUMP: materials whose shading normal is perturbed - DevBumps, the bump kernels' extra argument; with SPOT, MOTION, MS
// and AREA, compiled into those kernels only)
// (TORUS: leaf kind 7, a quartic - leaf_entries' and the normal's case 7 and the solver, torus_quartic; with BUMP, SPOT,
// MOTION, MS and AREA, compiled into the torus kernels' translation unit only, under RTC_TORUS_TU: the device functions
// that are not templates - csg_collect - see the kind through the unit, not through a parameter)
// (MESHUV: texture maps of mapping RTC_TEX_MESH - DevMeshUvs, the meshuv kernels' extra argument; the hit's triangle and
// barycentrics reach the pattern evaluation, texture_map_at's mapping-4 branch reads the triangle's texture row.  With TORUS
// and everything below it, compiled into the meshuv kernels' translation unit only, under RTC_MESHUV_TU, which implies
// RTC_TORUS_TU: one family renders a world that holds tori and textured meshes)
// (GLOSS: rough materials whose reflected and refracted rays are scattered - DevGloss, the gloss kernels' extra argument;
// a Pending carries its ray's path code, the draws come from gloss_scatter.  With MESHUV and everything below it, compiled
// into the gloss kernels' translation unit only, under RTC_GLOSS_TU, which implies RTC_MESHUV_TU and RTC_TORUS_TU)
// (OCCL: ambient occlusion - DevOcclusion, the occlusion kernels' extra argument: a material with a radius has its ambient
// term scaled by the share of hemisphere rays that leave the hit unoccluded within that radius.  With GLOSS and everything
// below it, compiled into the occlusion kernels' translation unit only, under RTC_OCCL_TU, which implies RTC_GLOSS_TU)
// (SFILT: shadow filters - DevShadowFilter, the shadow-filter kernels' extra argument: a light's shadow ray multiplies the
// filter rows of the entries it crosses instead of stopping at the first.  With OCCL and everything below it, compiled into
// the shadow-filter kernels' translation unit only, under RTC_SFILT_TU, which implies RTC_OCCL_TU)
// (MEDIA: participating media - DevMedia, the media kernels' extra argument: every ray of the tree carries a medium and a
// weight per channel, and is attenuated along its segment (Beer-Lambert absorption in a material, a uniform fog outside).
// With SFILT and everything below it, compiled into the media kernels' translation unit only, under RTC_MEDIA_TU, which
// implies RTC_SFILT_TU)
// (ENV: an environment - DevEnvironment, the environment kernels' extra argument: a ray that misses adds the sky's colour at
// its direction, and every hit is lit by the suns, directional lights whose shadow rays have no far end, in a second loop
// after World.lights.  With MEDIA and everything below it, compiled into the environment kernels' translation unit only,
// under RTC_ENV_TU, which implies RTC_MEDIA_TU)
// (SKYL: a sky light - DevSkyLight, the sky-light kernels' extra argument: every hit of a material with a diffuse term gathers
// the sky through cosine-weighted hemisphere rays that are walked as a sun's shadow ray is, and the mean is added after the
// suns' loop.  With ENV and everything below it, compiled into the sky-light kernels' translation unit only, under
// RTC_SKYL_TU, which implies RTC_ENV_TU)
// (INDIRECT: indirect light - DevIndirect, the indirect kernels' extra argument: every hit adds its material's emission row, and
// a hit of a material with a diffuse term forms a third child, a cosine-weighted direction of the geometric normal's
// hemisphere by occl_direction, which the main loop traces like every other Pending.  With SKYL and everything below it,
// compiled into the indirect kernels' translation unit only, under RTC_INDIR_TU, which implies RTC_SKYL_TU)
// (EMIT: emitter sampling - DevEmitters, the emitter kernels' extra argument: a hit that forms a diffuse child also draws
// points on the listed emissive surfaces and walks a shadow ray to each, in further iterations of the suns' loop, and a ray
// formed as a diffuse child adds no emission at a listed leaf.  With INDIRECT and everything below it, compiled into the
// emitter kernels' translation unit only, under RTC_EMIT_TU, which implies RTC_INDIR_TU)
// (MIS: multiple importance sampling - DevMis, the MIS kernels' extra argument: with mode 1 an emitter sample is weighted by
// w_e and a ray formed as a diffuse child adds a listed leaf's emission times w_b, the balance heuristic's pair; the child
// carries cos_b.  With EMIT and everything below it, compiled into the MIS kernels' translation unit only, under
// RTC_MIS_TU, which implies RTC_EMIT_TU)
template <bool LDS, bool CSG, int WORLD = 0, int WAVES = 2, bool COOP = false, bool BOX = true, bool AREA = false, bool MS = false,
          bool MOTION = false, bool SPOT = false, bool BUMP = false, bool TORUS = false, bool MESHUV = false, bool GLOSS = false,
          bool OCCL = false, bool SFILT = false, bool MEDIA = false, bool ENV = false, bool SKYL = false, bool INDIRECT = false,
          bool EMIT = false, bool MIS = false>
__device__ __forceinline__ void render_body(const DevScene& S, const DevCamera& cam, const DevPixelMap& map,
                                            const uint32_t max_depth, double* __restrict__ out,
                                            DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                            const DevAreaLights& area = DevAreaLights{}, const DevSampling& smp = DevSampling{},
                                            const DevMotion& mo = DevMotion{}, const DevSpots& spots = DevSpots{},
                                            const DevBumps& bumps = DevBumps{}, const DevMeshUvs& muv = DevMeshUvs{},
                                            const DevGloss& gloss = DevGloss{}, const DevOcclusion& occl = DevOcclusion{},
                                            const DevShadowFilter& sfilt = DevShadowFilter{},
                                            const DevMedia& media = DevMedia{},
                                            const DevEnvironment& env = DevEnvironment{},
                                            const DevSkyLight& skyl = DevSkyLight{},
                                            const DevIndirect& indir = DevIndirect{},
                                            const DevEmitters& emit = DevEmitters{},
                                            const DevMis& mis = DevMis{}) {
  static_assert(!AREA || !COOP, "the area kernels run no cooperative iterations");
  static_assert(!MS || !COOP, "the sampling kernels run no cooperative iterations");
  static_assert(!MOTION || (MS && AREA && WORLD == 0), "the motion kernels are the general area-sampling walk");
  static_assert(!SPOT || MOTION, "the spot kernels are the motion walk");
  static_assert(!BUMP || SPOT, "the bump kernels are the spot walk");
  static_assert(!TORUS || BUMP, "the torus kernels are the bump walk");
#ifdef RTC_TORUS_TU
  static_assert(TORUS, "the torus translation unit compiles the torus kernels only: leaf kind 7 is compiled into every walk of it");
#else
  static_assert(!TORUS, "leaf kind 7 is compiled in the torus translation unit (rtc_torus.hip) only");
#endif
  static_assert(!MESHUV || TORUS, "the meshuv kernels are the torus walk");
#ifdef RTC_MESHUV_TU
  static_assert(MESHUV, "the meshuv translation unit compiles the meshuv kernels only: its pattern functions take the hit");
#else
  static_assert(!MESHUV, "mapping RTC_TEX_MESH is compiled in the meshuv translation unit (rtc_meshuv.hip) only");
  (void)muv;
#endif
  static_assert(!GLOSS || MESHUV, "the gloss kernels are the meshuv walk");
#ifdef RTC_GLOSS_TU
  static_assert(GLOSS, "the gloss translation unit compiles the gloss kernels only: its Pending carries the path code");
#else
  static_assert(!GLOSS, "rough materials are compiled in the gloss translation unit (rtc_gloss.hip) only");
  (void)gloss;
#endif
  static_assert(!OCCL || GLOSS, "the occlusion kernels are the gloss walk");
#ifdef RTC_OCCL_TU
  static_assert(OCCL, "the occlusion translation unit compiles the occlusion kernels only");
#else
  static_assert(!OCCL, "ambient occlusion is compiled in the occlusion translation unit (rtc_occlusion.hip) only");
  (void)occl;
#endif
  static_assert(!SFILT || OCCL, "the shadow-filter kernels are the occlusion walk");
#ifdef RTC_SFILT_TU
  static_assert(SFILT, "the shadow-filter translation unit compiles the shadow-filter kernels only");
#else
  static_assert(!SFILT, "shadow filters are compiled in the shadow-filter translation unit (rtc_shadowfilter.hip) only");
  (void)sfilt;
#endif
  static_assert(!MEDIA || SFILT, "the media kernels are the shadow-filter walk");
#ifdef RTC_MEDIA_TU
  static_assert(MEDIA, "the media translation unit compiles the media kernels only: its Pending carries a medium and three weights");
#else
  static_assert(!MEDIA, "participating media are compiled in the media translation unit (rtc_media.hip) only");
  (void)media;
#endif
  static_assert(!ENV || MEDIA, "the environment kernels are the media walk");
#ifdef RTC_ENV_TU
  static_assert(ENV, "the environment translation unit compiles the environment kernels only");
  static_assert(CSG, "the environment kernels evaluate every pattern kind");
#else
  static_assert(!ENV, "the environment is compiled in the environment translation unit (rtc_environment.hip) only");
  (void)env;
#endif
  static_assert(!SKYL || ENV, "the sky-light kernels are the environment walk");
#ifdef RTC_SKYL_TU
  static_assert(SKYL, "the sky-light translation unit compiles the sky-light kernels only");
#else
  static_assert(!SKYL, "the sky light is compiled in the sky-light translation unit (rtc_skylight.hip) only");
  (void)skyl;
#endif
  static_assert(!INDIRECT || SKYL, "the indirect kernels are the sky-light walk");
  static_assert(!INDIRECT || !COOP, "a cooperative iteration's Yield holds two children: a hit of the indirect kernels may form three");
#ifdef RTC_INDIR_TU
  static_assert(INDIRECT, "the indirect translation unit compiles the indirect kernels only: its Pending carries the lineage");
#else
  static_assert(!INDIRECT, "indirect light is compiled in the indirect translation unit (rtc_indirect.hip) only");
  (void)indir;
#endif
  static_assert(!EMIT || INDIRECT, "the emitter kernels are the indirect walk");
  static_assert(!EMIT || !COOP, "the emitter kernels run no cooperative iterations");
#ifdef RTC_EMIT_TU
  static_assert(EMIT, "the emitter translation unit compiles the emitter kernels only: its suns' loop walks with EmitVisitor");
#else
  static_assert(!EMIT, "emitter sampling is compiled in the emitter translation unit (rtc_emitters.hip) only");
  (void)emit;
#endif
  static_assert(!MIS || EMIT, "the MIS kernels are the emitter walk");
  static_assert(!MIS || !COOP, "the MIS kernels run no cooperative iterations");
#ifdef RTC_MIS_TU
  static_assert(MIS, "the MIS translation unit compiles the MIS kernels only: its Pending carries cos_b");
#else
  static_assert(!MIS, "multiple importance sampling is compiled in the MIS translation unit (rtc_mis.hip) only");
  (void)mis;
#endif
  RTC_PRIO_PHASE(RTC_PRIO_WORK);
#ifndef RTC_PROFILE
  if (blockIdx.x == 0u) {  // the next launch's counters (see DevStats)
    uint32_t* z = reinterpret_cast<uint32_t*>(next_stats);
    for (uint32_t i = threadIdx.x; i < sizeof(DevStats) / sizeof(uint32_t); i += blockDim.x) z[i] = 0u;
  }
#else
  (void)next_stats;
  if (threadIdx.x == 0u) rtc_prof_stats = stats;
#ifndef RTC_PROFILE_LITE
  for (uint32_t i = threadIdx.x; i < 4u * 58u; i += blockDim.x) rtc_prof_counts[i / 58u][i % 58u] = 0ull;
#endif
  __syncthreads();
#endif
  // Small-world tables (World.objects records + their FP32 bounds, materials, patterns, lights):
  // staged once per work-group into LDS, so neither the per-ray root loop nor the shading of a hit
  // chases pointers through memory.  Larger worlds run the same code on the tables in memory.
  // (WAVES: what the launch bounds leave room for per SIMD; a three-wave kernel has 53 KB of LDS per work-group: smaller
  // tables, RTC_LDS3_*, so that two levels of the pending-ray stacks still fit - one level in LDS instead of two is
  // 145 MB more memory traffic per cover frame)
  constexpr int N_ROOTS = WAVES == 3 ? RTC_LDS3_ROOTS : RTC_LDS_ROOTS, N_MATS = WAVES == 3 ? RTC_LDS3_MATERIALS : RTC_LDS_MATERIALS,
                N_PATS = WAVES == 3 ? RTC_LDS3_PATTERNS : RTC_LDS_PATTERNS;
  __shared__ RootRec lds_recs[LDS ? N_ROOTS : 1];
  __shared__ RootCullPair lds_cull[(LDS && !BOX) ? N_ROOTS / 2 : 1];  // phase 1 of the root loop: bounding spheres ...
  __shared__ RootBoxPair lds_box[(LDS && BOX) ? N_ROOTS / 2 : 1];     // ... or world boxes (trace())
  __shared__ DevMaterial lds_mat[LDS ? N_MATS : 1];
  __shared__ DevPattern lds_pat[LDS ? N_PATS : 1];
  constexpr int N_LIGHTS = WAVES == 3 ? RTC_LDS3_LIGHTS : RTC_LDS_LIGHTS;
  __shared__ double lds_light[LDS ? 6 * N_LIGHTS : 1];
  // per wave: which pending ray (donor lane, level of its stack) an idle lane takes over, and the canvas pixel it belongs to
  __shared__ uint4 lds_mail[4][64];
  // The first LDS_LEVELS levels of every lane's stack of pending rays ([wave][level][quarter][lane], see
  // store_pending_lds); deeper levels are in the buffer in memory (DevPixelMap::ray_stack).  A lane's stack is empty
  // again after almost every pixel, so nearly every push and pop stays here: the pops no longer wait for memory and the
  // 2048 resident waves no longer cycle 59 MB of stack lines through the L2s (142 MB written per cover frame).
  constexpr bool SIMPLE = WORLD == 2, FLAT = WORLD >= 1;
  // (specular_skip: the point-light branch of the five simple kernels; every other kernel keeps its instructions.  What was
  // counted and measured: profiles/specular_skip/)
  constexpr bool kSpecularSkip = SIMPLE && RTC_SPECULAR_SKIP;
  // (shared_normalize: the world normal, the point-light vector and the camera ray's direction of the simple kernels are
  // divided by their magnitude with one refined reciprocal - shared_normalize() - where the operands of every lane of the
  // wave that divides lie in shared_normalize_ok()'s range; otherwise the whole wave takes the plain divisions.  Decided
  // for the wave: a branch, not a select between two forms both computed.  Three of the five simple kernels keep it:
  // rtc_render_kernel_simple3 loses with it (fresnel + 3.2 %, six more spilled VGPRs) and rtc_render_kernel_simple_ext
  // gains nothing (skybox_demo, twelve more spilled VGPRs); they and every other kernel keep their instructions.
  // What was measured: profiles/normalize/)
  constexpr bool kSharedNormalize = SIMPLE && !CSG && (BOX || WAVES == 2) && RTC_SHARED_NORMALIZE;
  // (roots32: a three-wave simple kernel's world has at most RTC_LDS3_ROOTS = 32 roots, rtc_scene_create's simple3_ok: the
  // closest-hit and shadow traces of rtc_render_kernel_simple3_b run one block of the root loop with a 32-bit survivor
  // mask.  Not its containers pass - a ninth of cover's traces; with it the hit point went to scratch memory for the whole
  // shading block, 512 -> 679 MB written per cover frame, and two thirds of the gain with it - and not the kernel that culls
  // by spheres: fresnel + 2.8 %, reflection_and_refraction + 2.1 % with the 32-bit mask alone (six more spilled VGPRs).
  // Every other kernel keeps its instructions.  profiles/roots32/)
  constexpr int ROOTS = (SIMPLE && WAVES == 3 && BOX && RTC_ROOTS32) ? 32 : 64;
  // (own_root: rtc_scene_create marks a top-level sphere or cube of a simple world RTC_ROOT_ALONE when every other root's
  // refractive index is exactly 1 and no other root - box against box, box against plane - can be open around a point of
  // it.  For a hit on such a root the containers walk's n1 and n2 follow from that root's own two entries: every other
  // open leaf has ior 1, which is what "no open leaf" gives as well, and none can have its last negative entry later than
  // the hit root's.  In a wave whose transparent hits ALL lie on such roots the containers trace keeps of each lane's roots
  // the hit root alone - no ray set-up, no phase 1, no plane step, no other cube's step (trace(), OWN); one lane on any
  // other root and the whole wave makes the pass as before.  rtc_render_kernel_simple_b and _simple3_b, the simple kernels
  // that cull by boxes: rtc_render_kernel_simple3 lost with it on worlds that never take it (fresnel + 6.4 %,
  // reflection_and_refraction + 3.8 %: 126 spilled VGPRs for 118) and rtc_render_kernel_simple 1.7 % on fresnel; they,
  // rtc_render_kernel_simple_ext and every other kernel keep their instructions.  The argument and its limits: DESIGN.md
  // section 5; what was counted and measured, the form with a second copy of the tests among it: profiles/own_root/)
  constexpr bool kOwnRoot = SIMPLE && !CSG && BOX && RTC_CONTAINERS_OWN_ROOT;
  constexpr int LDS_LEVELS = (FLAT || !LDS) ? 2 : 1;  // (what fits beside the tables at WAVES work-groups per CU)
  __shared__ Quad2 lds_pend[4][LDS_LEVELS][4][64];
  // The colour a lane has accumulated for its pixel: touched once per iteration and when the pixel is finished, live
  // across the whole loop.  In LDS (one 24-byte slot per lane) it costs a read and a write per iteration instead of
  // six VGPRs of a kernel at the 256-register limit.
  __shared__ double lds_acc[4][64][3];
  // per lane: the top of the BVH walk's stack (the eight-wide walk's entries are pairs of words)
  // (the three-wave general kernel keeps two entries in LDS: the eight-wide walk's stack is as deep as the tree and
  // mostly one or two entries long)
  // (MEDIA: the general media kernel keeps two entries fewer in LDS - 4 096 bytes, what the fifth quarter of its pending
  // rays' one LDS level takes: two work-groups per CU stay resident)
  constexpr int TRAV = (WAVES == 3 && RTC_BVH8) ? 2 : ((MEDIA && LDS && !FLAT) ? RTC_LDS_TRAV - 2 : RTC_LDS_TRAV);
  __shared__ uint32_t lds_trav[FLAT ? 1 : 4][FLAT ? 1 : TRAV][RTC_BVH8 ? 128 : 64];
  const RootRec* __restrict__ recs = S.root_recs;
  CullTables cull{S.root_cull, S.root_box};
  const DevMaterial* __restrict__ mats = S.mat;
  const DevPattern* __restrict__ pats = S.pat;
  const double* __restrict__ lights = S.light;
  const double* __restrict__ area_rows = AREA ? area.row : nullptr;
#ifdef RTC_PROFILE
  uint32_t area_avail = AREA ? RTC_AREA_ROW * S.n_lights : 0u;  // (words of the area table a light's row may reach)
#endif
  if (LDS) {
    auto stage = [&](void* dst_, const void* src_, uint32_t n_words) {
      const double* __restrict__ src = reinterpret_cast<const double*>(src_);
      double* dst = reinterpret_cast<double*>(dst_);
      for (uint32_t i = threadIdx.x; i < n_words; i += blockDim.x) dst[i] = src[i];
    };
#ifndef RTC_PROFILE
    stage(lds_recs, S.root_recs, S.n_roots * (sizeof(RootRec) / 8u));
    if constexpr (BOX) stage(lds_box, S.root_box, ((S.n_roots + 7u) & ~7u) / 2u * (sizeof(RootBoxPair) / 8u));
    else stage(lds_cull, S.root_cull, ((S.n_roots + 3u) & ~3u) / 2u * (sizeof(RootCullPair) / 8u));
    stage(lds_mat, S.mat, S.n_materials * (sizeof(DevMaterial) / 8u));
    stage(lds_pat, S.pat, S.n_patterns * (sizeof(DevPattern) / 8u));
    stage(lds_light, S.light, S.n_lights * 6u);
#else
    // (the same copies, each held against its table's allocation and its array's length: a copy past either is counted
    // and cut short, and what the root loop and the shading may index is what was staged)
    auto words = [&](uint32_t n, size_t src_words, size_t dst_words) -> uint32_t {
      const uint32_t m = static_cast<uint32_t>(min(static_cast<size_t>(n), min(src_words, dst_words)));
      if (threadIdx.x == 0u) (void)RTC_IN_BOUNDS(RTC_OOB_STAGING, m == n);
      return m;
    };
    constexpr uint32_t W_REC = sizeof(RootRec) / 8u, W_CULL = sizeof(RootCullPair) / 8u, W_BOX = sizeof(RootBoxPair) / 8u,
                       W_MAT = sizeof(DevMaterial) / 8u, W_PAT = sizeof(DevPattern) / 8u;
    const uint32_t w_recs = words(S.n_roots * W_REC, static_cast<size_t>(S.n_root_recs) * W_REC, sizeof lds_recs / 8u);
    stage(lds_recs, S.root_recs, w_recs);
    uint32_t w_box = 0u, w_cull = 0u;
    if constexpr (BOX) {
      w_box = words(((S.n_roots + 7u) & ~7u) / 2u * W_BOX, static_cast<size_t>(S.n_root_box) * W_BOX, sizeof lds_box / 8u);
      stage(lds_box, S.root_box, w_box);
    } else {
      w_cull = words(((S.n_roots + 3u) & ~3u) / 2u * W_CULL, static_cast<size_t>(S.n_root_cull) * W_CULL, sizeof lds_cull / 8u);
      stage(lds_cull, S.root_cull, w_cull);
    }
    const uint32_t w_mat = words(S.n_materials * W_MAT, static_cast<size_t>(S.n_materials) * W_MAT, sizeof lds_mat / 8u);
    stage(lds_mat, S.mat, w_mat);
    const uint32_t w_pat = words(S.n_patterns * W_PAT, static_cast<size_t>(S.n_patterns) * W_PAT, sizeof lds_pat / 8u);
    stage(lds_pat, S.pat, w_pat);
    const uint32_t w_light = words(S.n_lights * 6u, static_cast<size_t>(S.n_lights) * 6u, sizeof lds_light / 8u);
    stage(lds_light, S.light, w_light);
    if (threadIdx.x == 0u) {
      rtc_oob_avail[0] = w_recs / W_REC;
      rtc_oob_avail[1] = w_cull / W_CULL;
      rtc_oob_avail[2] = w_box / W_BOX;
      rtc_oob_avail[3] = w_mat / W_MAT;
      rtc_oob_avail[4] = w_pat / W_PAT;
      rtc_oob_avail[5] = w_light;
    }
#endif
    if constexpr (AREA) {  // (the area rows beside the point table; tablesInLds counts them with the lights)
      __shared__ double lds_area[RTC_AREA_ROW * N_LIGHTS];
#ifndef RTC_PROFILE
      stage(lds_area, area.row, S.n_lights * RTC_AREA_ROW);
#else
      const uint32_t w_area = words(S.n_lights * RTC_AREA_ROW, static_cast<size_t>(S.n_lights) * RTC_AREA_ROW, sizeof lds_area / 8u);
      stage(lds_area, area.row, w_area);
      area_avail = w_area;
#endif
      area_rows = lds_area;
    }
    __syncthreads();
    recs = lds_recs;
    cull.sphere = lds_cull;
    cull.box = lds_box;
    mats = lds_mat;
    pats = lds_pat;
    lights = lds_light;
  }
#ifdef RTC_PROFILE
  if (!LDS) {  // (the tables in memory, as allocated)
    if (threadIdx.x == 0u) {
      rtc_oob_avail[0] = S.n_root_recs;
      rtc_oob_avail[1] = S.n_root_cull;
      rtc_oob_avail[2] = S.n_root_box;
      rtc_oob_avail[3] = S.n_materials;
      rtc_oob_avail[4] = S.n_patterns;
      rtc_oob_avail[5] = 6u * S.n_lights;
    }
    __syncthreads();
  }
  // the launch's output: the rectangle, or the rank's tiles
  const size_t out_extent = map.mode == 0u ? static_cast<size_t>(map.w) * map.h : static_cast<size_t>(map.n_my_tiles) * map.tile_w * map.tile_h;
  const bool stack_ok = (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) < map.ray_stack_waves;
#endif
  const uint32_t lane = threadIdx.x & 63u;
  // (bits of a ballot below this lane, by mask and popcount.  v_mbcnt_lo / v_mbcnt_hi would do it in two instructions and
  // without the mask's two registers - and the three-wave kernel's register allocation comes out worse for it: 117
  // instead of 102 spilled VGPRs, 648 instead of 283 MB written per cover frame, 0.571 instead of 0.553 ms.)
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  auto bits_below = [&](unsigned long long m) -> uint32_t { return static_cast<uint32_t>(__builtin_popcountll(m & lanes_below)); };

  // wave-uniform cursor: the packet the wave pulled last (lane i < 16 holds its item i), the item that is
  // open, and the run of pixels of one 8x8 chunk that item names
  uint32_t items = RTC_NO_ITEM, item_next = RTC_PACKET_ITEMS;
  // schedule feedback: how long the wave took for the packet it holds (meaningful because a wave finishes one
  // packet before it pulls the next)
  uint32_t pk_cur = RTC_NO_ITEM;
  unsigned long long pk_t0 = 0ull;
  // (one scalar load per wave; uniform)
  const uint32_t n_units = map.n_units_dev != nullptr ? __builtin_amdgcn_readfirstlane(*map.n_units_dev) : map.n_units;
  uint32_t chunk_pos = 64u, chunk_end = 64u;
  uint32_t chunk_rx0 = 0u, chunk_ry0 = 0u, chunk_px0 = 0u, chunk_py0 = 0u, chunk_w = 0u, chunk_h = 0u;
  size_t chunk_out0 = 0;
  bool drained = false;
  bool first_pull = true;

  // per-lane pixel and ray state
  bool has_pixel = false, have_cur = false;
  bool shared = false;  // part of this pixel's ray tree runs (or ran) in another lane
  size_t out_index = 0;
  // cost feedback: traces this lane spent on its share of the pixel (closest-hit 2, containers 2, shadow 1 each:
  // roughly their shares of an iteration's time; a pixel behind glass costs several times a pixel on a wall per ray)
  uint32_t share_rays = 0u;
  double* const acc = lds_acc[threadIdx.x >> 6][threadIdx.x & 63u];
  uint32_t* const trav_stack = FLAT ? nullptr : &lds_trav[threadIdx.x >> 6][0][(RTC_BVH8 ? 2u : 1u) * (threadIdx.x & 63u)];
  acc[0] = acc[1] = acc[2] = 0.0;
  // (MS) the lane's sample word (RTC_SAMPLE_*): which camera sample of its pixel the lane's rays belong to.  A lane that
  // took over part of another lane's ray tree (step 2a) adds its share and is done; only the owner starts the pixel's next
  // sample.  In LDS, 4 bytes a lane: the area kernel's two work-groups per CU leave 1 872 B per work-group beside its tables.
  uint32_t* samp_word = nullptr;
  if constexpr (MS) {
    __shared__ uint32_t lds_sample[4][64];
    samp_word = &lds_sample[threadIdx.x >> 6][threadIdx.x & 63u];
  }
  unsigned n_primary = 0, n_secondary = 0, n_shadow_calls = 0, n_shadow_traced = 0, overflow = 0, n_stolen = 0;
  Pending cur;
  cur.ray = {0, 0, 0, 0, 0, 0};
  cur.weight = 0.0;
  cur.remaining = 0u;
  RTC_SET_CODE(cur, 0u);
  RTC_SET_LIN(cur, 0u);
  RTC_MEDIA_START(cur, 0.0);
#ifdef RTC_MIS_TU
  cur.cosb = 0.0;
#endif
  // The lane's pending refraction siblings: a deque.  The lane itself pops the newest entry (depth
  // first); an idle neighbour may take the OLDEST one (the largest sub-tree) through the mailbox.
  // It lives in a buffer of its own rather than in scratch: scratch interleaves the lanes dword by dword,
  // so ONE lane pushing one 64-byte entry touches 16 different cache lines; here a lane's entry is one
  // 64-byte line and a whole wave's push is 4 KB contiguous.  Layout [wave][level][lane].
  PendingRec* const stack = map.ray_stack +
      (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) * map.ray_stack_levels * 64u + lane;
  const int stack_cap = static_cast<int>(map.ray_stack_levels);
  int sp = 0, base = 0;
  uint4* const mailbox = lds_mail[threadIdx.x >> 6];
  Quad2* const pend_wave = &lds_pend[threadIdx.x >> 6][0][0][0];  // level l of lane x: pend_wave + l * 256 + x
  // (the buffer in memory keeps a slot for every level; the first LDS_LEVELS of them are never touched)
  auto push_level = [&](int level, const Pending& p) {
    if (level < LDS_LEVELS) {
      store_pending_lds(pend_wave + level * 256 + lane, p);
    } else {
#ifdef RTC_PROFILE
      if (!RTC_IN_BOUNDS(RTC_OOB_PENDING, stack_ok && static_cast<uint32_t>(level) < map.ray_stack_levels)) return;
#endif
      store_pending(stack + static_cast<size_t>(level) * 64u, p);
    }
  };
  auto load_level = [&](int level, uint32_t of_lane) -> Pending {
    if (level < LDS_LEVELS) return load_pending_lds(pend_wave + level * 256 + of_lane);
#ifdef RTC_PROFILE
    if (!RTC_IN_BOUNDS(RTC_OOB_PENDING, stack_ok && static_cast<uint32_t>(level) < map.ray_stack_levels && of_lane < 64u)) return Pending{};
#endif
    return load_pending(stack + static_cast<size_t>(level) * 64u - lane + of_lane);
  };
#ifdef RTC_MEDIA_TU
  // (MEDIA) the fifth quarter of every record - the green and blue weights - beside the four: for the levels in LDS in an
  // array of its own ([wave][level][lane]), for the levels in memory in DevMedia::stack_ext, laid out and sized as
  // DevPixelMap::ray_stack is ([wave][level][lane], 16 bytes a slot).  It moves wherever the record moves: push, pop, and
  // the read of a neighbour's oldest level.
  __shared__ Quad2 lds_pend_x[4][LDS_LEVELS][64];
  Quad2* const pend_x_wave = &lds_pend_x[threadIdx.x >> 6][0][0];
  Quad2* const stack_x = static_cast<Quad2*>(media.stack_ext) +
      (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) * map.ray_stack_levels * 64u + lane;
#ifdef RTC_MIS_TU
  // (MIS) cos_b of a waiting diffuse child: DevMis::carry, laid out as DevPixelMap::ray_stack is, 8 bytes a slot, in memory
  // for every level - a sixth quarter in LDS would take the LDS form's second work-group per CU.
  // Written and read only for a ray that carries RTC_LIN_DIFFUSE, with mode 1 (wave-uniform).
  double* const carry = mis.carry + (static_cast<size_t>(blockIdx.x) * 4u + (threadIdx.x >> 6)) * map.ray_stack_levels * 64u + lane;
#endif
  auto push_extra = [&](int level, const Pending& p) {
    Quad2 x;
    x.x = dbits(p.weight_g); x.y = dbits(p.weight_b);
#ifdef RTC_MIS_TU
    if constexpr (MIS) {
      if (mis.mode != 0u && (p.lin & RTC_LIN_DIFFUSE) != 0u &&
          RTC_IN_BOUNDS(RTC_OOB_PENDING, stack_ok && static_cast<uint32_t>(level) < map.ray_stack_levels))
        carry[static_cast<size_t>(level) * 64u] = p.cosb;
    }
#endif
    if (level < LDS_LEVELS) {
      pend_x_wave[level * 64 + lane] = x;
    } else {
#ifdef RTC_PROFILE
      if (!RTC_IN_BOUNDS(RTC_OOB_PENDING, stack_ok && static_cast<uint32_t>(level) < map.ray_stack_levels)) return;
#endif
      stack_x[static_cast<size_t>(level) * 64u] = x;
    }
  };
  auto load_extra = [&](Pending& p, int level, uint32_t of_lane) {
    Quad2 x;
    if (level < LDS_LEVELS) {
      x = pend_x_wave[level * 64 + of_lane];
    } else {
#ifdef RTC_PROFILE
      if (!RTC_IN_BOUNDS(RTC_OOB_PENDING, stack_ok && static_cast<uint32_t>(level) < map.ray_stack_levels && of_lane < 64u)) return;
#endif
      x = (stack_x + static_cast<size_t>(level) * 64u - lane)[of_lane];
    }
    p.weight_g = bitsd(x.x);
    p.weight_b = bitsd(x.y);
#ifdef RTC_MIS_TU
    if constexpr (MIS) {  // (after load_level: the lineage says whether the slot holds a value)
      p.cosb = 0.0;
      if (mis.mode != 0u && (p.lin & RTC_LIN_DIFFUSE) != 0u &&
          RTC_IN_BOUNDS(RTC_OOB_PENDING, stack_ok && static_cast<uint32_t>(level) < map.ray_stack_levels && of_lane < 64u))
        p.cosb = (carry + static_cast<size_t>(level) * 64u - lane)[of_lane];
    }
#endif
  };
#endif

#ifdef RTC_PROFILE
  unsigned long long prof_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long prof_t = __builtin_amdgcn_s_memtime();
  const unsigned long long prof_start = prof_t;
  unsigned prof_sec = 0;
  unsigned long long prof_iters = 0, prof_units = 0;
  unsigned long long prof2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long prof_snap[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // prof_acc at the wave's last packet fetch
  unsigned long long prof3[21] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned prof_last_unit = 0, prof_first_unit = 0;
  const unsigned long long prof_real0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long prof_real_fetch = prof_real0;
#endif
  for (;;) {
    RTC_STAMP(0);
    RTC_PRIO_PHASE(RTC_PRIO_DEAL);
    bool next_sample = false;  // (MS) the lane's pixel goes on with its next camera sample (its ray: step 2b)
    // ---- 1. a lane without a ray pops its stack; an empty stack means its share of the pixel is done.
    // Shares of one pixel may finish in several lanes (step 2a): those are ADDED to the pixel, which the
    // first hand-out zeroed; a pixel whose whole ray tree stayed in one lane (most of them) is stored once.
    if (!have_cur) {
      if (sp > base) {
        cur = load_level(--sp, lane);
        RTC_MEDIA_LOAD_EXTRA(cur, sp, lane);
        have_cur = true;
      } else {
        sp = base = 0;
        if constexpr (MS) {  // the pixel is written once, after its last sample
          if (has_pixel) {
            const uint32_t w = *samp_word;
            if ((w & RTC_SAMPLE_OWNER) != 0u && (w & RTC_SAMPLE_MASK) + 1u < smp.samples) {
              *samp_word = w + 1u;
              next_sample = true;
            }
          }
        }
        if (!next_sample && has_pixel && RTC_IN_BOUNDS(RTC_OOB_CANVAS, out_index < out_extent)) {
          double* __restrict__ o = out + 3 * out_index;  // Canvas pixel, canvas.zig:132-137
          const double acc_r = acc[0], acc_g = acc[1], acc_b = acc[2];
          if (!shared) {  // the whole ray tree ran in this lane: the pixel is written exactly once
            // 24 B at an 8-byte-aligned address: one 16-byte and one 8-byte store (gfx950 takes unaligned
            // vector accesses) instead of three separate write requests
            typedef double Double2 __attribute__((ext_vector_type(2), aligned(8)));
            Double2 rg;
            rg.x = acc_r;
            rg.y = acc_g;
            // streaming stores: a finished pixel is not read again, and the canvas (50 MB at 1080p) must not push the
            // BVH nodes and triangles of a mesh scene out of the 4 MB L2s
            __builtin_nontemporal_store(rg, reinterpret_cast<Double2*>(o));
            __builtin_nontemporal_store(acc_b, o + 2);
          } else
          {
            atomicAdd(o + 0, acc_r);
            atomicAdd(o + 1, acc_g);
            atomicAdd(o + 2, acc_b);
          }
          if (map.cost != nullptr) {  // rays this pixel took: next frame's schedule is packed by it
            if (!shared) {
              map.cost[out_index] = share_rays;
            } else {
              atomicAdd(map.cost + out_index, share_rays);
            }
          }
          share_rays = 0u;
          has_pixel = false;
        }
#ifdef RTC_PROFILE
        else if (has_pixel && !next_sample) {  // (a pixel outside the output: counted above, not written)
          share_rays = 0u;
          has_pixel = false;
        }
#endif
      }
    }
    RTC_STAMP(8);
    // ---- 2a. work sharing inside the wave: an idle lane takes the oldest pending ray (the root of the
    // largest unexplored sub-tree) of a busy lane.  Without this a pixel whose ray tree has 2^(depth+1)-1
    // nodes occupies ONE lane for that many iterations.
    {
      const bool idle = !have_cur && !next_sample;
      const bool donor = have_cur && sp > base;
      const unsigned long long imask = __ballot(idle), dmask = __ballot(donor);
      if (imask != 0ull && dmask != 0ull) {
        const uint32_t pairs = min(static_cast<uint32_t>(__builtin_popcountll(imask)),
                                   static_cast<uint32_t>(__builtin_popcountll(dmask)));
        const uint32_t irank = bits_below(imask);
        const uint32_t drank = bits_below(dmask);
        if (donor && drank < pairs) {
          // (MS: the donor's sample index rides above the lane number)
          mailbox[drank] = uint4{MS ? lane | (*samp_word & RTC_SAMPLE_MASK) << 8 : lane, static_cast<uint32_t>(base++), static_cast<uint32_t>(out_index), static_cast<uint32_t>(out_index >> 32)};
          if (!shared && RTC_IN_BOUNDS(RTC_OOB_CANVAS, out_index < out_extent)) {
            // First hand-out of this pixel: from here on its shares are ADDED, so it starts from zero.  The canvas is
            // not cleared per launch (a pixel nobody shares is stored once); the store is at L2 before the taker —
            // a lane of this wave — can issue its first atomic.
            double* __restrict__ o = out + 3 * out_index;
            o[0] = 0.0;
            o[1] = 0.0;
            o[2] = 0.0;
            if (map.cost != nullptr) map.cost[out_index] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          }
          shared = true;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (idle && irank < pairs) {
          // (the donor's slot is read here, in program order before any lane of the wave can push into it again)
          const uint4 m = mailbox[irank];
          cur = load_level(static_cast<int>(m.y), MS ? m.x & 63u : m.x);
          RTC_MEDIA_LOAD_EXTRA(cur, static_cast<int>(m.y), MS ? m.x & 63u : m.x);
          if constexpr (MS) *samp_word = m.x >> 8;  // (the sample's index; not the owner)
          out_index = static_cast<size_t>(m.z) | (static_cast<size_t>(m.w) << 32);
          have_cur = true;
          has_pixel = true;
          shared = true;
          acc[0] = acc[1] = acc[2] = 0.0;
          n_stolen++;
        }
        if (sp == base) sp = base = 0;  // a donor whose stack is empty again starts over at level 0 (in LDS)
      }
    }
    RTC_STAMP(9);
    // ---- 2b. deal new pixels to the lanes that still want one
    bool want = !have_cur && !next_sample, got_pixel = false;
    uint32_t new_px = 0u, new_py = 0u;
    unsigned long long wmask = __ballot(want);
    while (wmask) {
      if (chunk_pos >= chunk_end) {
        uint32_t unit = RTC_NO_ITEM;
        if (item_next < RTC_PACKET_ITEMS) unit = __builtin_amdgcn_readlane(items, item_next);
        RTC_STAMP(9);  // (diagnostic builds: section 15 ends when the items of a fresh packet have arrived)
        if (unit == RTC_NO_ITEM) {  // the packet is used up: pull the next one
          if (drained) break;
          // A wave owns every pixel of a packet it pulls.  Pulling one for a couple of idle lanes would commit the
          // wave to a whole packet more than its neighbours (when a frame is split over GPUs a wave's fair share is
          // one or two packets): those lanes wait, or take over a sub-tree (step 2a), until enough of them are free.
          if (static_cast<uint32_t>(__builtin_popcountll(wmask)) < map.pull_min_idle && __any(have_cur || got_pixel)) break;
          if (map.packet_time != nullptr && pk_cur != RTC_NO_ITEM) {  // the packet this wave just finished took ...
            if (lane == 0u) map.packet_time[pk_cur] = static_cast<uint32_t>((__builtin_amdgcn_s_memtime() - pk_t0) >> 4);
            pk_cur = RTC_NO_ITEM;
          }
          uint32_t c = 0u;
          RTC_STAMP(14);  // (diagnostic builds: section 14 = the round trip of the work counter)
          // A wave's FIRST packet is the one with its own number; the counter hands out the packets after those.  (At
          // the start of a launch every wave pulls at once, and atomics on one cache line are served one after the
          // other: the last of 3072 waves got its first packet 25 us into the frame.  fresnel 300x300 0.129 -> 0.105 ms,
          // cover 1080p 0.579 -> 0.554, teapot 0.310 -> 0.293.  The four waves of a work-group start on four
          // neighbouring packets.)
          if (first_pull) {
            first_pull = false;
            c = blockIdx.x * 4u + (threadIdx.x >> 6);
          } else if (lane == 0u) {
            c = atomicAdd(&stats->next_chunk, 1u) + gridDim.x * 4u;
          }
          c = __builtin_amdgcn_readfirstlane(c);
          RTC_STAMP(15);
          if (c >= n_units) {
            drained = true;
            break;
          }
#ifdef RTC_PROFILE
          prof_last_unit = c;
          prof_first_unit = static_cast<unsigned>((__builtin_amdgcn_s_memtime() - prof_start) >> 8);  // time of the last fetch
          prof_units += 1ull;
          prof_real_fetch = __builtin_amdgcn_s_memrealtime();
          for (int i = 0; i < 16; ++i) prof_snap[i] = prof_acc[i];
          prof_snap[7] = prof_iters;
#endif
          pk_cur = c;
          pk_t0 = __builtin_amdgcn_s_memtime();
          if (map.order != nullptr) {
            items = lane < RTC_PACKET_ITEMS ? map.order[static_cast<size_t>(c) * RTC_PACKET_ITEMS + lane] : RTC_NO_ITEM;
          } else {  // unscheduled: packet c is chunk c, whole - or, in a launch of a handful of chunks, one row of a chunk
            items = lane == 0u ? c : RTC_NO_ITEM;
          }
          item_next = 0u;
          continue;
        }
        item_next++;
        // an item: pixels [start, start + len) of chunk c, in the chunk's row-major 8x8 numbering
        // (a launch too small to be scheduled - fewer chunks than a schedule is made for - hands out ROWS of chunks: eight
        // packets per chunk on eight waves, each of which then works cooperatively where the kernel can (render_body, COOP);
        // whole, a chunk of glass pixels is 0.34 ms in ONE wave while two thousand others have nothing to do)
        const bool rows = map.order == nullptr && map.row_packets != 0u;
        const uint32_t c = map.order != nullptr ? (unit & 0xFFFFFu) : (rows ? unit >> 3 : unit);
        chunk_pos = map.order != nullptr ? ((unit >> 20) & 63u) : (rows ? (unit & 7u) * 8u : 0u);
        chunk_end = map.order != nullptr ? chunk_pos + (unit >> 26) + 1u : (rows ? chunk_pos + 8u : 64u);
        // wave-uniform placement of the chunk, once per fetch (scalar unit)
        const uint32_t region = c / map.chunks_per_region;
        const uint32_t cr = c - region * map.chunks_per_region;
        const uint32_t ccy = cr / map.chunks_x;
        chunk_rx0 = (cr - ccy * map.chunks_x) * 8u;
        chunk_ry0 = ccy * 8u;
        if (map.mode == 0u) {
          chunk_px0 = map.x0;
          chunk_py0 = map.y0;
          chunk_w = map.w;
          chunk_h = map.h;
          chunk_out0 = 0;
        } else {
          const uint32_t tile = map.mode == 1u ? map.first_tile + region * map.tile_stride : map.tile_list[region];
          const uint32_t ty = tile / map.tiles_x;
          chunk_px0 = (tile - ty * map.tiles_x) * map.tile_w;
          chunk_py0 = ty * map.tile_h;
          chunk_w = map.tile_w;
          chunk_h = map.tile_h;
          chunk_out0 = static_cast<size_t>(region) * map.tile_h * map.tile_w;
        }
      }
      const uint32_t avail = chunk_end - chunk_pos;
      const uint32_t rank = bits_below(wmask);
      if (want && rank < avail) {
        const uint32_t k = chunk_pos + rank;  // pixel k of the 8x8 chunk
        const uint32_t rx = chunk_rx0 + (k & 7u), ry = chunk_ry0 + (k >> 3);
        const bool in_buffer = rx < chunk_w && ry < chunk_h;
        const uint32_t px = chunk_px0 + rx, py = chunk_py0 + ry;
        if (in_buffer && px < cam.hsize && py < cam.vsize) {
          new_px = px;
          new_py = py;
          got_pixel = true;
          want = false;
          out_index = chunk_out0 + static_cast<size_t>(ry) * chunk_w + rx;
        }  // pixels of an edge tile outside the image are not written (rtc.h: the caller's padding is left alone)
      }
      chunk_pos += min(avail, static_cast<uint32_t>(__builtin_popcountll(wmask)));
      wmask = __ballot(want);
    }
    if constexpr (MS) {
      if (got_pixel || next_sample) {  // a new pixel's sample 0, or the owner's next sample of its pixel
        uint32_t k = 0u;
        if (next_sample) {
          k = *samp_word & RTC_SAMPLE_MASK;
          map_pixel(map, out_index, new_px, new_py);
        } else {
          *samp_word = RTC_SAMPLE_OWNER;
          shared = false;
          acc[0] = acc[1] = acc[2] = 0.0;
        }
        cur.ray = camera_sample(cam, smp, new_px, new_py, k);
        cur.weight = smp.weight;  // (the pixel is the samples' mean: each adds 1 / samples of its colour)
        RTC_MEDIA_START(cur, smp.weight);  // (MEDIA: the camera stands in the atmosphere)
        cur.remaining = max_depth;
        RTC_SET_CODE(cur, 1u);  // (GLOSS) the primary ray
        RTC_SET_LIN(cur, 0u);   // (INDIRECT) no diffuse bounce yet
        have_cur = true;
        has_pixel = true;
        n_primary++;
      }
    } else if (got_pixel) {  // once per refill, however many items the pixels came from
      // Camera.rayForPixel, camera.zig:64-76
      const double xoffset = (static_cast<double>(new_px) + 0.5) * cam.pixel_size;
      const double yoffset = (static_cast<double>(new_py) + 0.5) * cam.pixel_size;
      const double world_x = cam.half_width - xoffset;
      const double world_y = cam.half_height - yoffset;
      const double pix_x = row_pt(cam.inv + 0, world_x, world_y, -1.0);
      const double pix_y = row_pt(cam.inv + 4, world_x, world_y, -1.0);
      const double pix_z = row_pt(cam.inv + 8, world_x, world_y, -1.0);
      cur.ray.ox = row_pt(cam.inv + 0, 0.0, 0.0, 0.0);
      cur.ray.oy = row_pt(cam.inv + 4, 0.0, 0.0, 0.0);
      cur.ray.oz = row_pt(cam.inv + 8, 0.0, 0.0, 0.0);
      double dx = pix_x - cur.ray.ox, dy = pix_y - cur.ray.oy, dz = pix_z - cur.ray.oz;
      const double mag = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);  // Tuple.normalized, tuple.zig:109-116
      if (mag != 0.0) {
        if (kSharedNormalize && __ballot(!shared_normalize_ok(dx, dy, dz, mag)) == 0ull) {
          shared_normalize(dx, dy, dz, mag);
        } else {
          dx = dx / mag;
          dy = dy / mag;
          dz = dz / mag;
        }
      }
      cur.ray.dx = dx;
      cur.ray.dy = dy;
      cur.ray.dz = dz;
      cur.weight = 1.0;
      RTC_MEDIA_START(cur, 1.0);
      cur.remaining = max_depth;
      RTC_SET_CODE(cur, 1u);  // (GLOSS) the primary ray
      RTC_SET_LIN(cur, 0u);   // (INDIRECT) no diffuse bounce yet
      have_cur = true;
      has_pixel = true;
      shared = false;
      acc[0] = acc[1] = acc[2] = 0.0;
      n_primary++;
    }
    if (!__any(have_cur)) break;
    // ---- 3. (COOP kernels) a wave with at most eight rays left lends each of them eight lanes.  The wave's instruction
    // stream is what bounds it then - one wave issues an instruction every four cycles at best, and an iteration is 5 000
    // of them whether one lane has a ray or all 64 -, so the k-th ray goes to the aligned group of lanes 8k .. 8k + 7:
    // all eight run the iteration on the same ray and take identical branches, but inside trace() each takes its share of
    // World.objects and the group's visitors are merged.  What the iteration yields - the colour it adds to the pixel, the
    // children it spawns, its counts - travels back to the lane that owns the pixel (step 4), which is the only one with
    // side effects.  A glass pixel's chain of dependent iterations, the floor under every small launch and every rank's
    // share of a split frame, gets shorter; full waves never come here.
    struct Yield {  // (only the COOP kernels use it)
      double contrib[3] = {0.0, 0.0, 0.0};
      Pending kid_now, kid_later;  // the child that continues at once (the reflection when there are two), the one that waits
      uint32_t n_kids = 0u, share = 0u, secondary = 0u, shadow_calls = 0u, shadow_traced = 0u, overflow = 0u;
    } yield;
    bool coop = false, work = have_cur;
    uint32_t member = 0u, stride = 1u, yield_from = 0u;
    const bool owner = have_cur;
    if constexpr (COOP) {
      const unsigned long long live = __ballot(have_cur);
      const uint32_t n_live = static_cast<uint32_t>(__builtin_popcountll(live));
      coop = n_live <= 8u;  // (wave-uniform; at least one)
      if (coop) {
        uint32_t src = 0u;  // the lane whose ray this lane's group works on: the (lane / 8)-th lane with a ray
        unsigned long long m = live;
        for (uint32_t k = 0; k < n_live; ++k) {
          const uint32_t b = static_cast<uint32_t>(__builtin_ctzll(m));
          m &= m - 1ull;
          if ((lane >> 3) == k) src = b;
        }
        yield_from = 8u * bits_below(live);  // (for an owner: the first lane of the group that works on its ray)
        Pending w;
        w.ray = {__shfl(cur.ray.ox, src), __shfl(cur.ray.oy, src), __shfl(cur.ray.oz, src),
                 __shfl(cur.ray.dx, src), __shfl(cur.ray.dy, src), __shfl(cur.ray.dz, src)};
        w.weight = __shfl(cur.weight, src);
        w.remaining = __shfl(cur.remaining, src);
        cur = w;
        work = (lane >> 3) < n_live;
        member = lane & 7u;
        stride = 8u;
      }
    }
    if constexpr (!COOP) {
      if (!have_cur) continue;
    }
    have_cur = false;  // `cur` is consumed; a spawned child may refill it below
    // (the counts an iteration makes: the lane's own, or - cooperative kernels - the iteration's yield)
    unsigned& it_share = COOP ? yield.share : share_rays;
    unsigned& it_secondary = COOP ? yield.secondary : n_secondary;
    unsigned& it_shadow_calls = COOP ? yield.shadow_calls : n_shadow_calls;
    unsigned& it_shadow_traced = COOP ? yield.shadow_traced : n_shadow_traced;
    unsigned& it_overflow = COOP ? yield.overflow : overflow;
    if (work) do {  // (`continue` below ends the iteration's work, not the loop's turn: step 4 follows)
    it_share += 2u;
    cur.remaining = min(cur.remaining, max_depth);  // termination never depends on a value read back from memory
    const Ray ray = cur.ray;
    // (MOTION) the shutter time of the ray's camera sample, which its reflected, refracted and shadow rays share: the camera
    // hash on its own axis, recomputed from the lane's pixel and sample word whenever a ray starts - a register for the
    // length of the iteration, nothing in LDS
    double tm = 0.0;
    if constexpr (MOTION) {
      uint32_t px, py;
      map_pixel(map, out_index, px, py);
      const unsigned long long p = static_cast<unsigned long long>(py) * cam.hsize + px;
      tm = rtc_camera_jitter(smp.key, p, smp.sample_base + (*samp_word & RTC_SAMPLE_MASK), RTC_MOTION_AXIS);
    }

    // ---- World.colorAt: intersect + hit (world.zig:111-115)
    RTC_STAMP(1);
#ifdef RTC_PROFILE
    prof_iters += 1ull;
#endif
    using HitVisitor = typename std::conditional<MOTION, MotionClosestVisitor, ClosestVisitor>::type;
    HitVisitor hv;
    RTC_COUNT(0);
    {
      RTC_HIST_BEGIN();
      trace<CSG, WORLD, HitVisitor, TRAV, BOX, MOTION, ROOTS>(S, recs, cull, ray, hv, it_overflow, trav_stack, member, stride, mo.disp, tm);
      RTC_HIST_END(0);
    }
    RTC_STAMP(2);
#ifdef RTC_MEDIA_TU
    // (MEDIA, rtc.h's rtc_scene_set_media) the step: the segment's transmittance per channel, before shading and before the
    // children are formed; in the atmosphere the fog's in-scatter goes to the pixel.  sigma == 0 gives T == 1 exactly and
    // a density of zero forms no fog term: a handle without media keeps its bits.  A wave none of whose lanes has a
    // non-zero sigma branches around the three exp.
    if constexpr (MEDIA) {
      const bool atmosphere = cur.medium == RTC_NO_MEDIUM;
      double s_r = media.fog_density, s_g = media.fog_density, s_b = media.fog_density;
      if (!atmosphere) {
        const double* __restrict__ A = media.absorption + 3ull * cur.medium;
        s_r = A[0];
        s_g = A[1];
        s_b = A[2];
      }
      double t_r = 1.0, t_g = 1.0, t_b = 1.0;
      if (__any(s_r != 0.0 || s_g != 0.0 || s_b != 0.0)) {
        if (hv.leaf != RTC_NO_LEAF) {
          const double dist = hv.t * __builtin_sqrt((ray.dx * ray.dx + ray.dy * ray.dy) + ray.dz * ray.dz);
          t_r = s_r == 0.0 ? 1.0 : exp(-(s_r * dist));
          t_g = s_g == 0.0 ? 1.0 : exp(-(s_g * dist));
          t_b = s_b == 0.0 ? 1.0 : exp(-(s_b * dist));
        } else {
          t_r = s_r == 0.0 ? 1.0 : 0.0;
          t_g = s_g == 0.0 ? 1.0 : 0.0;
          t_b = s_b == 0.0 ? 1.0 : 0.0;
        }
      }
      if (atmosphere && media.fog_density > 0.0) {
        acc[0] = acc[0] + cur.weight * ((1.0 - t_r) * media.fog_color[0]);
        acc[1] = acc[1] + cur.weight_g * ((1.0 - t_g) * media.fog_color[1]);
        acc[2] = acc[2] + cur.weight_b * ((1.0 - t_b) * media.fog_color[2]);
      }
      cur.weight = cur.weight * t_r;
      cur.weight_g = cur.weight_g * t_g;
      cur.weight_b = cur.weight_b * t_b;
    }
    uint32_t kid_medium = RTC_NO_MEDIUM;  // the medium of a refracted child: the material that supplies n2, or none
#endif
#ifdef RTC_ENV_TU
    // (ENV, rtc.h's rtc_scene_set_environment) the sky: a ray that found nothing adds its weight - after the media step, so
    // with the miss transmittance in it - times the sky's colour at its direction.  The pattern is evaluated at the point
    // where the direction meets the unit sphere or the unit cube, as at an object-space point, with no hit triangle.  A
    // wave none of whose lanes missed, and every wave of a handle without a sky, branches around it.
    if constexpr (ENV) {
      const bool missed = hv.leaf == RTC_NO_LEAF;
      if (env.sky != 0u && __any(missed)) {
#ifdef RTC_INDIR_TU
        // (INDIRECT) where the sky-light step ran at its parent's hit, a diffuse child's own miss adds no sky: the step
        // counted it.  Only the ray formed as a diffuse child; its reflected and refracted descendants add the sky as before.
        const bool sky_counted = INDIRECT && (cur.lin & RTC_LIN_DIFFUSE) != 0u && skyl.gain > 0.0;
        if (missed && !sky_counted) {
#else
        if (missed) {
#endif
          double e_r = env.rgb[0], e_g = env.rgb[1], e_b = env.rgb[2];
          if (env.pattern != RTC_ENV_NO_PATTERN) {
            const double len = env.projection == RTC_ENV_CUBE
                                   ? __builtin_fmax(__builtin_fabs(ray.dx), __builtin_fmax(__builtin_fabs(ray.dy), __builtin_fabs(ray.dz)))
                                   : __builtin_sqrt((ray.dx * ray.dx + ray.dy * ray.dy) + ray.dz * ray.dz);
            const MeshUvHit mh{muv.row, RTC_NO_LEAF, 0.0, 0.0};
            const Rgb c = pattern_at_shared(S, pats, env.pattern, ray.dx / len, ray.dy / len, ray.dz / len, mh);
            e_r = c.r * e_r;
            e_g = c.g * e_g;
            e_b = c.b * e_b;
          }
          acc[0] = acc[0] + cur.weight * e_r;
          acc[1] = acc[1] + cur.weight_g * e_g;
          acc[2] = acc[2] + cur.weight_b * e_b;
        }
      }
    }
#endif
    if (hv.leaf == RTC_NO_LEAF) continue;  // black (world.zig:119)

    // ---- PreComputations.new (world.zig:212-227)
    // the hit Shape: its record sits in the (LDS) root table when it is a top-level object,
    // otherwise it is a leaf inside a group and comes from the leaf tables in memory
    uint32_t kind, geom, mat_index;
    [[maybe_unused]] bool hit_alone = false;  // (kOwnRoot) the hit root carries RTC_ROOT_ALONE
    // The hit shape's inverse.  The kernels that walk BVHs are at their register limit with values in scratch memory:
    // there the matrix is READ WHERE IT IS USED (three times: the local point, the normal, the pattern point) from where
    // it lives - the root record in LDS or the transform table - instead of sitting in 24 VGPRs from the hit to the
    // pattern lookup (rtc_render_kernel 95 -> 54 spilled VGPRs, dragons 4K 2.33 -> 2.30 ms).  The kernels without the
    // group traversal keep their copy: the three-wave kernel spills as much either way and writes 390 instead of 281 MB
    // per cover frame without it.
    double M_copy[FLAT ? 12 : 1];
    const double* M = M_copy;
    DevCyl hcy{0.0, 0.0, 0u, 0u};
    if (FLAT || hv.root != RTC_NO_LEAF) {  // (a world without groups: every hit is a top-level object)
      const RootRec& R = recs[RTC_CHECK_INDEX(RTC_OOB_ROOTS, hv.root, RTC_AVAIL(0))];
      if constexpr (FLAT) {
#pragma unroll
        for (int i = 0; i < 12; ++i) M_copy[i] = R.inv[i];
      } else {
        M = R.inv;
      }
      kind = R.kind_flags & 0xFFu;
      if constexpr (kOwnRoot) hit_alone = (R.kind_flags & RTC_ROOT_ALONE) != 0u;
      geom = R.geom;
      mat_index = R.material;
      hcy.ymin = R.ymin;
      hcy.ymax = R.ymax;
    } else {
      const uint4 meta = S.leaf_meta[hv.leaf];
      M = S.xf + 12ull * meta.y;
      kind = meta.x & 0xFFu;
      geom = meta.w;
      mat_index = meta.z;
      if (RTC_HAS_CYL_ROW(kind)) hcy = S.cyl[geom];
    }
#ifdef RTC_PROFILE
    mat_index = RTC_CHECK_INDEX(RTC_OOB_MATERIALS, mat_index, RTC_AVAIL(3));
#endif
    RTC_STAMP(10);
    const double t = hv.t;
    // ---- n1 / n2 of PreComputations.new (world.zig:229-255), needed only if a refracted ray can be
    // spawned.  Traced FIRST, while nothing of the shading is live yet (register peak, see pass 1 / 2 below).
    double n1 = 1.0, n2 = 1.0;
    if (cur.remaining != 0u && !(mats[mat_index].transparency == 0.0)) {
      RTC_STAMP(5);
      it_share += 2u;
      using BehindVisitor = BehindVisitorT<WORLD == 2>;
      BehindVisitor bv;
      bv.hit_leaf = hv.leaf;
      bv.hit_t = t;
      RTC_COUNT(4);
      // (kOwnRoot) decided for the wave, among the lanes that are here: every hit root alone, and the trace below keeps of
      // each lane's roots the hit root only - no ray set-up, no phase 1, no plane step (trace(), OWN).  In a cooperative
      // iteration the lanes of a group hold the same ray and the same hit: each tests that root itself and leaves with the
      // whole result, nothing is merged (merge_group adds hit_dups across a group's lanes, which is right only where every
      // root was tested by one of them).  One lane on any other root and the whole wave makes the pass as before.
      bool own_root = false;
      if constexpr (kOwnRoot) own_root = !__any(!hit_alone);
      if (!own_root) RTC_AUX_ADD(7, 1);  // (diagnostic builds: the passes the wave makes in full, counted by its first active lane - RTC_COUNT's are lane 0's)
      {
        RTC_HIST_BEGIN();
        trace<CSG, WORLD, BehindVisitor, TRAV, BOX, MOTION, 64, kOwnRoot>(S, recs, cull, ray, bv, it_overflow, trav_stack, member, stride, mo.disp, tm,
                                                                          own_root, kOwnRoot ? hv.root : 0u);
        RTC_HIST_END(2);
      }
        RTC_STAMP(6);
      bv.template flush<true>();
      const double hit_ior = mats[mat_index].ior;
      if (bv.best_leaf != RTC_NO_LEAF) n1 = mats[RTC_CHECK_INDEX(RTC_OOB_MATERIALS, bv.best_mat, RTC_AVAIL(3))].ior;
      if (!bv.hit_open) {
        n2 = hit_ior;
      } else if (bv.best_excl_leaf != RTC_NO_LEAF) {
        n2 = mats[RTC_CHECK_INDEX(RTC_OOB_MATERIALS, bv.best_excl_mat, RTC_AVAIL(3))].ior;
      } else if (bv.hit_dups >= 2u) {
        n2 = hit_ior;
      }
#ifdef RTC_MEDIA_TU
      // (MEDIA) the refracted child's medium: the material whose ior was just taken for n2
      kid_medium = !bv.hit_open ? mat_index : (bv.best_excl_leaf != RTC_NO_LEAF ? bv.best_excl_mat : (bv.hit_dups >= 2u ? mat_index : RTC_NO_MEDIUM));
#endif
    }
    const double ptx = ray.ox + ray.dx * t, pty = ray.oy + ray.dy * t, ptz = ray.oz + ray.dz * t;  // ray.position
    const double ex = -ray.dx, ey = -ray.dy, ez = -ray.dz;                                          // eyev
    // (MOTION) world space -> the hit object's space goes through the point where the hit root rests: p - tm * D, for the
    // normal and for the pattern; a translation leaves the normal transform as it is
    double spx = ptx, spy = pty, spz = ptz, mdx = 0.0, mdy = 0.0, mdz = 0.0;
    if constexpr (MOTION) {
      const double* __restrict__ D = mo.disp + 3ull * hv.hit_root;
      mdx = D[0];
      mdy = D[1];
      mdz = D[2];
      spx = ptx - tm * mdx;
      spy = pty - tm * mdy;
      spz = ptz - tm * mdz;
    }
    // Shape.normalAt (shape.zig:338-350): local point, local normal, normalToWorld
    const double lpx = row_pt(M + 0, spx, spy, spz);
    const double lpy = row_pt(M + 4, spx, spy, spz);
    const double lpz = row_pt(M + 8, spx, spy, spz);
    double lnx, lny, lnz;
    switch (SIMPLE ? min(kind, 2u) : kind) {
      case 0:  // sphere.zig:48-53
        lnx = lpx;
        lny = lpy;
        lnz = lpz;
        break;
      case 1:  // plane.zig:38-43
        lnx = 0.0;
        lny = 1.0;
        lnz = 0.0;
        break;
      case 2: {  // cube.zig:81-97
        const double ax = __builtin_fabs(lpx), ay = __builtin_fabs(lpy), az = __builtin_fabs(lpz);
        const double maxc = zmax(ax, zmax(ay, az));
        lnx = lny = lnz = 0.0;
        if (maxc == ax) {
          lnx = lpx;
        } else if (maxc == ay) {
          lny = lpy;
        } else {
          lnz = lpz;
        }
        break;
      }
      case 3: {  // cylinder.zig:100-112
        const DevCyl cy = hcy;
        const double dist = lpx * lpx + lpz * lpz;
        if (dist < 1.0 && lpy >= cy.ymax - 1e-5) {
          lnx = 0.0; lny = 1.0; lnz = 0.0;
        } else if (dist < 1.0 && lpy <= cy.ymin + 1e-5) {
          lnx = 0.0; lny = -1.0; lnz = 0.0;
        } else {
          lnx = lpx; lny = 0.0; lnz = lpz;
        }
        break;
      }
      case 6: {  // cone.zig:115-132
        const DevCyl cy = hcy;
        const double dist = lpx * lpx + lpz * lpz;
        if (dist < cy.ymax * cy.ymax && lpy >= cy.ymax - 1e-4) {
          lnx = 0.0; lny = 1.0; lnz = 0.0;
        } else if (dist < cy.ymin * cy.ymin && lpy <= cy.ymin + 1e-4) {
          lnx = 0.0; lny = -1.0; lnz = 0.0;
        } else {
          const double sgn = lpy > 0.0 ? 1.0 : (lpy < 0.0 ? -1.0 : lpy);  // std.math.sign
          lnx = lpx;
          lny = -sgn * __builtin_sqrt(lpx * lpx + lpz * lpz);
          lnz = lpz;
        }
        break;
      }
#ifdef RTC_TORUS_TU
      case 7: {  // RTC_TORUS (rtc.h): the point minus the nearest point of the tube's centre circle
        if constexpr (TORUS) {
          const double R = hcy.ymin;
          const double rho = __builtin_sqrt(lpx * lpx + lpz * lpz);
          lny = lpy;
          if (rho == 0.0) {
            lnx = 0.0;
            lnz = 0.0;
          } else {
            lnx = lpx - R * (lpx / rho);
            lnz = lpz - R * (lpz / rho);
          }
        }
        break;
      }
#endif
      case 4: {  // triangle.zig:65-70: the stored face normal
        const double* __restrict__ N = S.trin + 9ull * geom;
        lnx = N[0]; lny = N[1]; lnz = N[2];
        break;
      }
      default: {  // smooth triangle, triangle.zig:261-265: n2*u + n3*v + n1*(1-u-v)
        const double* __restrict__ N = S.trin + 9ull * geom;
        const double w1 = (1.0 - hv.u) - hv.v;
        lnx = (N[3] * hv.u + N[6] * hv.v) + N[0] * w1;
        lny = (N[4] * hv.u + N[7] * hv.v) + N[1] * w1;
        lnz = (N[5] * hv.u + N[8] * hv.v) + N[2] * w1;
        break;
      }
    }
    // normalToWorld (shape.zig:139-145): rows of inverse-transpose == columns of the inverse
    double nx = (M[0] * lnx + M[4] * lny) + M[8] * lnz;
    double ny = (M[1] * lnx + M[5] * lny) + M[9] * lnz;
    double nz = (M[2] * lnx + M[6] * lny) + M[10] * lnz;
    {
      const double mag = __builtin_sqrt((nx * nx + ny * ny) + nz * nz);
      if (mag != 0.0) {
        if (kSharedNormalize && __ballot(!shared_normalize_ok(nx, ny, nz, mag)) == 0ull) {
          shared_normalize(nx, ny, nz, mag);
        } else {
          nx = nx / mag;
          ny = ny / mag;
          nz = nz / mag;
        }
      }
    }
    const bool inside = ((nx * ex + ny * ey) + nz * ez) < 0.0;  // world.zig:218-221
    if (inside) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    // The shading normal: what Material.lighting, reflectv, refractedColor and schlick read.  (nx, ny, nz) stays the
    // geometric normal: inside, over_point, under_point - and n1 / n2, traced above - come from it alone.
    // (BUMP) a material with a bump (rtc_scene_set_bumps; the row is read per lane, mat_index being the lane's): the unit
    // local normal plus the field at B * local point times the amplitude, through normalToWorld, negated by the decision
    // above.  A row of kind none leaves the geometric normal's bits.
    double hx = nx, hy = ny, hz = nz;
    if constexpr (BUMP) {
      const double* __restrict__ R = bumps.row + static_cast<size_t>(RTC_BUMP_ROW) * mat_index;
      const double bump_kind = R[14];
      const double lmag = bump_kind != 0.0 ? __builtin_sqrt((lnx * lnx + lny * lny) + lnz * lnz) : 0.0;  // tuple.zig's normalize
      if (lmag != 0.0) {
        const double qx = row_pt(R + 0, lpx, lpy, lpz);
        const double qy = row_pt(R + 4, lpx, lpy, lpz);
        const double qz = row_pt(R + 8, lpx, lpy, lpz);
        double d0, d1, d2;
        if (bump_kind == 1.0) {  // RTC_BUMP_NOISE: perturb.zig:31-43's three evaluations
          const uint32_t octaves = static_cast<uint32_t>(R[15]);
          const double persistence = R[13];
          d0 = octave_noise(qx, qy, qz, octaves, persistence);
          d1 = octave_noise(qx, qy, qz + 1.0, octaves, persistence);
          d2 = octave_noise(qx, qy, qz + 2.0, octaves, persistence);
        } else {  // RTC_BUMP_RIPPLES
          d1 = 0.0;
          bump_ripples(qx, qz, d0, d2);
        }
        const double amp = R[12];
        const double bx = lnx / lmag + d0 * amp, by = lny / lmag + d1 * amp, bz = lnz / lmag + d2 * amp;
        hx = (M[0] * bx + M[4] * by) + M[8] * bz;
        hy = (M[1] * bx + M[5] * by) + M[9] * bz;
        hz = (M[2] * bx + M[6] * by) + M[10] * bz;
        const double mag = __builtin_sqrt((hx * hx + hy * hy) + hz * hz);
        if (mag != 0.0) {
          hx = hx / mag;
          hy = hy / mag;
          hz = hz / mag;
        }
        if (inside) {
          hx = -hx;
          hy = -hy;
          hz = -hz;
        }
      }
    }
    RTC_STAMP(11);
    const double eps = 1e-5;
    const double ovx = ptx + nx * eps, ovy = pty + ny * eps, ovz = ptz + nz * eps;  // over_point
#ifdef RTC_OCCL_TU
    // (OCCL) the hit's ambient factor, once, before the colour and the lights' temporaries exist: the material's radius is
    // read per lane (mat_index is the lane's); only a lane with a radius and an ambient term forms the hash of its camera
    // sample - the whole-image pixel and the global sample index, as the gloss block below - and traces `samples` shadow-type
    // rays of that length from over_point, the area branch's call.  What the loop keeps is an integer count, so the factor
    // does not depend on the order the rays ran in; every sample is a call of isShadowed and is traced.
    double occl_ka = mats[mat_index].ambient;
    if constexpr (OCCL) {
      const double occl_radius = occl.row[mat_index];
      if (occl_radius > 0.0 && occl_ka != 0.0) {
        uint32_t opx, opy;
        map_pixel(map, out_index, opx, opy);
        const unsigned long long occl_h = rtc_gloss_sample_key(
            RTC_DKEY(occl.key), static_cast<unsigned long long>(opy) * cam.hsize + opx,
            static_cast<unsigned long long>(smp.sample_base) + (*samp_word & RTC_SAMPLE_MASK));
        uint32_t clear = 0u;
        for (uint32_t k = 0u; k < occl.samples; ++k) {
          const GlossDir od = occl_direction(occl_h, (k << RTC_OCCLUSION_SAMPLE_SHIFT) | cur.code, nx, ny, nz);
          it_shadow_calls++;
          it_shadow_traced++;
          it_share++;
          ShadowVisitor sv;
          sv.distance = occl_radius;
          Ray sray{ovx, ovy, ovz, od.x, od.y, od.z};
          trace<CSG, WORLD, ShadowVisitor, TRAV, BOX, MOTION, ROOTS>(S, recs, cull, sray, sv, it_overflow, trav_stack, member, stride, mo.disp, tm);
          clear += sv.shadowed ? 0u : 1u;
        }
        if (clear != occl.samples) occl_ka = occl_ka * (static_cast<double>(clear) / static_cast<double>(occl.samples));
      }
    }
#endif
    // ---- World.shadeHit, lights loop (world.zig:89-96)
    double sr = 0.0, sg = 0.0, sb = 0.0;
#ifdef RTC_INDIR_TU
    double ind_r = 0.0, ind_g = 0.0, ind_b = 0.0;  // (INDIRECT) colour * diffuse of this hit, for the diffuse child's weight
#endif
    {
      const DevMaterial& mat = mats[mat_index];
      // Pattern.patternAtShape (pattern.zig:128-131) looks the colour up at over_point in object space - but a world all of
      // whose patterns are solid colours (cover, dragons, groups; DevScene::all_solid, a branch of the wave, not of its
      // lanes: solid.zig:20-24 looks at no point) needs neither the point nor the pattern code: cover 0.462 -> 0.446 ms,
      // cubes - 1.4 % (the form alone), dragons 4K - 1.1 %, nefertiti - 1.3 %.  The simple kernels that cull by spheres keep
      // the plain form: with the branch reflection_and_refraction lost 3-5 % to the register allocator (HISTORY).
      constexpr bool SOLID_PATH = RTC_ALL_SOLID_FORM != 0 && !(WORLD == 2 && !BOX);
      Rgb color;
      if (SOLID_PATH && S.all_solid != 0u) {
        const DevPattern& P = pats[RTC_CHECK_INDEX(RTC_OOB_PATTERNS, mat.pattern, RTC_AVAIL(4))];
        color = {P.rgb[0], P.rgb[1], P.rgb[2]};
      } else {
        double qx = ovx, qy = ovy, qz = ovz;  // (MOTION: over_point - tm * D)
        if constexpr (MOTION) {
          qx = ovx - tm * mdx;
          qy = ovy - tm * mdy;
          qz = ovz - tm * mdz;
        }
        const double opx = row_pt(M + 0, qx, qy, qz);
        const double opy = row_pt(M + 4, qx, qy, qz);
        const double opz = row_pt(M + 8, qx, qy, qz);
#ifdef RTC_MESHUV_TU
        // (MESHUV) the hit's triangle - geom is its tri_* index - and the entry's barycentrics, as Moller-Trumbore left them
        const MeshUvHit mh{muv.row, ((kind == 4u || kind == 5u) && muv.row != nullptr) ? geom : RTC_NO_LEAF, hv.u, hv.v};
#endif
        color = pattern_at<CSG>(S, pats, RTC_CHECK_INDEX(RTC_OOB_PATTERNS, mat.pattern, RTC_AVAIL(4)), opx, opy, opz RTC_MESHUV_ARG);
      }
      RTC_STAMP(12);
      // With diffuse == 0 and specular == 0 lighting() returns `ambient` whether or not the
      // point is shadowed (material.zig:55-73), so the shadow ray cannot change the result.
      const bool shadow_matters = !(mat.diffuse == 0.0 && mat.specular == 0.0);
      // (a cooperative iteration of a world with at most two lights deals them to the two halves of the ray's group: lanes
      // 0-3 take light 0, lanes 4-7 light 1, each half tracing its shadow ray four lanes wide; the halves' terms are added
      // below, (0 + l0) + (0 + l1): the reference's running sum of world.zig:89-96 to the bit.  With three or more lights
      // the halves' partial sums would round differently from that running sum - and whether an iteration runs
      // cooperatively depends on the schedule -, so there every lane of the group takes all lights, in order, with its
      // shadow rays traced eight lanes wide: a pixel's colour never depends on how its iterations were run.)
      const bool deal_lights = COOP && coop && S.n_lights <= 2u;
      const uint32_t li_first = deal_lights ? (member >> 2) : 0u, li_step = deal_lights ? 2u : 1u;
      const uint32_t s_member = deal_lights ? (member & 3u) : member, s_stride = deal_lights ? 4u : stride;
      const unsigned calls_before = it_shadow_calls, traced_before = it_shadow_traced, share_before = it_share;
      for (uint32_t li = li_first; li < S.n_lights; li += li_step) {
#ifdef RTC_PROFILE
        if (!RTC_IN_BOUNDS(RTC_OOB_LIGHTS, 6u * li + 6u <= RTC_AVAIL(5))) continue;
        if (AREA && !RTC_IN_BOUNDS(RTC_OOB_LIGHTS, RTC_AREA_ROW * li + RTC_AREA_ROW <= area_avail)) continue;
#endif
        if constexpr (AREA) {
          const double* __restrict__ A = area_rows + static_cast<size_t>(RTC_AREA_ROW) * li;
          const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(A[12]));
          if ((bits >> RTC_AREA_KIND_BIT) & 1ull) {
            // ---- an area light (the book's bonus chapter): two passes over its samples, v outer, u inner.  The first
            // builds the diffuse + specular sum and traces nothing; only when that sum is not zero - a sample in front of the
            // surface, a material that is not pure ambient - does the second trace the samples' shadow rays.  What it yields
            // is an integer count, so the colour does not depend on the order the rays ran in.
            const uint32_t us = static_cast<uint32_t>(bits) & ((1u << RTC_AREA_STEP_BITS) - 1u);
            const uint32_t vs = static_cast<uint32_t>(bits >> RTC_AREA_STEP_BITS) & ((1u << RTC_AREA_STEP_BITS) - 1u);
            const bool jitter = (bits >> RTC_AREA_JITTER_BIT) & 1ull;
            const uint32_t n_samples = us * vs;
            it_shadow_calls += n_samples;
            // the whole image's pixel of this ray tree (out_index travels with a ray handed to another lane): the jitter's key
            unsigned long long pixel = 0ull;
            if (jitter) {
              uint32_t px, py;
              if (map.mode == 0u) {
                const uint32_t ry = static_cast<uint32_t>(out_index / map.w);
                px = map.x0 + static_cast<uint32_t>(out_index - static_cast<size_t>(ry) * map.w);
                py = map.y0 + ry;
              } else {
                const size_t per_tile = static_cast<size_t>(map.tile_w) * map.tile_h;
                const uint32_t region = static_cast<uint32_t>(out_index / per_tile);
                const uint32_t r = static_cast<uint32_t>(out_index - static_cast<size_t>(region) * per_tile);
                const uint32_t ry = r / map.tile_w, rx = r - ry * map.tile_w;
                const uint32_t tile = map.mode == 1u ? map.first_tile + region * map.tile_stride : map.tile_list[region];
                const uint32_t ty = tile / map.tiles_x;
                px = (tile - ty * map.tiles_x) * map.tile_w + rx;
                py = ty * map.tile_h + ry;
              }
              pixel = static_cast<unsigned long long>(py) * cam.hsize + px;
              if constexpr (MS) pixel = pixel * smp.samples + (*samp_word & RTC_SAMPLE_MASK) + smp.pixel_base;  // (u64, wraps)
            }
            // point_on_light(u, v) - over_point
            auto to_sample = [&](uint32_t u, uint32_t v, double& vx, double& vy, double& vz) {
              double ju = 0.5, jv = 0.5;
              if (jitter) {
                const uint32_t k = v * us + u;
                ju = rtc_area_jitter(area.seed, pixel, S.n_lights, li, k, 0u);
                jv = rtc_area_jitter(area.seed, pixel, S.n_lights, li, k, 1u);
              }
              const double fu = static_cast<double>(u) + ju, fv = static_cast<double>(v) + jv;
              vx = ((A[0] + A[3] * fu) + A[6] * fv) - ovx;
              vy = ((A[1] + A[4] * fu) + A[7] * fv) - ovy;
              vz = ((A[2] + A[5] * fu) + A[8] * fv) - ovz;
            };
            const double er = color.r * A[9], eg = color.g * A[10], eb = color.b * A[11];  // effective_color
            const double ka = RTC_KA(mat);
            double lr_ = er * ka, lg_ = eg * ka, lb_ = eb * ka;
            double dr = 0.0, dg = 0.0, db = 0.0;
            if (shadow_matters) {
              for (uint32_t v = 0u; v < vs; ++v)
                for (uint32_t u = 0u; u < us; ++u) {
                  double vx, vy, vz;
                  to_sample(u, v, vx, vy, vz);
                  const double distance = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
                  double lvx = vx, lvy = vy, lvz = vz;
                  if (distance != 0.0) {
                    lvx = vx / distance;
                    lvy = vy / distance;
                    lvz = vz / distance;
                  }
                  const double light_dot_normal = (lvx * hx + lvy * hy) + lvz * hz;
                  if (light_dot_normal >= 0.0) {
                    const double kd = mat.diffuse * light_dot_normal;
                    dr = dr + er * kd;
                    dg = dg + eg * kd;
                    db = db + eb * kd;
                    const double two_dot = 2.0 * light_dot_normal;
                    const double rx = lvx - hx * two_dot, ry = lvy - hy * two_dot, rz = lvz - hz * two_dot;
                    const double reflect_dot_eye = ((-rx) * ex + (-ry) * ey) + (-rz) * ez;
                    if (reflect_dot_eye > 0.0) {
                      const uint32_t n = mat.shininess_int;
                      const double ks = mat.specular * (n != 0u && reflect_dot_eye < kInf ? pow_small_int(reflect_dot_eye, n)
                                                                                          : zig_pow(reflect_dot_eye, mat.shininess));
                      dr = dr + A[9] * ks;
                      dg = dg + A[10] * ks;
                      db = db + A[11] * ks;
                    }
                  }
                }
            }
            if (!(dr == 0.0 && dg == 0.0 && db == 0.0)) {
              RTC_LIT_DECL;
              for (uint32_t v = 0u; v < vs; ++v)
                for (uint32_t u = 0u; u < us; ++u) {
                  double vx, vy, vz;
                  to_sample(u, v, vx, vy, vz);
                  const double distance = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
                  double lvx = vx, lvy = vy, lvz = vz;
                  if (distance != 0.0) {
                    lvx = vx / distance;
                    lvy = vy / distance;
                    lvz = vz / distance;
                  }
                  it_shadow_traced++;
                  it_share++;
                  RTC_LIGHT_VISITOR sv;
                  sv.distance = distance;
                  RTC_LIGHT_VISITOR_SET(sv);
                  Ray sray{ovx, ovy, ovz, lvx, lvy, lvz};
                  trace<CSG, WORLD, RTC_LIGHT_VISITOR, TRAV, BOX, MOTION, ROOTS>(S, recs, cull, sray, sv, it_overflow, trav_stack, member, stride, mo.disp, tm);
                  RTC_LIT_ADD(sv);
                }
              const double samples = static_cast<double>(n_samples);
              RTC_LIT_INTENSITY(samples);  // intensity_at
              lr_ = lr_ + (dr / samples) * RTC_INTENSITY(r);
              lg_ = lg_ + (dg / samples) * RTC_INTENSITY(g);
              lb_ = lb_ + (db / samples) * RTC_INTENSITY(b);
            }
            sr = sr + lr_;
            sg = sg + lg_;
            sb = sb + lb_;
            continue;
          }
        }
        const double* __restrict__ L = lights + 6ull * li;
        if constexpr (!SPOT) it_shadow_calls++;  // (SPOT: below, once the cone has said whether isShadowed is called)
        // isShadowed (world.zig:127-131) and lighting's point_to_light (material.zig:51) share this
        const double vx = L[0] - ovx, vy = L[1] - ovy, vz = L[2] - ovz;
        const double distance = __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
        double lvx = vx, lvy = vy, lvz = vz;
        if (distance != 0.0) {
          if (kSharedNormalize && __ballot(!shared_normalize_ok(vx, vy, vz, distance)) == 0ull) {
            shared_normalize(lvx, lvy, lvz, distance);
          } else {
            lvx = vx / distance;
            lvy = vy / distance;
            lvz = vz / distance;
          }
        }
        // With light_dot_normal < 0 (light behind the surface) lighting() returns `ambient` shadowed
        // or not (material.zig:62-73): that shadow ray cannot change the result either.
        const double light_dot_normal = (lvx * hx + lvy * hy) + lvz * hz;
        bool shadowed = false;
        RTC_SF_DECL;  // (SFILT: the transmittance of this light's shadow ray; (1, 1, 1) where none is traced)
        // (SPOT) the cone's factor f at c = -(point_to_light . axis).  f == 0: the light gives `ambient` alone - what a
        // shadowed point gets -, so isShadowed is not called: no count, no shadow ray.  li is wave-uniform (no cooperative
        // iterations here): the row is read through the constant address space at a readfirstlane index - scalar loads,
        // the rows being read-only while a launch runs - and nothing of it is staged in LDS.
        double spot_f = 1.0;
        if constexpr (SPOT) {
          typedef const __attribute__((address_space(4))) double ConstRow;
          ConstRow* C = (ConstRow*)spots.row + static_cast<size_t>(RTC_SPOT_ROW) * __builtin_amdgcn_readfirstlane(li);
          if (C[5] != 0.0) spot_f = rtc_spot_factor(-((lvx * C[0] + lvy * C[1]) + lvz * C[2]), C[3], C[4]);
          shadowed = spot_f == 0.0;
          if (!shadowed) it_shadow_calls++;
        }
        if (!shadowed && shadow_matters && light_dot_normal >= 0.0 && !(RTC_EXPERIMENT & 1)) {
          it_shadow_traced++;
          it_share++;
          RTC_LIGHT_VISITOR sv;
          sv.distance = distance;
          RTC_LIGHT_VISITOR_SET(sv);
          Ray sray{ovx, ovy, ovz, lvx, lvy, lvz};
          RTC_STAMP(3);
          RTC_COUNT(2);
          {
            RTC_HIST_BEGIN();
            trace<CSG, WORLD, RTC_LIGHT_VISITOR, TRAV, BOX, MOTION, ROOTS>(S, recs, cull, sray, sv, it_overflow, trav_stack, s_member, s_stride, mo.disp, tm);
            RTC_HIST_END(1);
          }
                RTC_STAMP(4);
          shadowed = RTC_LIGHT_BLOCKED(sv);
          RTC_SF_TAKE(sv);
        }
        // Material.lighting (material.zig:40-74)
        const double er = color.r * L[3], eg = color.g * L[4], eb = color.b * L[5];  // effective_color
        const double ka = RTC_KA(mat);
        double lr_ = er * ka, lg_ = eg * ka, lb_ = eb * ka;
        if (!shadowed) {
          double dr = 0.0, dg = 0.0, db = 0.0, pr = 0.0, pg = 0.0, pb = 0.0;
          if (light_dot_normal >= 0.0) {
            const double kd = mat.diffuse * light_dot_normal;
            dr = er * kd;
            dg = eg * kd;
            db = eb * kd;
            if constexpr (SPOT) {  // (the diffuse term scaled once it is formed; f == 1: the same bits)
              dr = dr * spot_f;
              dg = dg * spot_f;
              db = db * spot_f;
            }
            const double two_dot = 2.0 * light_dot_normal;  // point_to_light.reflect(normal)
            const double rx = lvx - hx * two_dot, ry = lvy - hy * two_dot, rz = lvz - hz * two_dot;
            const double reflect_dot_eye = ((-rx) * ex + (-ry) * ey) + (-rz) * ez;
            if (reflect_dot_eye > 0.0) {
              const uint32_t n = mat.shininess_int;
              // (specular_skip) a lane whose material has no specular term keeps ks = specular, the zero itself: for
              // 0 < x <= 1 pow_small_int's squaring loop yields a finite value >= +0, and (+-0) * that is +-0 with
              // specular's sign.  zig_pow's path (n == 0: it can overflow, and 0 * inf is a NaN) and x > 1 stay as they
              // were.  The power is a loop, so the wave branches around it when no lane needs it.
              // (written nested on purpose: the compiler flattens it to the one-line form's three compares, but lays the kernel out
              // differently, and a world without such a material - cubes.json - keeps the parent's time: profiles/HISTORY.md)
              bool ks_is_specular = false;
              if (mat.specular == 0.0) ks_is_specular = n != 0u && reflect_dot_eye <= 1.0;
#ifdef RTC_PROFILE
              {  // (diagnostic builds: wave executions of the power by light, those no lane needs, and the lanes inside them;
                 // two 32-bit counts a word: good for one launch's counts - under 2^32 lanes -, not for sums over many)
                const unsigned long long lanes_ = static_cast<unsigned long long>(__builtin_popcountll(__ballot(true)));
                const unsigned long long idle_ = __ballot(!ks_is_specular) == 0ull ? 1ull : 0ull;
                RTC_AUX_ADD(li != 0u ? 1 : 0, 1ull + (idle_ << 32));
                RTC_AUX_ADD(li != 0u ? 3 : 2, lanes_ + ((idle_ * lanes_) << 32));
              }
#endif
              double ks = mat.specular;
              if (!(kSpecularSkip && ks_is_specular))
                ks = mat.specular * (n != 0u && reflect_dot_eye < kInf ? pow_small_int(reflect_dot_eye, n)
                                                                       : zig_pow(reflect_dot_eye, mat.shininess));
              pr = L[3] * ks;
              pg = L[4] * ks;
              pb = L[5] * ks;
              if constexpr (SPOT) {  // (... and the specular term)
                pr = pr * spot_f;
                pg = pg * spot_f;
                pb = pb * spot_f;
              }
            }
          }
          // (SFILT: both terms times the transmittance, after the spot factor; (1, 1, 1): the same bits)
          lr_ = (lr_ + RTC_SF(dr, r)) + RTC_SF(pr, r);
          lg_ = (lg_ + RTC_SF(dg, g)) + RTC_SF(pg, g);
          lb_ = (lb_ + RTC_SF(db, b)) + RTC_SF(pb, b);
        }
        sr = sr + lr_;
        sg = sg + lg_;
        sb = sb + lb_;
      }
#ifdef RTC_ENV_TU
      // (ENV, rtc.h's rtc_scene_set_environment) the suns, after World.lights and in table order: a point light in
      // everything but its geometry.  point_to_light is the row's unit vector whatever the point, the distance is
      // infinite: every entry with et >= 0 on a casts_shadow leaf counts (SunVisitor: FilterVisitor with an infinite limit
      // - not an any-hit walk, so no early-out that reasons about a segment's far end is compiled in; DESIGN.md section 24
      // lists what was read).  No cone, no area row.  si is wave-uniform: the row is read through the constant address space at a
      // readfirstlane index - scalar loads, as DevSpots' rows are -, and nothing of it is staged in LDS.
#ifndef RTC_SKYL_TU
      if constexpr (ENV) {
        for (uint32_t si = 0u; si < env.n_suns; ++si) {
          typedef const __attribute__((address_space(4))) double ConstRow;
          ConstRow* U = (ConstRow*)env.sun + static_cast<size_t>(RTC_ENV_SUN_ROW) * __builtin_amdgcn_readfirstlane(si);
          const double lvx = U[0], lvy = U[1], lvz = U[2];
          const double ir = U[3], ig = U[4], ib = U[5];
          it_shadow_calls++;
          const double light_dot_normal = (lvx * hx + lvy * hy) + lvz * hz;
          bool shadowed = false;
          RTC_SF_DECL;
          if (shadow_matters && light_dot_normal >= 0.0) {
            it_shadow_traced++;
            it_share++;
            SunVisitor sv;
            sv.distance = kInf;
            RTC_LIGHT_VISITOR_SET(sv);
            Ray sray{ovx, ovy, ovz, lvx, lvy, lvz};
            trace<CSG, WORLD, SunVisitor, TRAV, BOX, MOTION, ROOTS>(S, recs, cull, sray, sv, it_overflow, trav_stack, member, stride, mo.disp, tm);
            shadowed = RTC_LIGHT_BLOCKED(sv);
            RTC_SF_TAKE(sv);
          }
          // Material.lighting (material.zig:40-74) with the sun's intensity
          const double er = color.r * ir, eg = color.g * ig, eb = color.b * ib;  // effective_color
          const double ka = RTC_KA(mat);
          double lr_ = er * ka, lg_ = eg * ka, lb_ = eb * ka;
          if (!shadowed) {
            double dr = 0.0, dg = 0.0, db = 0.0, pr = 0.0, pg = 0.0, pb = 0.0;
            if (light_dot_normal >= 0.0) {
              const double kd = mat.diffuse * light_dot_normal;
              dr = er * kd;
              dg = eg * kd;
              db = eb * kd;
              const double two_dot = 2.0 * light_dot_normal;  // point_to_light.reflect(normal)
              const double rx = lvx - hx * two_dot, ry = lvy - hy * two_dot, rz = lvz - hz * two_dot;
              const double reflect_dot_eye = ((-rx) * ex + (-ry) * ey) + (-rz) * ez;
              if (reflect_dot_eye > 0.0) {
                const uint32_t n = mat.shininess_int;
                // (specular_skip, as in the loop above: a material without a specular term keeps the zero itself)
                bool ks_is_specular = false;
                if (mat.specular == 0.0) ks_is_specular = n != 0u && reflect_dot_eye <= 1.0;
                double ks = mat.specular;
                if (!(kSpecularSkip && ks_is_specular))
                  ks = mat.specular * (n != 0u && reflect_dot_eye < kInf ? pow_small_int(reflect_dot_eye, n)
                                                                         : zig_pow(reflect_dot_eye, mat.shininess));
                pr = ir * ks;
                pg = ig * ks;
                pb = ib * ks;
              }
            }
            lr_ = (lr_ + RTC_SF(dr, r)) + RTC_SF(pr, r);
            lg_ = (lg_ + RTC_SF(dg, g)) + RTC_SF(pg, g);
            lb_ = (lb_ + RTC_SF(db, b)) + RTC_SF(pb, b);
          }
          sr = sr + lr_;
          sg = sg + lg_;
          sb = sb + lb_;
        }
      }
#else
      // (SKYL, rtc.h's rtc_scene_set_sky_light) in the sky-light unit the suns' loop goes on after the last sun for the sky
      // light's samples, so that both kinds of ray without a far end share ONE inlined walk: a second call site of
      // trace<SunVisitor> made the flag alone cost cover + 27 % and teapot + 19 %.  Whether an iteration
      // is a sun's or a sample's is wave-uniform; a sun's part is the loop's of the environment unit, statement for statement.
      // A sample, at a hit of a material with a diffuse term: a direction of the geometric normal's hemisphere - the
      // occlusion step's rule and word, from this table's key: nx, ny, nz is ng after its inside flip, not the bumped hx,
      // hy, hz -, walked from over_point as a sun's shadow ray is, so the filter rows multiply and the early-outs are the ones
      // section 24 read; a direction that is not blocked looks the sky up as a miss does, through the out-of-line
      // pattern_at_shared.  Across the walk live L and the sample's hash; the mean is added after the last iteration: after
      // the last sun's term.
      if constexpr (SKYL) {
        const uint32_t n_sky = (skyl.gain > 0.0 && env.sky != 0u) ? skyl.samples : 0u;  // (wave-uniform)
        const bool sky_lane = n_sky != 0u && mat.diffuse != 0.0;
        unsigned long long skyl_h = 0ull;
        if (sky_lane) {
          uint32_t kpx, kpy;
          map_pixel(map, out_index, kpx, kpy);
          skyl_h = rtc_gloss_sample_key(RTC_DKEY(skyl.key), static_cast<unsigned long long>(kpy) * cam.hsize + kpx,
                                        static_cast<unsigned long long>(smp.sample_base) + (*samp_word & RTC_SAMPLE_MASK));
        }
        double l_r = 0.0, l_g = 0.0, l_b = 0.0;
#ifdef RTC_EMIT_TU
        // (EMIT, rtc.h's rtc_scene_set_emitters) in the emitter unit the loop goes on once more, after the last sky-light
        // sample, for the emitter samples: a third kind of iteration of the ONE inlined walk, wave-uniform as the other two.
        // A lane draws where it will form a diffuse child - the conditions of the children's section below, with
        // cur.remaining's, which that section has behind it -: the entry by the CDF (a binary search on global memory, per
        // lane), the point on its parallelogram, then the walk to it with a far end (EmitVisitor::bounded).  Across the walk
        // live the sample's factor per channel and the distance; the mean is added after the sky light's.
        const uint32_t n_emit = (EMIT && emit.count != 0u && indir.gain > 0.0 && indir.bounces != 0u) ? emit.samples : 0u;  // (wave-uniform)
        const bool emit_lane = n_emit != 0u && mat.diffuse != 0.0 && cur.remaining > 0u && (cur.lin & RTC_LIN_D) < indir.bounces;
        unsigned long long emit_h = 0ull;
        if (emit_lane) {
          uint32_t mpx, mpy;
          map_pixel(map, out_index, mpx, mpy);
          emit_h = rtc_gloss_sample_key(RTC_DKEY(emit.key), static_cast<unsigned long long>(mpy) * cam.hsize + mpx,
                                        static_cast<unsigned long long>(smp.sample_base) + (*samp_word & RTC_SAMPLE_MASK));
        }
        double m_r = 0.0, m_g = 0.0, m_b = 0.0;
        const uint32_t n_rays = (env.n_suns + n_sky) + n_emit;
#else
        const uint32_t n_rays = env.n_suns + n_sky;
#endif
        for (uint32_t si = 0u; si < n_rays; ++si) {
          const bool is_sun = si < env.n_suns;
          double lvx = 0.0, lvy = 0.0, lvz = 0.0, ir = 0.0, ig = 0.0, ib = 0.0, light_dot_normal = 0.0;
          bool walk = false;
#ifdef RTC_EMIT_TU
          const bool is_emit = si >= env.n_suns + n_sky;
          double far_end = kInf, emit_r = 0.0;
          if (is_emit) {
            if (emit_lane) {
              const uint32_t word = ((si - (env.n_suns + n_sky)) << RTC_OCCLUSION_SAMPLE_SHIFT) | cur.code;
              const double u0 = rtc_gloss_jitter(emit_h, word, 0u);
              double eu = rtc_gloss_jitter(emit_h, word, 1u);
              double ev = rtc_gloss_jitter(emit_h, word, 2u);
              // (the first k with cdf[k] > u0 * W, the last entry at the most)
              const uint32_t entry = rtc_emitter_pick(emit.cdf, emit.count, u0 * emit.total);
              const double* __restrict__ R = emit.row + static_cast<size_t>(RTC_EMITTER_ROW) * entry;
              if (R[16] != 0.0 && eu + ev > 1.0) {  // (a triangle: the other half of the parallelogram folds back)
                eu = 1.0 - eu;
                ev = 1.0 - ev;
              }
              const double yx = (R[0] + eu * R[3]) + ev * R[6];
              const double yy = (R[1] + eu * R[4]) + ev * R[7];
              const double yz = (R[2] + eu * R[5]) + ev * R[8];
              const double vx = yx - ovx, vy = yy - ovy, vz = yz - ovz;
              const double r2 = (vx * vx + vy * vy) + vz * vz;
              const double r = __builtin_sqrt(r2);
              lvx = vx / r, lvy = vy / r, lvz = vz / r;
              const double cos_x = (nx * lvx + ny * lvy) + nz * lvz;
              const double cos_e = __builtin_fabs((R[9] * lvx + R[10] * lvy) + R[11] * lvz);
              walk = !(cos_x <= 0.0) && !(cos_e == 0.0) && !(r <= 2e-4);
              if (walk) {
                far_end = r - 1e-4;
                // (the term but for the filter, per channel: E.c * (W / sum E) * ((cos_x * cos_e) / (pi * r2)))
                const double geo = (cos_x * cos_e) / (RTC_PI * r2);
                ir = (R[12] * R[15]) * geo;
                ig = (R[13] * R[15]) * geo;
                ib = (R[14] * R[15]) * geo;
#ifdef RTC_MIS_TU
                // (MIS, mode 1) the balance heuristic's weight of the sample, w_e = n * pi * r2 / (n * pi * r2 + q * cos_x *
                // cos_e): the term but for the filter, times w_e
                if constexpr (MIS) {
                  if (mis.mode != 0u) {
                    double w_e, w_b;
                    rtc_mis_weights(static_cast<double>(emit.samples), R[15], cos_x, cos_e, r2, w_e, w_b);
                    ir = ir * w_e;
                    ig = ig * w_e;
                    ib = ib * w_e;
                  }
                }
#endif
                emit_r = r;
                it_shadow_calls++;
              }
            }
          } else
#endif
          if (is_sun) {
            typedef const __attribute__((address_space(4))) double ConstRow;
            ConstRow* U = (ConstRow*)env.sun + static_cast<size_t>(RTC_ENV_SUN_ROW) * __builtin_amdgcn_readfirstlane(si);
            lvx = U[0], lvy = U[1], lvz = U[2];
            ir = U[3], ig = U[4], ib = U[5];
            it_shadow_calls++;
            light_dot_normal = (lvx * hx + lvy * hy) + lvz * hz;
            walk = shadow_matters && light_dot_normal >= 0.0;
          } else if (sky_lane) {
            const GlossDir sd = occl_direction(skyl_h, ((si - env.n_suns) << RTC_OCCLUSION_SAMPLE_SHIFT) | cur.code, nx, ny, nz);
            lvx = sd.x, lvy = sd.y, lvz = sd.z;
            it_shadow_calls++;
            walk = true;
          }
          bool shadowed = false;
          RTC_SF_DECL;
          if (walk) {
            it_shadow_traced++;
            it_share++;
#ifdef RTC_EMIT_TU
            EmitVisitor sv;
            sv.distance = far_end;  // (+infinity but for an emitter sample)
            sv.bounded = is_emit;
#else
            SunVisitor sv;
            sv.distance = kInf;
#endif
            RTC_LIGHT_VISITOR_SET(sv);
            Ray sray{ovx, ovy, ovz, lvx, lvy, lvz};
#ifdef RTC_EMIT_TU
            trace<CSG, WORLD, EmitVisitor, TRAV, BOX, MOTION, ROOTS>(S, recs, cull, sray, sv, it_overflow, trav_stack, member, stride, mo.disp, tm);
#else
            trace<CSG, WORLD, SunVisitor, TRAV, BOX, MOTION, ROOTS>(S, recs, cull, sray, sv, it_overflow, trav_stack, member, stride, mo.disp, tm);
#endif
            shadowed = RTC_LIGHT_BLOCKED(sv);
            RTC_SF_TAKE(sv);
          }
#ifdef RTC_EMIT_TU
          if (is_emit) {
            if (walk && !shadowed) {
              // (MEDIA: times the transmittance of a segment of length r in the ray's medium; the attenuation alone)
              double a_r = media.fog_density, a_g = media.fog_density, a_b = media.fog_density;
              if (cur.medium != RTC_NO_MEDIUM) {
                const double* __restrict__ A = media.absorption + 3ull * cur.medium;
                a_r = A[0];
                a_g = A[1];
                a_b = A[2];
              }
              double t_r = RTC_SF(ir, r), t_g = RTC_SF(ig, g), t_b = RTC_SF(ib, b);
              if (a_r != 0.0) t_r = t_r * exp(-(a_r * emit_r));
              if (a_g != 0.0) t_g = t_g * exp(-(a_g * emit_r));
              if (a_b != 0.0) t_b = t_b * exp(-(a_b * emit_r));
              m_r = m_r + t_r;
              m_g = m_g + t_g;
              m_b = m_b + t_b;
            }
          } else
#endif
          if (is_sun) {
            // Material.lighting (material.zig:40-74) with the sun's intensity
            const double er = color.r * ir, eg = color.g * ig, eb = color.b * ib;  // effective_color
            const double ka = RTC_KA(mat);
            double lr_ = er * ka, lg_ = eg * ka, lb_ = eb * ka;
            if (!shadowed) {
              double dr = 0.0, dg = 0.0, db = 0.0, pr = 0.0, pg = 0.0, pb = 0.0;
              if (light_dot_normal >= 0.0) {
                const double kd = mat.diffuse * light_dot_normal;
                dr = er * kd;
                dg = eg * kd;
                db = eb * kd;
                const double two_dot = 2.0 * light_dot_normal;  // point_to_light.reflect(normal)
                const double rx = lvx - hx * two_dot, ry = lvy - hy * two_dot, rz = lvz - hz * two_dot;
                const double reflect_dot_eye = ((-rx) * ex + (-ry) * ey) + (-rz) * ez;
                if (reflect_dot_eye > 0.0) {
                  const uint32_t n = mat.shininess_int;
                  bool ks_is_specular = false;
                  if (mat.specular == 0.0) ks_is_specular = n != 0u && reflect_dot_eye <= 1.0;
                  double ks = mat.specular;
                  if (!(kSpecularSkip && ks_is_specular))
                    ks = mat.specular * (n != 0u && reflect_dot_eye < kInf ? pow_small_int(reflect_dot_eye, n)
                                                                           : zig_pow(reflect_dot_eye, mat.shininess));
                  pr = ir * ks;
                  pg = ig * ks;
                  pb = ib * ks;
                }
              }
              lr_ = (lr_ + RTC_SF(dr, r)) + RTC_SF(pr, r);
              lg_ = (lg_ + RTC_SF(dg, g)) + RTC_SF(pg, g);
              lb_ = (lb_ + RTC_SF(db, b)) + RTC_SF(pb, b);
            }
            sr = sr + lr_;
            sg = sg + lg_;
            sb = sb + lb_;
          } else if (walk && !shadowed) {
            double e_r = env.rgb[0], e_g = env.rgb[1], e_b = env.rgb[2];
            if (env.pattern != RTC_ENV_NO_PATTERN) {
              const double len = env.projection == RTC_ENV_CUBE
                                     ? __builtin_fmax(__builtin_fabs(lvx), __builtin_fmax(__builtin_fabs(lvy), __builtin_fabs(lvz)))
                                     : __builtin_sqrt((lvx * lvx + lvy * lvy) + lvz * lvz);
              const MeshUvHit sky_mh{muv.row, RTC_NO_LEAF, 0.0, 0.0};
              const Rgb c = pattern_at_shared(S, pats, env.pattern, lvx / len, lvy / len, lvz / len, sky_mh);
              e_r = c.r * e_r;
              e_g = c.g * e_g;
              e_b = c.b * e_b;
            }
            l_r = l_r + RTC_SF(e_r, r);
            l_g = l_g + RTC_SF(e_g, g);
            l_b = l_b + RTC_SF(e_b, b);
          }
        }
        if (sky_lane) {
          const double n_mean = static_cast<double>(skyl.samples);
          sr = sr + (color.r * mat.diffuse) * (skyl.gain * (l_r / n_mean));
          sg = sg + (color.g * mat.diffuse) * (skyl.gain * (l_g / n_mean));
          sb = sb + (color.b * mat.diffuse) * (skyl.gain * (l_b / n_mean));
        }
#ifdef RTC_EMIT_TU
        if (emit_lane) {  // (EMIT) the emitter samples' mean, after the sky light's and before the emission row
          const double n_mean = static_cast<double>(emit.samples);
          sr = sr + (color.r * mat.diffuse) * (indir.gain * (m_r / n_mean));
          sg = sg + (color.g * mat.diffuse) * (indir.gain * (m_g / n_mean));
          sb = sb + (color.b * mat.diffuse) * (indir.gain * (m_b / n_mean));
        }
#endif
      }
#endif
#endif
#ifdef RTC_INDIR_TU
      // (INDIRECT, rtc.h's rtc_scene_set_indirect) the material's emission row, after the last light's, sun's and sky-light
      // term and before the ray's weight; a handle without rows has a null pointer (wave-uniform)
      if constexpr (INDIRECT) {
#ifdef RTC_EMIT_TU
        // (EMIT) nothing counted twice: the ray formed as a diffuse child adds no emission at a leaf of the emitter list -
        // its parent's samples counted it.  Only such a ray reads the leaf's bit.
        bool emits_here = indir.emission != nullptr;
#ifdef RTC_MIS_TU
        // (MIS, mode 1) the ray formed as a diffuse child adds a listed leaf's emission times w_b = a / (b + a), a = q *
        // (cos_b * cos_e'), b = n * (pi * t * t): the direction's weight under the balance heuristic, whose other half its
        // parent's samples took.  cos_e' is against the flat normal the list stores for the face hit - the leaf's word names
        // its first entry and its faces; a cube's face is the reference's rule for cube normals on the object-space point,
        // formed again here from the hit's own transform: nothing of it is live across the lights' loop.  (A listed leaf's
        // root does not move: the point needs no displacement.)  A face the list leaves out, cos_b <= 0, cos_e' == 0 and
        // t <= 2e-4 - where a sample would have been zero - keep the whole row.  Only such a ray reads the word and the row.
        double mis_wb = 1.0;
        if constexpr (MIS) {
          if (mis.mode != 0u && emits_here && emit.count != 0u && (cur.lin & RTC_LIN_DIFFUSE) != 0u) {
            const uint32_t lw = mis.leaf_entry[hv.leaf];
            if (lw != 0u) {
              const double* __restrict__ Mh;
              uint32_t kh;
              if (hv.root != RTC_NO_LEAF) {
                const RootRec& Rh = recs[RTC_CHECK_INDEX(RTC_OOB_ROOTS, hv.root, RTC_AVAIL(0))];
                Mh = Rh.inv;
                kh = Rh.kind_flags & 0xFFu;
              } else {
                const uint4 meta = S.leaf_meta[hv.leaf];
                Mh = S.xf + 12ull * meta.y;
                kh = meta.x & 0xFFu;
              }
              uint32_t face = 0u;
              if (kh == 2u) {  // cube.zig:81-97: the axis of the largest |coordinate|, x before y before z
                const double fx = row_pt(Mh + 0, ptx, pty, ptz), fy = row_pt(Mh + 4, ptx, pty, ptz), fz = row_pt(Mh + 8, ptx, pty, ptz);
                const double ax = __builtin_fabs(fx), ay = __builtin_fabs(fy), az = __builtin_fabs(fz);
                const double maxc = zmax(ax, zmax(ay, az));
                if (maxc == ax) face = fx < 0.0 ? 1u : 0u;
                else if (maxc == ay) face = fy < 0.0 ? 3u : 2u;
                else face = fz < 0.0 ? 5u : 4u;
              }
              const uint32_t mask = lw >> RTC_MIS_FACE_SHIFT;
              if (((mask >> face) & 1u) != 0u) {
                const uint32_t entry = (lw & 0xFFFFu) + static_cast<uint32_t>(__builtin_popcount(mask & ((1u << face) - 1u)));
                const double* __restrict__ R = emit.row + static_cast<size_t>(RTC_EMITTER_ROW) * entry;
                const double cos_e = __builtin_fabs((R[9] * ray.dx + R[10] * ray.dy) + R[11] * ray.dz);
                if (!(cur.cosb <= 0.0) && !(cos_e == 0.0) && !(t <= 2e-4)) {
                  double w_e;
                  rtc_mis_weights(static_cast<double>(emit.samples), R[15], cur.cosb, cos_e, t * t, w_e, mis_wb);
                }
              }
            }
          }
        }
#endif
        if constexpr (EMIT) {
          if (emits_here && emit.count != 0u && (cur.lin & RTC_LIN_DIFFUSE) != 0u)
#ifdef RTC_MIS_TU
            if (!(MIS && mis.mode != 0u))  // (mode 0: the emitter kernels' rule)
#endif
            emits_here =((emit.leaf_bits[hv.leaf >> 5] >> (hv.leaf & 31u)) & 1u) == 0u;
        }
        if (emits_here) {
#else
        if (indir.emission != nullptr) {
#endif
          const double* __restrict__ EM = indir.emission + 3ull * mat_index;
#ifdef RTC_MIS_TU
          sr = sr + EM[0] * mis_wb;
          sg = sg + EM[1] * mis_wb;
          sb = sb + EM[2] * mis_wb;
#else
          sr = sr + EM[0];
          sg = sg + EM[1];
          sb = sb + EM[2];
#endif
        }
        ind_r = color.r * mat.diffuse;
        ind_g = color.g * mat.diffuse;
        ind_b = color.b * mat.diffuse;
      }
#endif
      if constexpr (COOP) {
        if (deal_lights) {  // the other half's light (lane i <-> 7 - i pairs the halves), and what it counted
          sr = sr + group8_other<2>(sr);
          sg = sg + group8_other<2>(sg);
          sb = sb + group8_other<2>(sb);
          it_shadow_calls += group8_other<2>(it_shadow_calls - calls_before);
          it_shadow_traced += group8_other<2>(it_shadow_traced - traced_before);
          it_share += group8_other<2>(it_share - share_before);
        }
      }
    }
    if constexpr (COOP) {
      yield.contrib[0] = cur.weight * sr;
      yield.contrib[1] = cur.weight * sg;
      yield.contrib[2] = cur.weight * sb;
    } else {
      acc[0] += cur.weight * sr;
      acc[1] += RTC_W(cur, g) * sg;
      acc[2] += RTC_W(cur, b) * sb;
    }

    RTC_STAMP(6);
    // ---- reflectedColor / refractedColor / schlick (world.zig:98-107, 157-189, 272-289)
    if (cur.remaining == 0u) continue;
    const DevMaterial& mat = mats[mat_index];
    const bool do_reflect = !(mat.reflective == 0.0);
    const bool transparent = !(mat.transparency == 0.0);
#ifdef RTC_INDIR_TU
    // (INDIRECT) the diffuse child's conditions; cur.remaining > 0 holds here
    const bool do_diffuse = INDIRECT && indir.gain > 0.0 && mat.diffuse != 0.0 && (cur.lin & RTC_LIN_D) < indir.bounces;
    if (!do_reflect && !transparent && !do_diffuse) continue;
#else
    if (!do_reflect && !transparent) continue;
#endif

    const double cos_i = (ex * hx + ey * hy) + ez * hz;  // eyev.dot(normal)
    double w_reflect = mat.reflective, w_refract = mat.transparency;
    bool do_refract = false;
    double n_ratio = 1.0, sin2_t = 0.0;
    if (transparent) {
      n_ratio = n1 / n2;
      sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
      do_refract = !(sin2_t > 1.0);
      if (mat.reflective > 0.0 && mat.transparency > 0.0) {  // schlick, world.zig:272-289
        double reflectance;
        double c = cos_i;
        bool tir = false;
        if (n1 > n2) {
          const double nr = n1 / n2;
          const double s2 = nr * nr * (1.0 - c * c);
          if (s2 > 1.0) {
            tir = true;
          } else {
            c = __builtin_sqrt(1.0 - s2);
          }
        }
        if (tir) {
          reflectance = 1.0;
        } else {
          const double frac = (n1 - n2) / (n1 + n2);
          const double r0 = frac * frac;
          reflectance = r0 + (1.0 - r0) * zig_pow(1.0 - c, 5.0);
        }
        w_reflect = mat.reflective * reflectance;
        w_refract = mat.transparency * (1.0 - reflectance);
      }
    }
    RTC_STAMP(13);
    Pending child;
    child.remaining = cur.remaining - 1u;
#ifdef RTC_GLOSS_TU
    // (GLOSS) the material's roughness pair, read per lane as the bump row is (mat_index is the lane's); a lane whose
    // children are both smooth hashes nothing and leaves the directions' bits.  The hash of the ray's camera sample: the
    // whole-image pixel and the global sample index, as the shutter time's.
    double rough_r = 0.0, rough_t = 0.0;
    unsigned long long gloss_h = 0ull;
    if constexpr (GLOSS) {
      const double* __restrict__ G = gloss.row + static_cast<size_t>(RTC_GLOSS_ROW) * mat_index;
      if (do_reflect) rough_r = G[0];
      if (do_refract) rough_t = G[1];
      if (rough_r > 0.0 || rough_t > 0.0) {
        uint32_t px, py;
        map_pixel(map, out_index, px, py);
        const unsigned long long p = static_cast<unsigned long long>(py) * cam.hsize + px;
        gloss_h = rtc_gloss_sample_key(RTC_DKEY(gloss.key), p, static_cast<unsigned long long>(smp.sample_base) + (*samp_word & RTC_SAMPLE_MASK));
      }
    }
#endif
#ifdef RTC_INDIR_TU
    // (INDIRECT) the diffuse child: from over_point along a direction of ng's hemisphere - the occlusion step's rule, from
    // this table's key at word (d << shift) | code -, in its parent's medium, with the reflected child's path code.  It is
    // formed first and, where a reflected or refracted child follows, waits on the stack below the refraction: a hit pushes
    // at most two (ensureScratch sizes the indirect family's stack by that).  Alone it continues in registers.
    if constexpr (INDIRECT) {
      if (do_diffuse) {
        uint32_t ipx, ipy;
        map_pixel(map, out_index, ipx, ipy);
        const unsigned long long ind_h = rtc_gloss_sample_key(RTC_DKEY(indir.key), static_cast<unsigned long long>(ipy) * cam.hsize + ipx,
                                                              static_cast<unsigned long long>(smp.sample_base) + (*samp_word & RTC_SAMPLE_MASK));
        const uint32_t d = cur.lin & RTC_LIN_D;
        const GlossDir dd = occl_direction(ind_h, (d << RTC_OCCLUSION_SAMPLE_SHIFT) | cur.code, nx, ny, nz);
        Pending q;
        q.ray = {ovx, ovy, ovz, dd.x, dd.y, dd.z};
        q.weight = cur.weight * (ind_r * indir.gain);
        q.weight_g = cur.weight_g * (ind_g * indir.gain);
        q.weight_b = cur.weight_b * (ind_b * indir.gain);
        q.medium = cur.medium;
        q.remaining = cur.remaining - 1u;
        q.code = 2u * cur.code;
        q.lin = (d + 1u) | RTC_LIN_DIFFUSE;
#ifdef RTC_MIS_TU
        q.cosb = (dd.x * nx + dd.y * ny) + dd.z * nz;  // (MIS) cos_b: the direction against the normal it was drawn about
#endif
        it_secondary++;
        if (do_reflect || do_refract) {
          if (sp < stack_cap) {
            RTC_MEDIA_PUSH_EXTRA(sp, q);
            push_level(sp++, q);
          } else {
            overflow = CSG ? (overflow | 1u) : 1u;
          }
        } else {
          cur = q;
          have_cur = true;
        }
      }
    }
#endif
    if (do_reflect) {
      const double two_dot = 2.0 * ((ray.dx * hx + ray.dy * hy) + ray.dz * hz);  // direction.reflect(normal)
      child.ray = {ovx, ovy, ovz, ray.dx - hx * two_dot, ray.dy - hy * two_dot, ray.dz - hz * two_dot};
      child.weight = cur.weight * w_reflect;
      RTC_MEDIA_KID(child, cur, w_reflect, cur.medium);  // (MEDIA: a reflected child stays in its parent's medium)
      RTC_SET_CODE(child, 2u * cur.code);
      RTC_SET_LIN(child, cur.lin & RTC_LIN_D);  // (INDIRECT: its parent's d; not a diffuse child)
#ifdef RTC_MIS_TU
      child.cosb = 0.0;
#endif
#ifdef RTC_GLOSS_TU
      if (rough_r > 0.0) {
        const GlossDir g = gloss_scatter(gloss_h, child.code, rough_r, child.ray.dx, child.ray.dy, child.ray.dz, nx, ny, nz, false);
        child.ray.dx = g.x;
        child.ray.dy = g.y;
        child.ray.dz = g.z;
      }
#endif
      it_secondary++;
    }
    if (do_refract) {
      const double cos_t = __builtin_sqrt(1.0 - sin2_t);
      const double k = n_ratio * cos_i - cos_t;
      const double unx = ptx - nx * eps, uny = pty - ny * eps, unz = ptz - nz * eps;  // under_point
      Pending p;
      p.ray = {unx, uny, unz, hx * k - ex * n_ratio, hy * k - ey * n_ratio, hz * k - ez * n_ratio};
      p.weight = cur.weight * w_refract;
      RTC_MEDIA_KID(p, cur, w_refract, kid_medium);
      p.remaining = cur.remaining - 1u;
      RTC_SET_CODE(p, 2u * cur.code + 1u);
      RTC_SET_LIN(p, cur.lin & RTC_LIN_D);
#ifdef RTC_MIS_TU
      p.cosb = 0.0;
#endif
#ifdef RTC_GLOSS_TU
      if (rough_t > 0.0) {
        const GlossDir g = gloss_scatter(gloss_h, p.code, rough_t, p.ray.dx, p.ray.dy, p.ray.dz, nx, ny, nz, true);
        p.ray.dx = g.x;
        p.ray.dy = g.y;
        p.ray.dz = g.z;
      }
#endif
      it_secondary++;
      if (do_reflect) {  // both children: the reflection continues in registers, the refraction waits
        if constexpr (COOP) {
          yield.kid_later = p;
          yield.n_kids = 1u;
        } else {
          if (sp < stack_cap) {
            RTC_MEDIA_PUSH_EXTRA(sp, p);
            push_level(sp++, p);
          } else {
            overflow = CSG ? (overflow | 1u) : 1u;
          }
        }
      } else {
        child = p;
      }
    }
    if (do_reflect || do_refract) {
      if constexpr (COOP) {
        yield.kid_now = child;
        yield.n_kids += 1u;
      } else {
        cur = child;
        have_cur = true;
      }
    }
    } while (0);
    // ---- 4. (COOP kernels) what the iteration yielded, applied by the lane that owns the pixel: its own yield, or - after
    // a cooperative iteration - that of the first lane of the group that worked on its ray
    if constexpr (COOP) {
      if (coop) {
        const int from = static_cast<int>(yield_from);
        Yield y;
#pragma unroll
        for (int i = 0; i < 3; ++i) y.contrib[i] = __shfl(yield.contrib[i], from);
        auto fetch = [&](const Pending& k) {
          Pending r;
          r.ray = {__shfl(k.ray.ox, from), __shfl(k.ray.oy, from), __shfl(k.ray.oz, from),
                   __shfl(k.ray.dx, from), __shfl(k.ray.dy, from), __shfl(k.ray.dz, from)};
          r.weight = __shfl(k.weight, from);
          r.remaining = __shfl(k.remaining, from);
          return r;
        };
        y.kid_now = fetch(yield.kid_now);
        y.kid_later = fetch(yield.kid_later);
        y.n_kids = __shfl(yield.n_kids, from);
        y.share = __shfl(yield.share, from);
        y.secondary = __shfl(yield.secondary, from);
        y.shadow_calls = __shfl(yield.shadow_calls, from);
        y.shadow_traced = __shfl(yield.shadow_traced, from);
        y.overflow = __shfl(yield.overflow, from);
        yield = y;
      }
      if (owner) {
        acc[0] += yield.contrib[0];
        acc[1] += yield.contrib[1];
        acc[2] += yield.contrib[2];
        share_rays += yield.share;
        n_secondary += yield.secondary;
        n_shadow_calls += yield.shadow_calls;
        n_shadow_traced += yield.shadow_traced;
        overflow |= yield.overflow;
        if (yield.n_kids == 2u) {  // the reflection continues in registers, the refraction waits
          if (sp < stack_cap) {
            push_level(sp++, yield.kid_later);
          } else {
            overflow = CSG ? (overflow | 1u) : 1u;
          }
        }
        if (yield.n_kids != 0u) {
          cur = yield.kid_now;
          have_cur = true;
        }
      }
    }
  }

  if (map.packet_time != nullptr && pk_cur != RTC_NO_ITEM && lane == 0u)
    map.packet_time[pk_cur] = static_cast<uint32_t>((__builtin_amdgcn_s_memtime() - pk_t0) >> 4);
#ifdef RTC_PROFILE
  RTC_STAMP(7);
  prof_acc[7] = prof_iters;  // slot 7 reports main-loop iterations (wave-level), not cycles
  if (lane == 0u) {
    for (int i = 0; i < 16; ++i) atomicAdd(&stats->prof[i], prof_acc[i]);
    atomicMin(&stats->prof_t0, prof_t - prof_start);  // shortest / longest wave lifetime (s_memtime is
    atomicMax(&stats->prof_t1, ((prof_t - prof_start) << 24) | (prof_last_unit & 0xFFFFFFull));  // longest wave + its last unit
    atomicAdd(&stats->prof_busy, prof_t - prof_start);
    for (int i = 0; i < 8; ++i) atomicAdd(&stats->prof2[i], prof2[i]);
    for (int i = 0; i < 21; ++i) atomicAdd(&stats->prof3[i], prof3[i]);
#ifndef RTC_PROFILE_LITE
    for (int i = 0; i < 8; ++i) {
      atomicAdd(&stats->prof4[i], rtc_prof_counts[threadIdx.x >> 6][i]);
      atomicAdd(&stats->prof5[i], rtc_prof_counts[threadIdx.x >> 6][8 + i]);
    }
    for (int i = 0; i < 24; ++i) atomicAdd(&stats->prof6[i], rtc_prof_counts[threadIdx.x >> 6][16 + i]);
    for (int i = 0; i < 18; ++i) atomicAdd(&stats->prof7[i], rtc_prof_counts[threadIdx.x >> 6][40 + i]);
#endif
    const unsigned wid = (blockIdx.x * 4u + (threadIdx.x >> 6)) & 4095u;
    stats->prof_log[wid][0] = prof_t - prof_start;
    stats->prof_log[wid][1] = prof_iters;
    stats->prof_log[wid][2] = prof_units;
    stats->prof_log[wid][3] = (static_cast<unsigned long long>(prof_first_unit) << 32) | prof_last_unit;
    for (int i = 0; i < 16; ++i) stats->prof_last[wid][i] = prof_acc[i] - prof_snap[i];  // sections of the last packet
#ifdef RTC_PROFILE_LITE
    // (no sections in this mode: when the wave began, fetched its last packet and ended, by the 100 MHz clock all XCDs
    // share - s_memtime is a counter per XCD)
    stats->prof_last[wid][0] = prof_real0;
    stats->prof_last[wid][1] = __builtin_amdgcn_s_memrealtime();
    stats->prof_last[wid][2] = prof_real_fetch;
#endif
  }
#endif
  // The counters: summed over the wave, then over the work-group in LDS, one atomic per counter per work-group (each
  // counter in a cache line of its own, see DevStats).
  {
    __shared__ unsigned long long wg_sum[6];
    if (threadIdx.x < 6u) wg_sum[threadIdx.x] = 0ull;
    __syncthreads();  // (every wave of the group gets here: the loop above ends for all of them)
    const unsigned long long s_pri = wave_sum(n_primary), s_sec = wave_sum(n_secondary), s_shc = wave_sum(n_shadow_calls),
                             s_sht = wave_sum(n_shadow_traced), s_ovf = wave_sum(CSG ? (overflow != 0u ? 1u : 0u) : overflow), s_stolen = wave_sum(n_stolen);
    if constexpr (CSG)  // (only the *_ext kernels can have a csg list to run out of)
    if (__any((overflow >> 8) != 0u)) {  // a csg list ran out somewhere in the wave: what it needed (rare: straight to memory)
      unsigned need = overflow >> 8;
      for (int off = 32; off > 0; off >>= 1) need = max(need, static_cast<unsigned>(__shfl_xor(need, off, 64)));
      if (lane == 0u) atomicMax(&stats->csg_needed, need);
    }
    if (lane == 0u) {
      atomicAdd(&wg_sum[0], s_pri);
      atomicAdd(&wg_sum[1], s_sec);
      atomicAdd(&wg_sum[2], s_shc);
      atomicAdd(&wg_sum[3], s_sht);
      if (s_ovf) atomicAdd(&wg_sum[4], s_ovf);
      if (s_stolen) atomicAdd(&wg_sum[5], s_stolen);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
      atomicAdd(&stats->primary, wg_sum[0]);
      atomicAdd(&stats->secondary, wg_sum[1]);
      atomicAdd(&stats->shadow_calls, wg_sum[2]);
      atomicAdd(&stats->shadow_traced, wg_sum[3]);
      if (wg_sum[4]) atomicAdd(&stats->overflow, wg_sum[4]);
      if (wg_sum[5]) atomicAdd(&stats->stolen, static_cast<unsigned int>(wg_sum[5]));
    }
  }
}

// The kernels.  rtc_motion.hip includes this file with RTC_MOTION_TU defined and gets the motion kernels alone: a
// translation unit of their own, so that this one compiles in the time and to the code it did; rtc_spot.hip likewise
// with RTC_SPOT_TU and the spot kernels, rtc_bump.hip with RTC_BUMP_TU and the bump kernels, rtc_torus.hip with RTC_TORUS_TU
// and the torus kernels, rtc_meshuv.hip with RTC_MESHUV_TU (and, with it, RTC_TORUS_TU) and the meshuv kernels, rtc_gloss.hip
// with RTC_GLOSS_TU (and, with it, both of those) and the gloss kernels, rtc_occlusion.hip with RTC_OCCL_TU (and, with it, those
// three) and the occlusion kernels, rtc_shadowfilter.hip with RTC_SFILT_TU (and, with it, those four) and the shadow-filter
// kernels, rtc_media.hip with RTC_MEDIA_TU (and, with it, those five) and the media kernels, rtc_environment.hip with
// RTC_ENV_TU (and, with it, those six) and the environment kernels, rtc_skylight.hip with RTC_SKYL_TU (and, with it, those
// seven) and the sky-light kernels, rtc_indirect.hip with RTC_INDIR_TU (and, with it, those eight) and the indirect kernels,
// rtc_emitters.hip with RTC_EMIT_TU (and, with it, those nine) and the emitter kernels.
// rtc_kernels_ext.hip
// includes it with RTC_EXT_TU defined: in the -DRTC_PROFILE diagnostic build, whose instrumented walk makes this unit's
// compile about a third longer, it gets the csg / texture-map, flat and area-light kernels (rtc_render_kernel_ext to
// rtc_render_kernel_area_bigworld below), so that neither unit takes the time of all of them.  The product build keeps
// them here - that unit's code is the same as before to the byte - and its rtc_kernels_ext.o holds no kernel.
#if (defined(RTC_EXT_TU) && defined(RTC_PROFILE)) || (!defined(RTC_MOTION_TU) && !defined(RTC_SPOT_TU) && !defined(RTC_BUMP_TU) && !defined(RTC_TORUS_TU) && !defined(RTC_EXT_TU) && !defined(RTC_PROFILE))
#define RTC_EXT_KERNELS_HERE 1
#else
#define RTC_EXT_KERNELS_HERE 0
#endif
#if !defined(RTC_MOTION_TU) && !defined(RTC_SPOT_TU) && !defined(RTC_BUMP_TU) && !defined(RTC_TORUS_TU) && !defined(RTC_EXT_TU)
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                  double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, false>(S, cam, map, max_depth, out, stats, next_stats);
}

// Same kernel for worlds whose World.objects table does not fit the LDS staging area.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                           double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<false, false>(S, cam, map, max_depth, out, stats, next_stats);
}

// Worlds made of top-level spheres, planes and cubes only (cover, fresnel, reflection_and_refraction): nothing
// of the group traversal, the triangle / cylinder / cone tests or their normals is compiled in.  The code fits
// the instruction cache better: cover.json 1.035 -> 0.98 ms.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_simple(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                         double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, false, 2, 2, true, false>(S, cam, map, max_depth, out, stats, next_stats);
}

// ... and the same kernel with the root loop's first phase on world boxes: the simple worlds that are mostly cubes (trace()).
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_simple_b(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                           double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, false, 2, 2, true, true>(S, cam, map, max_depth, out, stats, next_stats);
}

// The `simple` kernel at THREE waves per SIMD (168 VGPRs; about a hundred values go to scratch memory, nearly all of them
// outside the loops that matter).  The vector pipes of a SIMD issue in 62 % of a cover frame's cycles at two waves
// (DESIGN.md section 5): the third wave fills part of the rest.  cover.json 1080p 0.696 -> 0.667 ms,
// reflection_and_refraction depth 8 2.22 -> 2.02.  Only this kernel gains (every other variant spills three times as
// much at 168 registers and loses), and only with several packets per wave: small images and one rank's share of a
// split frame are bound by single waves' chains of dependent iterations and run the two-wave kernel (rtc_capi.hip).
extern "C" __global__ void __launch_bounds__(256, 3)
rtc_render_kernel_simple3(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                          double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, false, 2, 3, false, false>(S, cam, map, max_depth, out, stats, next_stats);
}

extern "C" __global__ void __launch_bounds__(256, 3)
rtc_render_kernel_simple3_b(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                            double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, false, 2, 3, false, true>(S, cam, map, max_depth, out, stats, next_stats);
}

// The general kernel at THREE waves per SIMD (168 VGPRs, ~195 of them spilled; the small LDS tables of the three-wave
// simple kernel, two LDS entries of the walk's stack).  A frame that is mostly BVH walks waits as much as it issues at two
// waves (dragons 4K: four shadow walks per hit on a black background: 2.10 -> 1.97 ms), a frame that is mostly shading
// pays for the spills (teapot 0.27 -> 0.40): which of the two a scene is is MEASURED, not guessed - a handle times both
// kernels on its own steady-state frames and keeps the faster (rtc_capi.hip, KernelTune).
#if RTC_BVH8
extern "C" __global__ void __launch_bounds__(256, 3)
rtc_render_kernel3(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                   double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, false, 0, 3>(S, cam, map, max_depth, out, stats, next_stats);
}
#endif

#endif  // !RTC_MOTION_TU && !RTC_SPOT_TU && !RTC_BUMP_TU && !RTC_TORUS_TU && !RTC_EXT_TU

#if RTC_EXT_KERNELS_HERE
// The same two kernels with the csg and texture-map paths compiled in (template flag CSG), for scenes that
// have csg nodes or texture maps.  Kept apart because the out-of-line calls cost the main loop ~150 spilled
// VGPRs at every trace site (1.07 -> 1.38 ms on cover.json when csg was part of the only kernel).
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_ext(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                      double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, true>(S, cam, map, max_depth, out, stats, next_stats);
}

// Worlds of top-level spheres, planes and cubes whose patterns include texture maps (earth, skybox, align_check): the
// `simple` kernel with the texture-map path compiled in - none of the group traversal, no csg.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_simple_ext(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                             double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, true, 2, 2, false, false>(S, cam, map, max_depth, out, stats, next_stats);
}

// Worlds without groups or csg but with other leaf kinds at top level (cylinders, cones, triangles: cylinders.json,
// earth.json's pedestal, xyz.json): none of the group traversal either; planes, spheres and cubes one kind at a time,
// the rest in table order.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_flat(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                       double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, false, 1>(S, cam, map, max_depth, out, stats, next_stats);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_flat_ext(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                           double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<true, true, 1>(S, cam, map, max_depth, out, stats, next_stats);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_bigworld_ext(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                               double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats) {
  render_body<false, true>(S, cam, map, max_depth, out, stats, next_stats);
}

// Worlds with area lights (rtc_scene_create_with_lights; the book's bonus chapter): the general walk with the csg and
// texture-map paths compiled in, World.lights' area rows as an extra argument (DevAreaLights) - every other kernel is
// compiled without them.  Tables in LDS (the area rows beside the point lights, RTC_LDS_LIGHTS of them) or in memory.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_area(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                       double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                       const DevAreaLights area) {
  render_body<true, true, 0, 2, false, true, true>(S, cam, map, max_depth, out, stats, next_stats, area);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_area_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                const DevAreaLights area) {
  render_body<false, true, 0, 2, false, true, true>(S, cam, map, max_depth, out, stats, next_stats, area);
}
#endif  // RTC_EXT_KERNELS_HERE

#if !defined(RTC_MOTION_TU) && !defined(RTC_SPOT_TU) && !defined(RTC_BUMP_TU) && !defined(RTC_TORUS_TU) && !defined(RTC_EXT_TU)
// Several camera samples per pixel (rtc_scene_set_sampling: anti-aliasing, focal blur): the general walk with the csg and
// texture-map paths compiled in, the sampling parameters as an extra argument (DevSampling) - every other kernel is
// compiled without them.  Point lights (tables in LDS or in memory), and the area-light forms.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_ms(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                     double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                     const DevSampling smp) {
  render_body<true, true, 0, 2, false, true, false, true>(S, cam, map, max_depth, out, stats, next_stats, DevAreaLights{}, smp);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_ms_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                              double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                              const DevSampling smp) {
  render_body<false, true, 0, 2, false, true, false, true>(S, cam, map, max_depth, out, stats, next_stats, DevAreaLights{}, smp);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_area_ms(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                          double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                          const DevAreaLights area, const DevSampling smp) {
  render_body<true, true, 0, 2, false, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_area_ms_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                   double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                   const DevAreaLights area, const DevSampling smp) {
  render_body<false, true, 0, 2, false, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp);
}

// Rank 0's un-permute after the tile gather: one thread per canvas channel value, so both the read (a run
// of tile_w * 3 doubles inside one tile row) and the write (the canvas row) are contiguous across a wave.
extern "C" __global__ void __launch_bounds__(256)
rtc_assemble_kernel(const double* __restrict__ gathered, const uint32_t world, const uint32_t padded,
                    const uint32_t tile_w, const uint32_t tile_h, const uint32_t hsize, const uint32_t vsize,
                    double* __restrict__ canvas) {
  const size_t n = static_cast<size_t>(hsize) * vsize * 3u;
  const uint32_t tiles_x = (hsize + tile_w - 1u) / tile_w;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const size_t pixel = i / 3u;
    const uint32_t ch = static_cast<uint32_t>(i - pixel * 3u);
    const uint32_t y = static_cast<uint32_t>(pixel / hsize), x = static_cast<uint32_t>(pixel - static_cast<size_t>(y) * hsize);
    const uint32_t tile = (y / tile_h) * tiles_x + x / tile_w;
    const uint32_t r = tile % world, k = tile / world;
    const size_t src = (((static_cast<size_t>(r) * padded + k) * tile_h + y % tile_h) * tile_w + x % tile_w) * 3u + ch;
    canvas[i] = gathered[src];
  }
}

// The RGBA8 framebuffer of the reference's interactive seam (lib.zig:146-153): clamp() of color.zig:61-71 on every
// channel of an [n][3] f64 canvas - @round (half away from zero) of channel * 255, clamped to 0..255 - alpha 255.
// One thread per pixel; 8 MB instead of 50 leave the GPU for a 1080p frame.
extern "C" __global__ void __launch_bounds__(256)
rtc_rgba8_kernel(const double* __restrict__ canvas, const size_t n_pixels, uint32_t* __restrict__ rgba) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_pixels) return;
  auto clamp = [](double channel) -> uint32_t {
    const double t = round(channel * 255);
    if (!(t >= 0)) return 0u;  // negative (or NaN, on which Zig's @intFromFloat would trap)
    if (t > 255) return 255u;
    return static_cast<uint32_t>(t);
  };
  const double r = canvas[3 * i], g = canvas[3 * i + 1], b = canvas[3 * i + 2];
  rgba[i] = clamp(r) | (clamp(g) << 8) | (clamp(b) << 16) | 0xFF000000u;
}

// The same for a cost-balanced split: tile t sits in slot slot_of_tile[t] (rank * padded + k) of the gathered buffer.
extern "C" __global__ void __launch_bounds__(256)
rtc_assemble_list_kernel(const double* __restrict__ gathered, const uint32_t* __restrict__ slot_of_tile,
                         const uint32_t tile_w, const uint32_t tile_h, const uint32_t hsize, const uint32_t vsize,
                         double* __restrict__ canvas) {
  const size_t n = static_cast<size_t>(hsize) * vsize * 3u;
  const uint32_t tiles_x = (hsize + tile_w - 1u) / tile_w;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const size_t pixel = i / 3u;
    const uint32_t ch = static_cast<uint32_t>(i - pixel * 3u);
    const uint32_t y = static_cast<uint32_t>(pixel / hsize), x = static_cast<uint32_t>(pixel - static_cast<size_t>(y) * hsize);
    const uint32_t slot = slot_of_tile[(y / tile_h) * tiles_x + x / tile_w];
    const size_t src = ((static_cast<size_t>(slot) * tile_h + y % tile_h) * tile_w + x % tile_w) * 3u + ch;
    canvas[i] = gathered[src];
  }
}

// ... and for shares that were clamped to RGBA8 before they were gathered (4 bytes per pixel cross the links instead of
// 24): one thread per pixel of the framebuffer.
extern "C" __global__ void __launch_bounds__(256)
rtc_assemble_list_rgba8_kernel(const uint32_t* __restrict__ gathered, const uint32_t* __restrict__ slot_of_tile,
                               const uint32_t tile_w, const uint32_t tile_h, const uint32_t hsize, const uint32_t vsize,
                               uint32_t* __restrict__ rgba) {
  const size_t n = static_cast<size_t>(hsize) * vsize;
  const uint32_t tiles_x = (hsize + tile_w - 1u) / tile_w;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const uint32_t y = static_cast<uint32_t>(i / hsize), x = static_cast<uint32_t>(i - static_cast<size_t>(y) * hsize);
    const uint32_t slot = slot_of_tile[(y / tile_h) * tiles_x + x / tile_w];
    rgba[i] = gathered[(static_cast<size_t>(slot) * tile_h + y % tile_h) * tile_w + x % tile_w];
  }
}

// A rank's compact tiles written straight to where they belong in a row-major canvas - the canvas being any memory the
// device can write, in particular the caller's REGISTERED host canvas (rtc_canvas_register: pinned and mapped): every
// GPU of a split frame then sends its own share over its own host link, 64-pixel rows at a time, instead of all shares
// funnelling through GPU 0 and one link (rtc_multi.h, host forms).  tiles[k] is tile tile_list[k] of the tiling.
// One thread per channel value; pixels of edge tiles outside the image are skipped.
extern "C" __global__ void __launch_bounds__(256)
rtc_scatter_tiles_kernel(const double* __restrict__ tiles, const uint32_t* __restrict__ tile_list, const uint32_t n_tiles,
                         const uint32_t tile_w, const uint32_t tile_h, const uint32_t hsize, const uint32_t vsize,
                         double* __restrict__ canvas) {
  const uint32_t tiles_x = (hsize + tile_w - 1u) / tile_w;
  const size_t per_tile = static_cast<size_t>(tile_w) * tile_h * 3u, n = per_tile * n_tiles;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const uint32_t k = static_cast<uint32_t>(i / per_tile);
    const uint32_t in = static_cast<uint32_t>(i - k * per_tile);
    const uint32_t ly = in / (tile_w * 3u), lx3 = in - ly * (tile_w * 3u);
    const uint32_t tile = tile_list[k], ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t y = ty * tile_h + ly, x3 = tx * tile_w * 3u + lx3;
    if (y < vsize && x3 < hsize * 3u) __builtin_nontemporal_store(tiles[i], canvas + static_cast<size_t>(y) * hsize * 3u + x3);
  }
}

// The same with the clamp of color.zig:61-71 on the way (rtc_rgba8_kernel): one thread per pixel, 4 bytes per pixel leave.
extern "C" __global__ void __launch_bounds__(256)
rtc_scatter_tiles_rgba8_kernel(const double* __restrict__ tiles, const uint32_t* __restrict__ tile_list, const uint32_t n_tiles,
                               const uint32_t tile_w, const uint32_t tile_h, const uint32_t hsize, const uint32_t vsize,
                               uint32_t* __restrict__ rgba) {
  const uint32_t tiles_x = (hsize + tile_w - 1u) / tile_w;
  const size_t per_tile = static_cast<size_t>(tile_w) * tile_h, n = per_tile * n_tiles;
  auto clamp = [](double channel) -> uint32_t {
    const double t = round(channel * 255);
    if (!(t >= 0)) return 0u;
    if (t > 255) return 255u;
    return static_cast<uint32_t>(t);
  };
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const uint32_t k = static_cast<uint32_t>(i / per_tile);
    const uint32_t in = static_cast<uint32_t>(i - k * per_tile);
    const uint32_t ly = in / tile_w, lx = in - ly * tile_w;
    const uint32_t tile = tile_list[k], ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t y = ty * tile_h + ly, x = tx * tile_w + lx;
    if (y < vsize && x < hsize) {
      const double r = tiles[3 * i], g = tiles[3 * i + 1], b = tiles[3 * i + 2];
      __builtin_nontemporal_store(clamp(r) | (clamp(g) << 8) | (clamp(b) << 16) | 0xFF000000u, rgba + static_cast<size_t>(y) * hsize + x);
    }
  }
}

// ------------------------------------------------------------------------------------------
// The schedule of the NEXT frame, packed on the device from what THIS frame measured: no host in
// the loop, so a moving camera (lib.zig:166-190) renders every frame with a schedule that is one frame old.  Policy:
// classes of a quarter octave of measured time, image order (about) kept inside a class - neighbouring chunks run at the
// same moment: same objects, same BVH nodes -, cheap chunks several to a packet, chunks above a wave's fair share cut
// into runs of pixels, those packets first; then every wave's first packet, longest first; behind those the schedule
// alternates between its long and its short end (rtc_pack_emit_kernel).  Small launches on the render's stream, every
// one a grid over chunks or packets (a single work-group doing all of it took 180 us at 1080p: forty dependent round
// trips to memory; these take 57 us together, profiles/HISTORY.md):
//   rtc_chunk_cost_kernel  per chunk: the sum of the per-pixel ray counts and how the rays are spread (DevChunkShape);
//                          clears what the next steps add into
//   rtc_chunk_time_kernel  a packet's measured time, shared among its items by their cost; counts the runs of a chunk
//   rtc_pack_class_kernel  per chunk: its time whole (cost x `cost_to_time` if it was not timed; a chunk that ran in
//                          runs: without what the runs added), its class; histogram, totals
//   rtc_pack_extra_kernel  (three rounds) what the cuts add to the frame, for the share a wave gets with them
//   rtc_pack_sort_kernel   counting sort by class, a block of 1024 consecutive chunks at a time; the runs of the chunks
//                          of cut classes, one packet each, at the front of the schedule
//   rtc_pack_emit_kernel   the other packets: k chunks of one class each, k = group_cap / the class's upper time bound, 1..16
// Results never depend on the schedule.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack_class(uint32_t t) {
  return static_cast<uint32_t>(4.0f * __builtin_log2f(1.0f + static_cast<float>(t)));  // < RTC_PACK_CLASSES for any 32-bit t
}

// The first frame of a pixel map has no measurement to be packed from.  One thread per chunk estimates what the chunk
// will cost from what its pixels can see: the ray through the chunk's centre, widened to a cone that holds the chunk's
// 64 pixels, against the bounding sphere of every World.objects entry (the FP32 spheres of the root loop), summing the
// roots' weights (rtc_scene_create: an opaque box 10 us per chunk, a mirror 3 x, glass 4 x, glass that also reflects
// 25 x, a mesh by the depth of its BVH).  Crude - it knows nothing about what a reflection goes on to hit - but it
// puts the glass first and the sky last in one launch of a few microseconds, on the device; round 1 did this on the host
// (14 ms of wall time for dragons at 4K).  Writes what rtc_chunk_cost_kernel + rtc_chunk_time_kernel would have left.
extern "C" __global__ void __launch_bounds__(256)
rtc_estimate_kernel(const DevScene S, const DevCamera cam, const DevPixelMap map, uint32_t* __restrict__ chunk_cost,
                    uint32_t* __restrict__ chunk_time, DevChunkShape* __restrict__ chunk_shape, DevPackState* __restrict__ state
#ifdef RTC_PROFILE
                    , unsigned long long* __restrict__ oob  // root-table indices outside their allocation (counted, not read)
#endif
                    ) {
  if (blockIdx.x == 0u) {
    uint32_t* z = reinterpret_cast<uint32_t*>(state);
    for (uint32_t i = threadIdx.x; i < sizeof(DevPackState) / sizeof(uint32_t); i += blockDim.x) z[i] = 0u;
  }
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= map.n_chunks) return;
  const uint32_t region = c / map.chunks_per_region, cr = c - region * map.chunks_per_region;
  const uint32_t ccy = cr / map.chunks_x;
  uint32_t px0 = (cr - ccy * map.chunks_x) * 8u, py0 = ccy * 8u;
  if (map.mode == 0u) {
    px0 += map.x0;
    py0 += map.y0;
  } else {
    const uint32_t tile = map.mode == 1u ? map.first_tile + region * map.tile_stride : map.tile_list[region];
    const uint32_t ty = tile / map.tiles_x;
    px0 += (tile - ty * map.tiles_x) * map.tile_w;
    py0 += ty * map.tile_h;
  }
  // Camera.rayForPixel (camera.zig:64-76) through the middle of the chunk, in FP32
  const float ps = static_cast<float>(cam.pixel_size);
  const float wx = static_cast<float>(cam.half_width) - (static_cast<float>(px0) + 4.0f) * ps;
  const float wy = static_cast<float>(cam.half_height) - (static_cast<float>(py0) + 4.0f) * ps;
  float m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = static_cast<float>(cam.inv[i]);
  const float ox = m[3], oy = m[7], oz = m[11];
  float dx = m[0] * wx + m[1] * wy - m[2], dy = m[4] * wx + m[5] * wy - m[6], dz = m[8] * wx + m[9] * wy - m[10];
  const float len = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
  const float inv_len = len > 0.0f ? 1.0f / len : 0.0f;
  dx *= inv_len;
  dy *= inv_len;
  dz *= inv_len;
  // half the chunk's diagonal seen from the camera: the pixel vector has length >= 1 in camera space (z = -1); the view
  // transform may scale, which `len` carries
  const float tan_a = 5.7f * ps * (len > 0.0f ? __builtin_sqrtf(m[0] * m[0] + m[4] * m[4] + m[8] * m[8]) * inv_len : 0.0f) + 1e-6f;
  float cost = 400.0f;  // a chunk of sky: ray generation and one trace that finds nothing
  for (uint32_t i = 0; i < S.n_roots; ++i) {
#ifdef RTC_PROFILE
    if ((i >> 1) >= S.n_root_cull || i >= S.n_root_recs || i >= S.n_root_weight) {
      atomicAdd(oob, 1ull);
      continue;
    }
#endif
    const RootCullPair P = S.root_cull[i >> 1];
    const float cx = P.cx[i & 1u], cy = P.cy[i & 1u], cz = P.cz[i & 1u], r2 = P.r2[i & 1u];
    bool seen = true;  // no finite bound (a plane): every pixel may see it
    if (r2 < 3.0e38f) {
      const float ocx = cx - ox, ocy = cy - oy, ocz = cz - oz;
      const float t = ocx * dx + ocy * dy + ocz * dz;
      const float r = __builtin_sqrtf(r2);
      const float perp2 = (ocx * ocx + ocy * ocy + ocz * ocz) - t * t;
      const float reach = r + fmaxf(t, 0.0f) * tan_a;
      seen = (t + r > 0.0f) & (perp2 <= reach * reach);
    }
    // A cube fills a third of its bounding sphere's outline, and the spheres of neighbouring cubes overlap: for a top-level
    // sphere or cube the centre ray is taken into the object's space (Ray.transform) and tested against the unit shape
    // grown by the chunk's cone there (the cone's radius at the object, in object units: the inverse's largest row norm).
    if (seen && r2 < 3.0e38f) {
      const RootRec& R = S.root_recs[i];
      const uint32_t kind = R.kind_flags & 0xFFu;
      if ((R.kind_flags & RTC_ROOT_IS_GROUP) == 0u && (kind == 0u || kind == 2u)) {
        float M[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) M[k] = static_cast<float>(R.inv[k]);
        const float qx = M[0] * ox + M[1] * oy + M[2] * oz + M[3], qy = M[4] * ox + M[5] * oy + M[6] * oz + M[7],
                    qz = M[8] * ox + M[9] * oy + M[10] * oz + M[11];
        const float ex = M[0] * dx + M[1] * dy + M[2] * dz, ey = M[4] * dx + M[5] * dy + M[6] * dz, ez = M[8] * dx + M[9] * dy + M[10] * dz;
        const float norm = __builtin_sqrtf(fmaxf(fmaxf(M[0] * M[0] + M[1] * M[1] + M[2] * M[2], M[4] * M[4] + M[5] * M[5] + M[6] * M[6]),
                                                 M[8] * M[8] + M[9] * M[9] + M[10] * M[10]));
        const float ocx = cx - ox, ocy = cy - oy, ocz = cz - oz;
        const float dist = fmaxf(0.0f, ocx * dx + ocy * dy + ocz * dz);
        const float grow = 1.0f + dist * tan_a * norm;
        if (kind == 0u) {  // |q + t e|^2 = grow^2 has a root at t >= 0
          const float a = ex * ex + ey * ey + ez * ez, b = qx * ex + qy * ey + qz * ez, c = qx * qx + qy * qy + qz * qz - grow * grow;
          seen = (b * b - a * c >= 0.0f) & ((c <= 0.0f) | (b < 0.0f));
        } else {
          const float ix = 1.0f / __builtin_copysignf(fmaxf(__builtin_fabsf(ex), 1e-30f), ex);
          const float iy = 1.0f / __builtin_copysignf(fmaxf(__builtin_fabsf(ey), 1e-30f), ey);
          const float iz = 1.0f / __builtin_copysignf(fmaxf(__builtin_fabsf(ez), 1e-30f), ez);
          const float t0x = (-grow - qx) * ix, t1x = (grow - qx) * ix, t0y = (-grow - qy) * iy, t1y = (grow - qy) * iy;
          const float t0z = (-grow - qz) * iz, t1z = (grow - qz) * iz;
          const float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), 0.0f));
          const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
          seen = tn <= tf;
        }
      }
    }
    float w = seen ? S.root_weight[i] : 0.0f;
#if RTC_BVH8
    // A mesh is not its bounding sphere: most chunks inside the sphere's outline see no triangle at all (teapot's first
    // frame ran 56 % over its steady state on such a schedule).  For a group the root's weight is scaled by how much
    // of the chunk looks at geometry: four sample rays (the centres of the chunk's quadrants) against the top two levels
    // of the group's eight-wide candidate BVH - up to 64 boxes, one 80-byte node each for the root and for every inner
    // child a ray enters.  A twentieth of the weight stays for the walk that finds nothing.
    if (seen && r2 < 3.0e38f) {
      const RootRec& R = S.root_recs[i];
      if ((R.kind_flags & (RTC_ROOT_IS_GROUP | RTC_ROOT_IS_CSG)) == RTC_ROOT_IS_GROUP) {
        int entered = 0;
        // (a 4K frame has 130 000 chunks: two samples - opposite quadrants - there, or the estimate costs what it saves)
        const int n_samples = map.n_chunks > 65536u ? 2 : 4;
#pragma unroll 1
        for (int qi = 0; qi < n_samples; ++qi) {
          const int q = n_samples == 2 ? 3 * qi : qi;
          const float sx = static_cast<float>(px0) + ((q & 1) ? 6.0f : 2.0f), sy = static_cast<float>(py0) + ((q & 2) ? 6.0f : 2.0f);
          const float qx = static_cast<float>(cam.half_width) - sx * ps, qy = static_cast<float>(cam.half_height) - sy * ps;
          float ex = m[0] * qx + m[1] * qy - m[2], ey = m[4] * qx + m[5] * qy - m[6], ez = m[8] * qx + m[9] * qy - m[10];
          const float il = 1.0f / fmaxf(__builtin_sqrtf(ex * ex + ey * ey + ez * ez), 1e-30f);
          ex *= il;
          ey *= il;
          ez *= il;
          const float ix = 1.0f / __builtin_copysignf(fmaxf(__builtin_fabsf(ex), 1e-30f), ex);
          const float iy = 1.0f / __builtin_copysignf(fmaxf(__builtin_fabsf(ey), 1e-30f), ey);
          const float iz = 1.0f / __builtin_copysignf(fmaxf(__builtin_fabsf(ez), 1e-30f), ez);
          // boxes a quadrant's centre ray passes within the quadrant's half-diagonal of: the box grown by t * tan(2.9 pixels)
          auto node_hits = [&](uint32_t node, uint32_t& inner_mask, uint32_t& child_base) -> uint32_t {
            const Bvh8Node& N = S.bvh8[node];
            const float stx = __builtin_bit_cast(float, static_cast<uint32_t>(N.ex) << 23);
            const float sty = __builtin_bit_cast(float, static_cast<uint32_t>(N.ey) << 23);
            const float stz = __builtin_bit_cast(float, static_cast<uint32_t>(N.ez) << 23);
            uint32_t hits = 0u;
            for (int k = 0; k < 8; ++k) {
              const float lx = N.ox + stx * N.q[k], ly = N.oy + sty * N.q[8 + k], lz = N.oz + stz * N.q[16 + k];
              const float hx = N.ox + stx * N.q[24 + k], hy = N.oy + sty * N.q[32 + k], hz = N.oz + stz * N.q[40 + k];
              if (lx > hx) continue;  // an empty slot
              const float dist = fmaxf(0.0f, (0.5f * (lx + hx) - ox) * ex + (0.5f * (ly + hy) - oy) * ey + (0.5f * (lz + hz) - oz) * ez);
              const float grow = dist * tan_a * 0.5f;
              const float t0x = (lx - grow - ox) * ix, t1x = (hx + grow - ox) * ix;
              const float t0y = (ly - grow - oy) * iy, t1y = (hy + grow - oy) * iy;
              const float t0z = (lz - grow - oz) * iz, t1z = (hz + grow - oz) * iz;
              const float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), 0.0f));
              const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
              hits |= (tn <= tf) ? (1u << k) : 0u;
            }
            inner_mask = N.imask;
            child_base = N.child_base;
            return hits;
          };
          uint32_t imask = 0u, base = 0u;
          const uint32_t top = node_hits(R.geom, imask, base);
          bool any = (top & ~imask) != 0u;  // a leaf child of the root entered
          for (uint32_t todo = top & imask; todo != 0u && !any; todo &= todo - 1u) {
            const uint32_t slot = static_cast<uint32_t>(__builtin_ctz(todo));
            uint32_t im2 = 0u, b2 = 0u;
            any = node_hits(base + static_cast<uint32_t>(__builtin_popcount(imask & ((1u << slot) - 1u))), im2, b2) != 0u;
          }
          entered += any ? 1 : 0;
        }
        w *= 0.05f + 0.95f * static_cast<float>(entered) / static_cast<float>(n_samples);
      }
    }
#endif
    cost += w;  // (the plain sum: counting the roots in view other than the heaviest with 0 - 50 % of their weight measured no better)
  }
  chunk_cost[c] = static_cast<uint32_t>(fminf(cost, 4.0e9f));
  chunk_time[c] = 0u;  // nothing was timed: the packer takes the cost (cost_to_time = 1)
  chunk_shape[c].rays = 0.0f;  // (not measured: a chunk that is cut is cut into equal runs)
  chunk_shape[c].parts = 0u;
}

// One wave per 8x8 chunk: coalesced rows of the cost array.
extern "C" __global__ void __launch_bounds__(256)
rtc_chunk_cost_kernel(const uint32_t* __restrict__ cost, const DevPixelMap map, const uint32_t max_depth,
                      uint32_t* __restrict__ chunk_cost, uint32_t* __restrict__ chunk_time,
                      DevChunkShape* __restrict__ chunk_shape, DevPackState* __restrict__ state) {
  if (blockIdx.x == 0u) {
    uint32_t* z = reinterpret_cast<uint32_t*>(state);
    for (uint32_t i = threadIdx.x; i < sizeof(DevPackState) / sizeof(uint32_t); i += blockDim.x) z[i] = 0u;
  }
  const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), k = threadIdx.x & 63u;
  if (c >= map.n_chunks) return;
  const uint32_t region = c / map.chunks_per_region, cr = c - region * map.chunks_per_region;
  const uint32_t ccy = cr / map.chunks_x;
  const uint32_t rx = (cr - ccy * map.chunks_x) * 8u + (k & 7u), ry = ccy * 8u + (k >> 3);
  const uint32_t w = map.mode == 0u ? map.w : map.tile_w, h = map.mode == 0u ? map.h : map.tile_h;
  const size_t out0 = map.mode == 0u ? 0 : static_cast<size_t>(region) * map.tile_h * map.tile_w;
  const bool inside = rx < w && ry < h;
  const uint32_t mine = inside ? cost[out0 + static_cast<size_t>(ry) * w + rx] : 0u;
  uint32_t sum = mine;
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  // How the chunk's rays are spread over its pixels (the model of cut_runs below: a pixel's tree has about
  // cost / 5 rays and min(rays, max_depth + 1) levels): the total, the deepest tree, and the sixteenths of the running sum.
  const float rays = inside ? fmaxf(1.0f, static_cast<float>(mine) * 0.2f) : 0.0f;
  float run = rays;  // inclusive prefix sum over the wave's lanes = the chunk's pixels in row-major order
  for (int off = 1; off < 64; off <<= 1) {
    const float below = __shfl_up(run, off, 64);
    if (k >= static_cast<uint32_t>(off)) run += below;
  }
  const float total = __shfl(run, 63, 64);
  float deepest = fminf(rays, static_cast<float>(max_depth) + 1.0f);
  for (int off = 32; off > 0; off >>= 1) deepest = fmaxf(deepest, __shfl_xor(deepest, off, 64));
  uint32_t bound = 0u;  // lane j < 16: q[j]
  for (uint32_t j = 1u; j < 16u; ++j) {
    const unsigned long long passed = __ballot(run >= total * (static_cast<float>(j) * (1.0f / 16.0f)));
    const uint32_t at = passed != 0ull ? static_cast<uint32_t>(__builtin_ctzll(passed)) : 63u;
    if (k == j) bound = at + 1u;  // (the pixel that passes the mark still belongs to the run before it)
  }
  if (k < 16u) chunk_shape[c].q[k] = static_cast<uint8_t>(bound);
  if (k == 0u) {
    chunk_cost[c] = sum;
    chunk_time[c] = 0u;
    chunk_shape[c].rays = total;
    chunk_shape[c].depth = deepest;
    chunk_shape[c].parts = 0u;
  }
}

// One thread per packet of the schedule the measured launch ran (prev_order == nullptr: packet p was chunk p).
extern "C" __global__ void __launch_bounds__(256)
rtc_chunk_time_kernel(const uint32_t* __restrict__ prev_order, const uint32_t* __restrict__ prev_n_units_dev,
                      const uint32_t prev_n_units_host, const uint32_t* __restrict__ packet_time,
                      const uint32_t* __restrict__ chunk_cost, const uint32_t n_chunks, uint32_t* __restrict__ chunk_time,
                      DevChunkShape* __restrict__ chunk_shape) {
  const uint32_t prev_n = prev_order == nullptr ? n_chunks : (prev_n_units_dev != nullptr ? *prev_n_units_dev : prev_n_units_host);
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= prev_n) return;
  const uint32_t pt = packet_time[p];
  if (pt == 0u) return;
  if (prev_order == nullptr) {
    if (p < n_chunks) atomicAdd(&chunk_time[p], pt);
    return;
  }
  float w[RTC_PACKET_ITEMS], sum = 0.0f;
  uint32_t ch[RTC_PACKET_ITEMS];
  const uint4* row = reinterpret_cast<const uint4*>(prev_order + static_cast<size_t>(p) * RTC_PACKET_ITEMS);
#pragma unroll
  for (uint32_t q = 0; q < RTC_PACKET_ITEMS / 4u; ++q) {
    const uint4 v = row[q];
    const uint32_t its[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t it = its[e];
      const uint32_t c = it & 0xFFFFFu, len = (it >> 26) + 1u;
      const bool ok = it != RTC_NO_ITEM && c < n_chunks;
      ch[q * 4u + e] = ok ? c : RTC_NO_ITEM;
      w[q * 4u + e] = ok ? (static_cast<float>(chunk_cost[ok ? c : 0u]) + 1.0f) * static_cast<float>(len) * (1.0f / 64.0f) : 0.0f;
      sum += w[q * 4u + e];
    }
  }
  if (!(sum > 0.0f)) return;
  // (atomics: a chunk that was cut into runs is timed in several packets - and counted, see rtc_pack_class_kernel)
#pragma unroll
  for (uint32_t i = 0; i < RTC_PACKET_ITEMS; ++i)
    if (ch[i] != RTC_NO_ITEM) {
      atomicAdd(&chunk_time[ch[i]], static_cast<uint32_t>(static_cast<float>(pt) * w[i] / sum));
      atomicAdd(&chunk_shape[ch[i]].parts, 1u);
    }
}

// One thread per chunk.
extern "C" __global__ void __launch_bounds__(1024)
rtc_pack_class_kernel(const uint32_t* __restrict__ chunk_cost, const uint32_t n_chunks, const float cost_to_time,
                      const DevChunkShape* __restrict__ chunk_shape, uint32_t* __restrict__ chunk_time,
                      DevPackState* __restrict__ state) {
  __shared__ uint32_t cnt[RTC_PACK_CLASSES];
  __shared__ unsigned long long sh_total;
  __shared__ uint32_t sh_heaviest;
  const uint32_t tid = threadIdx.x;
  if (tid < RTC_PACK_CLASSES) cnt[tid] = 0u;
  if (tid == 0u) {
    sh_total = 0ull;
    sh_heaviest = 0u;
  }
  __syncthreads();
  const uint32_t c = blockIdx.x * blockDim.x + tid;
  unsigned long long total = 0ull;
  uint32_t heaviest = 0u;
  if (c < n_chunks) {
    const uint32_t t = chunk_time[c];
    // a chunk that was not timed (a probe launch times nothing): its cost at the caller's estimate of ticks per unit
    float v = t != 0u ? static_cast<float>(t) : static_cast<float>(chunk_cost[c]) * cost_to_time;
    // A chunk that ran in r parts was timed r times, and every part paid for the depth of its deepest tree: the parts
    // took (r L + S) iterations together, the chunk whole would take L + S (the model of rtc_pack_emit_kernel).  What is
    // packed is the time of the WHOLE chunk - otherwise a cut chunk looks heavier than it is and is cut further.
    const DevChunkShape shape = chunk_shape[c];
    if (t != 0u && shape.parts > 1u && shape.rays > 0.0f) {
      const float S = shape.rays * (1.0f / 64.0f);
      v *= (shape.depth + S) / (static_cast<float>(shape.parts) * shape.depth + S);
    }
    const uint32_t tv = v < 4.0e9f ? static_cast<uint32_t>(v) : 4000000000u;
    chunk_time[c] = tv;
    total = tv;
    heaviest = tv;
    atomicAdd(&cnt[pack_class(tv)], 1u);
  }
  for (int off = 32; off > 0; off >>= 1) {
    total += __shfl_down(total, off, 64);
    heaviest = max(heaviest, static_cast<uint32_t>(__shfl_down(heaviest, off, 64)));
  }
  if ((tid & 63u) == 0u) {
    atomicAdd(&sh_total, total);
    atomicMax(&sh_heaviest, heaviest);
  }
  __syncthreads();
  if (tid < RTC_PACK_CLASSES && cnt[tid] != 0u) atomicAdd(&state->cnt[tid], cnt[tid]);
  if (tid == 0u) {
    atomicAdd(&state->total, sh_total);
    atomicMax(&state->heaviest, sh_heaviest);
  }
}

// Into how many runs a chunk of a cut class goes.  A wave renders one ray per lane
// per iteration and the rays of a pixel's tree depend on each other level by level: pixels [a, b) take about L + S
// iterations, L the deepest tree among them, S their rays / 64.  Every part pays L again, so the chunk is cut until a
// part fits a wave's share or its S falls under L / 2 - a chunk that is all depth (a mirror chain, a few glass pixels on
// a silhouette) stays whole.  At most sixteen: the runs end on sixteenths of the chunk's rays (DevChunkShape::q).
// Without a measurement of the spread (the first frame of a pixel map): by the time alone, equal runs.
__device__ __forceinline__ uint32_t cut_runs(const DevChunkShape& shape, const float T, const float fair) {
  float want = T / fmaxf(fair, 1.0f);
  if (shape.rays > 0.0f) {
    const float S = shape.rays * (1.0f / 64.0f), depth = shape.depth;
    const float per_iteration = T / fmaxf(depth + S, 1e-9f);
    const float room = fmaxf(fair / fmaxf(per_iteration, 1e-9f) - depth, fmaxf(0.5f * depth, 0.5f));
    want = S / room;
  }
  return static_cast<uint32_t>(fminf(fmaxf(__builtin_ceilf(want), 1.0f), 16.0f));
}

// A wave's fair share of the frame, the time the cuts add included (`round` rounds of rtc_pack_extra_kernel, at most
// four: a cut adds work, which raises the share, which takes back some cuts).
__device__ __forceinline__ float fair_share(const DevPackState* __restrict__ state, const float n_waves, const int round) {
  const unsigned long long extra = round > 0 ? state->extra[round - 1] : 0ull;
  return static_cast<float>(state->total + extra) / fmaxf(1.0f, n_waves);
}

// One thread per chunk: what cutting it (with the share of round - 1) adds to the frame.
extern "C" __global__ void __launch_bounds__(1024)
rtc_pack_extra_kernel(const uint32_t* __restrict__ chunk_time, const uint32_t n_chunks, const float n_waves, const float cut_above,
                      const DevChunkShape* __restrict__ chunk_shape, const int round, DevPackState* __restrict__ state) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  float add = 0.0f;
  if (c < n_chunks && cut_above > 0.0f) {
    const float fair = fair_share(state, n_waves, round), T = static_cast<float>(chunk_time[c]);
    const DevChunkShape shape = chunk_shape[c];
    if (T > cut_above * fair && shape.rays > 0.0f) {
      const uint32_t r = cut_runs(shape, T, fair);
      const float S = shape.rays * (1.0f / 64.0f);
      add = static_cast<float>(r - 1u) * shape.depth * T / fmaxf(shape.depth + S, 1e-9f);
    }
  }
  for (int off = 32; off > 0; off >>= 1) add += __shfl_down(add, off, 64);
  if ((threadIdx.x & 63u) == 0u && add > 0.0f) atomicAdd(&state->extra[round], static_cast<unsigned long long>(add));
}

// Class bases (longest class first), chunks per packet and first packet of every class, from the histogram.
struct PackLayout {
  uint32_t cbase[RTC_PACK_CLASSES], per_packet[RTC_PACK_CLASSES], pbase[RTC_PACK_CLASSES], parts[RTC_PACK_CLASSES], n_packets;
};
// Called by every thread of a work-group (at least RTC_PACK_CLASSES of them); ends with a barrier.
// cut_above: a class whose chunks take more than this many fair shares of a wave is CUT - every chunk of it into 1, 2,
// 4, 8 or 16 runs of consecutive pixels, one packet each (cut_runs).  Small images and one rank's share of a frame split
// over GPUs have such chunks (a full 1080p frame's heaviest chunk is about one share), and a launch ends when its
// longest packet does.  The runs' packets are the FIRST of the schedule (the longest there are); a cut class has no
// packets in the part of the schedule laid out here.  0: nothing is cut.
__device__ __forceinline__ void pack_layout(const DevPackState* __restrict__ state, const float n_waves, const float t_min,
                                            const float cut_above, const int rounds, PackLayout& L) {
  const uint32_t k = threadIdx.x;
  if (k < RTC_PACK_CLASSES) {  // per class, in parallel: its size, chunks per packet, packets
    const float fair = fair_share(state, n_waves, rounds);
    const float group_cap = fmaxf(fair * (1.0f / 32.0f), t_min);
    const float t_hi = __builtin_exp2f(static_cast<float>(k + 1u) * 0.25f) - 1.0f;  // upper time bound of class k
    const float per = group_cap / fmaxf(t_hi, 1.0f);
    const uint32_t kk = per >= 16.0f ? 16u : (per < 1.0f ? 1u : static_cast<uint32_t>(per));
    const uint32_t n = state->cnt[k];
    const bool cut = cut_above > 0.0f && t_hi > cut_above * fair;
    L.per_packet[k] = kk;
    L.parts[k] = cut ? 1u : 0u;       // a cut class: its chunks' packets are at the front of the schedule (rtc_pack_sort_kernel)
    L.cbase[k] = n;                   // (turned into the exclusive sums below)
    L.pbase[k] = cut ? 0u : (n + kk - 1u) / kk;
  }
  __syncthreads();
  if (k == 0u) {  // longest class first
    uint32_t at = 0u, packets = 0u;
    for (int c = RTC_PACK_CLASSES - 1; c >= 0; --c) {
      const uint32_t n = L.cbase[c], np = L.pbase[c];
      L.cbase[c] = at;
      L.pbase[c] = packets;
      at += n;
      packets += np;
    }
    L.n_packets = packets;
  }
  __syncthreads();
}

// One work-group per block of 1024 consecutive chunks: a class keeps the image order of its chunks block by block
// (inside a block and between blocks the order is arrival order).
extern "C" __global__ void __launch_bounds__(1024)
rtc_pack_sort_kernel(const uint32_t* __restrict__ chunk_time, const uint32_t n_chunks, const float n_waves, const float t_min,
                     const float cut_above, const int rounds, const DevChunkShape* __restrict__ chunk_shape,
                     DevPackState* __restrict__ state, uint32_t* __restrict__ sorted, uint32_t* __restrict__ order_out) {
  __shared__ PackLayout L;
  __shared__ uint32_t cnt[RTC_PACK_CLASSES], start[RTC_PACK_CLASSES], cursor[RTC_PACK_CLASSES];
  const uint32_t tid = threadIdx.x;
  if (tid < RTC_PACK_CLASSES) {
    cnt[tid] = 0u;
    cursor[tid] = 0u;
  }
  pack_layout(state, n_waves, t_min, cut_above, rounds, L);
  const uint32_t c = blockIdx.x * blockDim.x + tid;
  uint32_t k = 0u;
  if (c < n_chunks) {
    k = pack_class(chunk_time[c]);
    atomicAdd(&cnt[k], 1u);
  }
  __syncthreads();
  if (tid < RTC_PACK_CLASSES && cnt[tid] != 0u) start[tid] = atomicAdd(&state->cursor[tid], cnt[tid]);
  __syncthreads();
  if (c < n_chunks) sorted[L.cbase[k] + start[k] + atomicAdd(&cursor[k], 1u)] = c | (k << 20);  // 2^20 chunks at most; the class rides along
  if (c < n_chunks && L.parts[k] != 0u) {  // a chunk of a cut class: its runs, one packet each, at the front of the schedule
    const DevChunkShape shape = chunk_shape[c];
    const float fair = fair_share(state, n_waves, rounds), T = static_cast<float>(chunk_time[c]);
    // (never more than 1 + 15 T / F runs: the chunks' times add up to at most F x the waves, so all cuts together add
    // at most 15 packets per wave - what the schedule buffers are sized for, maxPackets() in rtc_capi.hip.  The model
    // asks for about T / F.)
    const uint32_t r = min(cut_runs(shape, T, fair), 1u + static_cast<uint32_t>(fminf(15.0f * T / fmaxf(fair, 1.0f), 15.0f)));
    const uint32_t at = atomicAdd(&state->parts_cursor, r);
    // run q ends at the sixteenth of the chunk's rays (or, unmeasured, of its pixels) nearest to (q + 1) / r
    auto mark = [&](uint32_t q) -> uint32_t {
      const uint32_t sixteenth = (16u * q + r / 2u) / r;
      return shape.rays > 0.0f ? shape.q[sixteenth] : sixteenth * 4u;
    };
    for (uint32_t q = 0; q < r; ++q) {
      const uint32_t a = q == 0u ? 0u : mark(q);
      const uint32_t b = q + 1u == r ? 64u : mark(q + 1u);
      uint4* row = reinterpret_cast<uint4*>(order_out + static_cast<size_t>(at + q) * RTC_PACKET_ITEMS);
      row[0] = uint4{b > a ? (c | (a << 20) | ((b - a - 1u) << 26)) : RTC_NO_ITEM, RTC_NO_ITEM, RTC_NO_ITEM, RTC_NO_ITEM};  // (an empty run: an empty packet)
      row[1] = row[2] = row[3] = uint4{RTC_NO_ITEM, RTC_NO_ITEM, RTC_NO_ITEM, RTC_NO_ITEM};
    }
  }
}

// One thread per sorted chunk; the first chunk of each packet writes the whole row of 16 items.
extern "C" __global__ void __launch_bounds__(1024)
rtc_pack_emit_kernel(const uint32_t* __restrict__ sorted, const uint32_t n_chunks, const float n_waves, const float t_min,
                     const float cut_above, const int rounds, const DevPackState* __restrict__ state,
                     uint32_t* __restrict__ order_out, DevSchedInfo* __restrict__ info, const int mix) {
  __shared__ PackLayout L;
  pack_layout(state, n_waves, t_min, cut_above, rounds, L);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0u) {
    info->n_units = state->parts_cursor + L.n_packets;
    info->heaviest = state->heaviest;
    info->pad_[0] = info->pad_[1] = 0u;
    info->total = state->total;
  }
  if (i >= n_chunks) return;
  const uint32_t e = sorted[i];
  const uint32_t k = e >> 20;
  const uint32_t j = i - L.cbase[k], kk = L.per_packet[k];
  if (L.parts[k] != 0u) return;  // (a cut class: rtc_pack_sort_kernel wrote its packets)
  if (j % kk != 0u) return;
  uint32_t rank = L.pbase[k] + j / kk;  // longest first
  if (mix != 0) {
    // Behind the first packet of every wave the schedule takes a packets from its long end, then b from its short end, and
    // so on (5 : 3), and ends in the middle of the range.  Longest first throughout - rounds 2 and 3 - puts every wave's
    // cheapest packets last, and by the per-wave log of the light profile build (tools/wave_ends.py) those ran several
    // times longer at the end of a frame than the schedule had them down for: cover 1080p 0.517 -> 0.498 ms, teapot
    // 0.268 -> 0.256, nefertiti 0.507 -> 0.490, dragons 4K 1.91 -> 1.89 with the same instructions and bytes
    // (profiles/r04/schedule_order.txt; 1:1, blocks, a reserved short tail, a pseudo-random order: all worse).
    const uint32_t a = max(1u, static_cast<uint32_t>(mix) & 0xFFu), b = max(1u, (static_cast<uint32_t>(mix) >> 8) & 0xFFu);
    const uint32_t mode = (static_cast<uint32_t>(mix) >> 16) & 0xFu;
    const uint32_t keep = min(static_cast<uint32_t>(n_waves), L.n_packets);
    if (rank >= keep) {
      const uint32_t m = L.n_packets - keep, r = rank - keep;
      if (mode == 1u) {  // (diagnostic: a fixed pseudo-random order)
        uint32_t K = 7919u;
        while (m % K == 0u || K % 2u == 0u) K += 2u;
        uint32_t g0 = m, g1 = K;  // gcd
        while (g1 != 0u) { const uint32_t t = g0 % g1; g0 = g1; g1 = t; }
        if (g0 == 1u) rank = keep + static_cast<uint32_t>((static_cast<unsigned long long>(r) * K) % m);
      } else {  // a packets from the long end, then b from the short end, and so on; what is left over (the middle) last
        const uint32_t G = min((m * a / (a + b)) / a, (m - m * a / (a + b)) / b);
        const uint32_t sa = G * a, sb = G * b;
        if (r < sa) {
          rank = keep + (r / a) * (a + b) + r % a;
        } else if (r >= m - sb) {
          const uint32_t c = m - 1u - r;
          rank = keep + (c / b) * (a + b) + a + c % b;
        } else {
          rank = keep + G * (a + b) + (r - sa);
        }
      }
    }
  }
  const uint32_t p = state->parts_cursor + rank;  // (behind the runs of the cut chunks)
  const uint32_t have = min(kk, state->cnt[k] - j);
  uint32_t items[RTC_PACKET_ITEMS];
#pragma unroll
  for (uint32_t q = 0; q < RTC_PACKET_ITEMS; ++q)
    items[q] = q < have ? ((sorted[i + q] & 0xFFFFFu) | (63u << 26)) : RTC_NO_ITEM;  // chunk | start 0 | (64 - 1) << 26
  uint4* row = reinterpret_cast<uint4*>(order_out + static_cast<size_t>(p) * RTC_PACKET_ITEMS);
#pragma unroll
  for (uint32_t q = 0; q < RTC_PACKET_ITEMS / 4u; ++q) row[q] = uint4{items[q * 4u], items[q * 4u + 1u], items[q * 4u + 2u], items[q * 4u + 3u]};
}

#elif defined(RTC_MOTION_TU)

// Motion blur (rtc_scene_set_motion): the area-sampling walk with the shutter time and the per-root shift compiled in
// (DevMotion), for point-only and area light tables alike (a point-only table comes with zero rows: every light takes the
// point path).  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_motion(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                         double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                         const DevAreaLights area, const DevSampling smp, const DevMotion mo) {
  render_body<true, true, 0, 2, false, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp, mo);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_motion_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                  double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                  const DevAreaLights area, const DevSampling smp, const DevMotion mo) {
  render_body<false, true, 0, 2, false, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp, mo);
}

#elif defined(RTC_SPOT_TU)

// Spot lights (rtc_scene_set_spots): the motion walk with the cones of point lights compiled in (DevSpots), one pair for
// every world and every combination of sampling, passes, motion and area lights (a static handle passes zero
// displacements, a point-only table zero area rows).  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_spot(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                       double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                       const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots) {
  render_body<true, true, 0, 2, false, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_spot_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots) {
  render_body<false, true, 0, 2, false, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots);
}

#elif defined(RTC_BUMP_TU)

// Normal perturbation (rtc_scene_set_bumps): the spot walk with the materials' bumps compiled in (DevBumps), one pair for
// every world and every combination of sampling, passes, motion, area lights and cones (a handle without cones passes
// zero spot rows).  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_bump(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                       double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                       const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp, mo,
                                                                           spots, bumps);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_bump_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                const DevBumps bumps) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp, mo,
                                                                            spots, bumps);
}

#elif defined(RTC_MIS_TU)

// Multiple importance sampling (rtc_scene_set_emitter_mis): the emitter walk with the balance
// heuristic's weights on the emitter samples and on the diffuse child's hit of a listed leaf, and the mode, the per-leaf entry
// words and the carry buffer of cos_b (DevMis) as one more argument; one pair for every world.  Every other kernel is compiled
// without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_mis(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                      double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                      const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                      const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl, const DevShadowFilter sfilt,
                      const DevMedia media, const DevEnvironment env, const DevSkyLight skyl, const DevIndirect indir,
                      const DevEmitters emit, const DevMis mis) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl, indir, emit, mis);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_mis_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                               double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                               const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                               const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl,
                               const DevShadowFilter sfilt, const DevMedia media, const DevEnvironment env, const DevSkyLight skyl,
                               const DevIndirect indir, const DevEmitters emit, const DevMis mis) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl, indir, emit, mis);
}

#elif defined(RTC_EMIT_TU)

// Emitter sampling (rtc_scene_set_emitters): the indirect walk with the emitter samples in the suns'
// loop and the suppressed emission of a diffuse child, and the emitter rows, their CDF, the leaf bits, the count, the sample
// count, the hash key and the total weight (DevEmitters) as one more argument; one pair for every world.  Every other kernel
// is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_emit(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                       double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                       const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                       const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl, const DevShadowFilter sfilt,
                       const DevMedia media, const DevEnvironment env, const DevSkyLight skyl, const DevIndirect indir,
                       const DevEmitters emit) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl, indir, emit);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_emit_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl,
                                const DevShadowFilter sfilt, const DevMedia media, const DevEnvironment env, const DevSkyLight skyl,
                                const DevIndirect indir, const DevEmitters emit) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl, indir, emit);
}

#elif defined(RTC_INDIR_TU)

// Indirect light (rtc_scene_set_indirect): the sky-light walk with the emission rows and the diffuse
// child, and the gain, the hash key, the bounce limit and the emission rows (DevIndirect) as one more argument; one pair for
// every world.  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_indir(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                        double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                        const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                        const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl, const DevShadowFilter sfilt,
                        const DevMedia media, const DevEnvironment env, const DevSkyLight skyl, const DevIndirect indir) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl, indir);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_indir_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                 double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                 const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                 const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl,
                                 const DevShadowFilter sfilt, const DevMedia media, const DevEnvironment env, const DevSkyLight skyl,
                                 const DevIndirect indir) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl, indir);
}

#elif defined(RTC_SKYL_TU)

// A sky light (rtc_scene_set_sky_light): the environment walk with the hemisphere rays that gather the
// sky at every diffuse hit, and the gain, the sample count and the hash key (DevSkyLight) as one more argument; one pair for
// every world.  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_skyl(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                       double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                       const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                       const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl, const DevShadowFilter sfilt,
                       const DevMedia media, const DevEnvironment env, const DevSkyLight skyl) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_skyl_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl,
                                const DevShadowFilter sfilt, const DevMedia media, const DevEnvironment env, const DevSkyLight skyl) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env, skyl);
}

#elif defined(RTC_ENV_TU)

// An environment (rtc_scene_set_environment): the media walk with a sky where a ray misses and the
// suns' loop after World.lights, and the sky and the sun rows (DevEnvironment) as one more argument; one pair for every
// world.  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_env(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                      double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                      const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                      const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl, const DevShadowFilter sfilt,
                      const DevMedia media, const DevEnvironment env) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_env_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                               double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                               const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                               const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl,
                               const DevShadowFilter sfilt, const DevMedia media, const DevEnvironment env) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media, env);
}

#elif defined(RTC_MEDIA_TU)

// Participating media (rtc_scene_set_media): the shadow-filter walk with a medium and a weight per
// channel carried by every ray of the tree, the segment's transmittance applied after every closest-hit trace, and the
// absorption rows, the atmosphere and the pending rays' fifth quarter in memory (DevMedia) as one more argument; one pair
// for every world.  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_media(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                        double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                        const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                        const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl, const DevShadowFilter sfilt,
                        const DevMedia media) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_media_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                 double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                 const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                 const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl,
                                 const DevShadowFilter sfilt, const DevMedia media) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt, media);
}

#elif defined(RTC_SFILT_TU)

// Shadow filters (rtc_scene_set_shadow_filters): the occlusion walk with every light's shadow ray
// multiplying the filter rows of the entries it crosses (FilterVisitor), and the filter rows (DevShadowFilter) as one more
// argument; one pair for every world, tori, textured meshes, rough materials and occlusion radii included.  Every other
// kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_sfilter(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                          double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                          const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                          const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl, const DevShadowFilter sfilt) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_sfilter_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                   double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                   const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                   const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl,
                                   const DevShadowFilter sfilt) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl, sfilt);
}

#elif defined(RTC_OCCL_TU)

// Ambient occlusion (rtc_scene_set_occlusion): the gloss walk with every hit's ambient term scaled by
// the share of its hemisphere rays that are not occluded within the material's radius, and the radius rows (DevOcclusion)
// as one more argument; one pair for every world, tori, textured meshes and rough materials included.  Every other kernel
// is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_occl(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                       double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                       const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                       const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_occl_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss, const DevOcclusion occl) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true, true>(
      S, cam, map, max_depth, out, stats, next_stats, area, smp, mo, spots, bumps, muv, gloss, occl);
}

#elif defined(RTC_GLOSS_TU)

// Glossy reflection and refraction (rtc_scene_set_gloss): the meshuv walk with every ray's path code in
// its Pending, the child directions of a rough material scattered, and the roughness rows (DevGloss) as one more argument;
// one pair for every world, tori and textured meshes included.  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_gloss(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                        double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                        const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                        const DevMeshUvs muv, const DevGloss gloss) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats,
                                                                                             area, smp, mo, spots, bumps, muv, gloss);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_gloss_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                 double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                 const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                 const DevBumps bumps, const DevMeshUvs muv, const DevGloss gloss) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats,
                                                                                              area, smp, mo, spots, bumps, muv, gloss);
}

#elif defined(RTC_MESHUV_TU)

// UV-mapped mesh textures (RTC_TEX_MESH): the torus walk with the hit's triangle and barycentrics
// handed to the pattern evaluation and the texture rows (DevMeshUvs) as one more argument; one pair for every world, tori
// included.  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_meshuv(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                         double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                         const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps,
                         const DevMeshUvs muv) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area,
                                                                                       smp, mo, spots, bumps, muv);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_meshuv_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                  double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                  const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                  const DevBumps bumps, const DevMeshUvs muv) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats,
                                                                                        area, smp, mo, spots, bumps, muv);
}

#elif defined(RTC_TORUS_TU)

// Torus primitives (RTC_TORUS): the bump walk with leaf kind 7 compiled in, one pair for every
// world and every combination of sampling, passes, motion, area lights, cones and bumps (a handle without bumps passes
// zero bump rows).  Every other kernel is compiled without it.
extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_torus(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                        double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                        const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots, const DevBumps bumps) {
  render_body<true, true, 0, 2, false, true, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area, smp,
                                                                                 mo, spots, bumps);
}

extern "C" __global__ void __launch_bounds__(256, RTC_LB2)
rtc_render_kernel_torus_bigworld(const DevScene S, const DevCamera cam, const DevPixelMap map, const uint32_t max_depth,
                                 double* __restrict__ out, DevStats* __restrict__ stats, DevStats* __restrict__ next_stats,
                                 const DevAreaLights area, const DevSampling smp, const DevMotion mo, const DevSpots spots,
                                 const DevBumps bumps) {
  render_body<false, true, 0, 2, false, true, true, true, true, true, true, true>(S, cam, map, max_depth, out, stats, next_stats, area,
                                                                                  smp, mo, spots, bumps);
}

#endif  // RTC_MOTION_TU / RTC_SPOT_TU / RTC_BUMP_TU / RTC_INDIR_TU / RTC_SKYL_TU / RTC_ENV_TU / RTC_MEDIA_TU / RTC_SFILT_TU / RTC_OCCL_TU / RTC_GLOSS_TU / RTC_MESHUV_TU / RTC_TORUS_TU
