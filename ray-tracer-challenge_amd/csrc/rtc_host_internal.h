// rtc_host_internal.h — what the host-side translation units of librtc_hip.so share: error reporting, the
// device-buffer holder and the scene handle behind `rtc_scene*` (include/rtc.h).  Included by rtc_capi.hip only.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <string>
#include <memory>
#include <vector>

#include "../../include/rtc.h"
#include "rtc_device.h"

namespace {

thread_local std::string g_error;

int fail(int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = std::string(rtc_status_name(status)) + ": " + buf;
  return status;
}

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      (void)hipGetLastError(); /* reported here: not the next call's hipGetLastError() */     \
      return fail(e_ == hipErrorOutOfMemory ? RTC_ERR_OUT_OF_MEMORY : RTC_ERR_NO_DEVICE,      \
                  "%s -> %s", #expr, hipGetErrorString(e_));                                  \
    }                                                                                         \
  } while (0)

// Tuning and test options (rtc_set_option, include/rtc_diag.h): process-wide, read when a scene is created or a launch is
// enqueued; none changes a result.  0 / negative = the library's own choice.  Every option is an atomic double (relaxed:
// an option is one independent number): a host thread may set one while another thread's launch reads it.
struct RtcOption {
  std::atomic<double> v;
  RtcOption(double d) : v(d) {}
  operator double() const { return v.load(std::memory_order_relaxed); }
  void set(double d) { v.store(d, std::memory_order_relaxed); }
};
struct RtcOptions {
  RtcOption simple3_min_chunks{-1.0};  // chunks from which a simple world runs the three-wave kernel (0: always)
  RtcOption sched_off{0.0};            // != 0: no schedule at all (packet i is chunk i)
  RtcOption cut_above{0.0};            // shares of a wave above which a chunk is cut into runs (< 0: never)
  RtcOption pack_rounds{3.0};          // rounds of rtc_pack_extra_kernel
  RtcOption pull_min_idle{64.0};       // idle lanes before a wave pulls its next packet
  RtcOption blocks_per_cu{0.0};        // cap on resident work-groups per CU
  RtcOption sched_tmin{0.0};           // time up to which cheap chunks share a packet
  RtcOption bvh_leaf{RTC_BVH8 ? 1.0 : 2.0};  // leaves per candidate-BVH leaf (eight-wide tree, 1 / 2 / 3 / 4: dragons 4K 2.03 / 2.10 / 2.18 / 2.30 ms, nefertiti 0.522 / 0.534 / 0.548 / 0.562, teapot 0.264 / 0.265 / 0.263 / 0.272)
  RtcOption bvh_one_axis{0.0};         // != 0: SAH on the longest axis only
  RtcOption bvh_check{0.0};            // != 0: host self-check of the candidate BVH at create (stderr)
  RtcOption waves3{-1.0};              // the general kernel at three waves per SIMD: 1 always (where the tables fit), 0 never, < 0: measured per handle
  RtcOption sched_mix{773.0};          // a | b << 8: behind every wave's first packet the schedule takes a packets from its long end, b from its short end, ... (5 : 3); 0: longest first throughout
  RtcOption inflight_chunks_per_wave{3.0};  // a launch of a scene with frames in flight runs on at most one wave per this many chunks (0: no cap)
  RtcOption measure_every{1.0};        // a moving view is measured (and its schedule re-packed) every this many frames (see updateSchedule)
  RtcOption host_bands{0.0};           // bands rtc_render cuts a frame into (copy of band i under the render of band i + 1); 0: by size
  RtcOption box_cull{-1.0};            // a simple world's kernels reject roots by world boxes (1) or bounding spheres (0); < 0: boxes if it has more cubes than spheres
  RtcOption containers_own_root{1.0};  // read at create: 0 leaves every root without RTC_ROOT_ALONE, so that every wave of a simple kernel makes the containers pass (tests: against a handle with the flags)
  RtcOption sampling_kernels{0.0};     // != 0: the sampling kernels even with the default sampling (tests: one sample against the other kernels)
  RtcOption motion_kernels{0.0};       // != 0: the motion kernels even on a static handle, all displacements zero (tests: against the _ms kernels)
  RtcOption spot_kernels{0.0};         // != 0: the spot kernels even on a handle without cones, every flag zero (tests: against the motion kernels)
  RtcOption bump_kernels{0.0};         // != 0: the bump kernels even on a handle without bumps, every row of kind none (tests: against the spot kernels)
  RtcOption torus_kernels{0.0};        // != 0: the torus kernels even on a handle without a torus (tests: against the bump kernels)
  RtcOption meshuv_kernels{0.0};       // != 0: the meshuv kernels even on a handle without a mesh map (tests: against the handle's ordinary kernels)
  RtcOption gloss_kernels{0.0};        // != 0: the gloss kernels even on a handle without a rough material, every row zero (tests: against the handle's ordinary kernels)
  RtcOption occlusion_kernels{0.0};    // != 0: the occlusion kernels even on a handle without a radius, every row zero (tests: against the handle's ordinary kernels)
  RtcOption shadow_filter_kernels{0.0};  // != 0: the shadow-filter kernels even on a handle without a filter, every row zero (tests: against the handle's ordinary kernels)
  RtcOption media_kernels{0.0};        // != 0: the media kernels even on a handle without media, every row and the density zero (tests: against the handle's ordinary kernels)
  RtcOption environment_kernels{0.0};  // != 0: the environment kernels even on a handle without an environment, no sky and no sun (tests: against the handle's ordinary kernels)
  RtcOption sky_light_kernels{0.0};    // != 0: the sky-light kernels even on a handle without a sky light, the gain zero (tests: against the handle's ordinary kernels)
  RtcOption indirect_kernels{0.0};     // != 0: the indirect kernels even on a handle without an indirect table, the gain zero and no emission (tests: against the handle's ordinary kernels)
  RtcOption mis_kernels{0.0};          // != 0: the MIS kernels even on a handle whose MIS mode is 0 or whose emitter list is empty, the mode zero (tests: against the handle's ordinary kernels)
  RtcOption emitter_kernels{0.0};      // != 0: the emitter kernels even on a handle without an emitter list, the count zero (tests: against the handle's ordinary kernels)
  RtcOption denoise_naive{0.0};        // != 0: rtc_denoise_device runs the literal kernel, one thread per pixel (tests and timing: against the tiled one)
  RtcOption film_naive{0.0};           // != 0: a rtc_film_device that blooms runs the literal kernels, one thread per pixel (tests and timing: against the tiled ones)
  RtcOption robust_naive{0.0};         // != 0: rtc_robust_device runs the literal kernel, one thread per pixel (tests and timing: against the register forms)
  RtcOption build_threads{0.0};        // threads of rtc_scene_create's candidate-BVH build (one top-level group each); 0: as many as the host allows, up to 8
};
inline RtcOptions& rtcOptions() {
  static RtcOptions options;
  return options;
}

template <typename T>
struct DevBuf {
  T* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t upload(const std::vector<T>& v) {
    const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);  // never a null table
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), bytes);
    if (e != hipSuccess) return e;
    if (!v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};

}  // namespace

// conservative world-space bounding sphere (see leafSphere below)
struct Sphere {
  double cx = 0, cy = 0, cz = 0, r = INFINITY;
  bool finite() const { return std::isfinite(r) && std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz); }
};

// The scene's tables in device memory: written by rtc_scene_create, read-only from then on, so a handle and its clones
// (rtc_scene_clone: one handle per frame in flight) share one copy; freed with the last of them.
struct SceneTables {
  std::atomic<int> handles{0};  // handles that share this copy: more than one = frames in flight (kernel choice, rtc_capi.hip)
  // the csg list length any handle of this scene has grown to (rtc_grow_csg_lists): the others - clones, one per frame in
  // flight - take it over at their next launch instead of overflowing, growing and rendering again one by one
  std::atomic<uint32_t> csg_entries_wanted{0};
  DevBuf<uint32_t> roots, kids;
  DevBuf<RootRec> root_recs;
  DevBuf<RootCullPair> root_cull;
  DevBuf<RootBoxPair> root_box;
  DevBuf<float> root_weight;
  DevBuf<uint4> leaf_meta;
  DevBuf<double> xf, tri, trin, node_box, light;
  DevBuf<double> area;  // DevAreaLights::row (rtc_scene_create_with_lights with an area light; else empty)
  DevBuf<DevPattern> pat;
  DevBuf<DevCyl> cyl;
  DevBuf<DevMaterial> mat;
  DevBuf<uint2> node_kids;
  DevBuf<Bvh4Node> bvh;
  DevBuf<Bvh8Node> bvh8;
  DevBuf<BvhLeafRec> bvh_leaf;
  DevBuf<uint32_t> leaf_parent, node_parent, node_info;
  DevBuf<uint2> node_range;
  DevBuf<DevTexMap> tex;
  DevBuf<DevUv> uv;
  DevBuf<DevImage> img;
  DevBuf<float> img_rgb;
  // motion blur (rtc_scene_set_motion): the root tables as uploaded, on the host, from which a handle's motion tables are
  // made; the zero displacements of a static handle under option "motion_kernels"; and zero area rows, with which a
  // point-only light table goes through the motion kernels (every row says "point light")
  std::vector<RootRec> h_root_recs;
  std::vector<RootCullPair> h_root_cull;
  std::vector<RootBoxPair> h_root_box;
  std::vector<uint32_t> h_root_order;  // table position -> World.objects index
  DevBuf<double> zero_disp, zero_rows;
  // spot lights (rtc_scene_set_spots): which lights are area lights (a cone on one is refused); a handle without cones
  // passes zero_rows to the spot kernels as its spot rows (RTC_SPOT_ROW <= RTC_AREA_ROW: every flag zero)
  std::vector<uint8_t> h_light_area;
  // normal perturbation (rtc_scene_set_bumps): the bump rows of a handle without bumps under the "bump_kernels" option
  // (RTC_BUMP_ROW zeros per material: every kind none)
  DevBuf<double> zero_bump;
  // emitter sampling (rtc_scene_set_emitters): what a handle's emitter list is derived from, on the host - the depth-first
  // leaves' kind | casts_shadow << 8, transform, material and triangle, the inverses' rows and the triangles as uploaded,
  // whether a leaf lies below a csg node, and the World.objects index of the root above it
  std::vector<uint4> h_leaf_meta;
  std::vector<double> h_xf, h_tri;
  std::vector<uint8_t> h_leaf_csg;
  std::vector<uint32_t> h_leaf_root;
};

// A handle's bumps (rtc_scene_set_bumps): DevBumps::row.  Read-only once made: a clone and the band clones share it.
struct BumpTables {
  DevBuf<double> row;
};

// A handle's texture rows (rtc_scene_set_mesh_uvs): DevMeshUvs::row.  Read-only once made: a clone and the band clones share it.
struct MeshUvTables {
  DevBuf<double> row;
};

// A handle's roughness rows and hash key (rtc_scene_set_gloss): DevGloss.  Read-only once made: a clone and the band clones share it.
struct GlossTables {
  DevBuf<double> row;
  unsigned long long key = 0ull;
};

// A handle's occlusion radius rows, hash key and sample count (rtc_scene_set_occlusion): DevOcclusion.  Read-only once made:
// a clone and the band clones share it.
struct OcclusionTables {
  DevBuf<double> row;
  unsigned long long key = 0ull;
  uint32_t samples = 1u;
};

// A handle's shadow-filter rows (rtc_scene_set_shadow_filters): DevShadowFilter::row.  Read-only once made: a clone and the
// band clones share it.
struct ShadowFilterTables {
  DevBuf<double> row;
  std::vector<double> h_row;  // the rows on the host: what the emitter list is derived from
};

// A handle's media (rtc_scene_set_media): DevMedia's absorption rows and atmosphere.  Read-only once made: a clone and the
// band clones share it.
struct MediaTables {
  DevBuf<double> row;
  double fog_density = 0.0;
  double fog_color[3] = {0.0, 0.0, 0.0};
};

// A handle's environment (rtc_scene_set_environment): DevEnvironment's sky and sun rows.  Read-only once made: a clone and
// the band clones share it.
struct EnvironmentTables {
  double rgb[3] = {0.0, 0.0, 0.0};
  uint32_t pattern = 0xFFFFFFFFu, projection = 0u, n_suns = 0u;
  bool sky = false;     // a non-zero colour or a pattern: the miss step runs
  DevBuf<double> sun;   // [n_suns][RTC_ENV_SUN_ROW]; empty without suns
};

// A handle's sky light (rtc_scene_set_sky_light): DevSkyLight's values; nothing on the device.  Read-only once made: a clone
// and the band clones share it.
struct SkyLightTable {
  double gain = 0.0;
  uint32_t samples = 1u;
  unsigned long long key = 0ull;  // rtc_mix64(seed ^ RTC_SKY_LIGHT_SALT)
};

// A handle's indirect light (rtc_scene_set_indirect): DevIndirect's values, and the emission rows on the device (empty:
// no material emits).  Read-only once made: a clone and the band clones share it.
struct IndirectTables {
  double gain = 0.0;
  uint32_t bounces = 0u;
  unsigned long long key = 0ull;  // rtc_mix64(seed ^ RTC_INDIRECT_SALT)
  DevBuf<double> emission;        // [n_materials][3]; empty without rows
  bool emits = false;             // an emission entry is not zero
  std::vector<double> h_emission; // the rows on the host (empty without rows): what the emitter list is derived from
};

// A handle's emitter sampling (rtc_scene_set_emitters): the setter's values, and the list derived from the handle's tables -
// DevEmitters' rows, CDF and leaf bits on the device, and on the host the rows, the CDF and each entry's leaf.  A table with
// an empty list is kept: rtc_scene_set_indirect and rtc_scene_set_shadow_filters derive the list again.  Read-only once made:
// a clone and the band clones share it.
struct EmitterTables {
  uint32_t samples = 1u;
  uint64_t seed = 0u;
  unsigned long long key = 0ull;  // rtc_mix64(seed ^ RTC_EMITTER_SALT)
  uint32_t count = 0u;
  double total = 0.0;
  std::vector<double> h_row, h_cdf;
  std::vector<uint32_t> h_leaf;   // per entry: its depth-first leaf
  DevBuf<double> row, cdf;
  DevBuf<uint32_t> leaf_bits;
  DevBuf<uint32_t> leaf_entry;    // DevMis::leaf_entry: per depth-first leaf, its first entry and its listed faces (rtc_scene_set_emitter_mis)
};

// A handle's spot lights (rtc_scene_set_spots): DevSpots::row.  Read-only once made: a clone and the band clones share it.
struct SpotTables {
  DevBuf<double> row;
};

// A handle's motion (rtc_scene_set_motion): the displacements in table order, and copies of the root tables in which a
// moving root's bounds cover its whole path and its "room" flag is cleared.  Read-only once made: a clone and the band
// clones share them.
struct MotionTables {
  DevBuf<double> disp;             // DevMotion::disp, table order
  DevBuf<RootRec> root_recs;
  DevBuf<RootCullPair> root_cull;
  DevBuf<RootBoxPair> root_box;
  float cull_cmax = 0.0f, cull_bmax = 0.0f;
  std::vector<uint8_t> moves;      // per World.objects index: a displacement that is not zero
};

constexpr uint32_t RTC_MAX_HOST_BANDS = 4;

// The render kernels' launch families, lowest priority first: a launch runs the highest family whose condition holds
// (family() in rtc_capi.hip, which also names every family's kernel pair and its arguments - forFamilyKernel).  Each takes
// the arguments of the one below and, but for TORUS, one more.
enum class Family : uint32_t { BASE, MS, MOTION, SPOT, BUMP, TORUS, MESHUV, GLOSS, OCCL, SFILT, MEDIA, ENV, SKYL, INDIR };
// The emitter family (rtc_scene_set_emitters) heads the list: the value above INDIR, the indirect family's arguments and
// DevEmitters.  Named beside the enumeration, whose text the indirect family's tests pin.
constexpr Family kFamilyEmit = static_cast<Family>(static_cast<uint32_t>(Family::INDIR) + 1u);
// The MIS family (rtc_scene_set_emitter_mis) heads the list in its turn: the emitter family's arguments and DevMis.
constexpr Family kFamilyMis = static_cast<Family>(static_cast<uint32_t>(kFamilyEmit) + 1u);
constexpr uint32_t RTC_FAMILIES = 16;
// A family whose occupancy is asked for by the first launch that selects it and not at create: the query loads the unit's
// code object, and a process none of whose handles has a sky light - or an indirect table, or an emitter list - loads,
// allocates and runs what it did before the unit existed.
constexpr bool familyIsLazy(Family f) { return f == Family::SKYL || f == Family::INDIR || f == kFamilyEmit || f == kFamilyMis; }

// Resident work-groups per CU of every family's kernels, [family][tables in LDS ? 0 : 1], and whether they have been asked
// for (at create, or for a lazy family at its first launch).  A clone takes its source's.
struct FamilyOccupancy {
  uint32_t blocks_per_cu[RTC_FAMILIES][2];
  bool known[RTC_FAMILIES] = {};
  FamilyOccupancy() {
    for (auto& pair : blocks_per_cu) pair[0] = pair[1] = 1;  // (until asked for: one work-group, as every answer is at least)
  }
  uint32_t& at(Family f, bool lds) { return blocks_per_cu[static_cast<uint32_t>(f)][lds ? 0 : 1]; }
  uint32_t at(Family f, bool lds) const { return blocks_per_cu[static_cast<uint32_t>(f)][lds ? 0 : 1]; }
};

struct rtc_scene {
  int device = 0;
  hipStream_t stream = nullptr;
  DevScene dev{};
  DevStats* d_stats = nullptr;  // two, used alternately (see DevStats)
  uint32_t stats_parity = 0;    // which of the two the last launch counted in
  double* d_frame = nullptr;  // staging for rtc_render (host output)
  size_t frame_capacity = 0;  // in doubles
  std::shared_ptr<SceneTables> tab;  // the scene in device memory (`dev` points into it): shared with the handle's clones
  bool has_csg = false;
  bool ext_kernel = false;         // csg nodes or texture maps: the *_ext kernels
  bool simple_kernel = false;      // only top-level spheres / planes / cubes: the `simple` kernel
  bool flat_kernel = false;        // no groups at all (any leaf kind): the `flat` kernel
  const char* last_kernel = "";   // name of the render kernel of the last launch (rtc_last_kernel_name)
  bool area_kernel = false;        // World.lights has an area light: the area kernels, with `area` as their extra argument
  DevAreaLights area{};            // rows (in SceneTables::area) and this handle's jitter seed (rtc_scene_set_light_seed)
  rtc_sampling sampling_desc{1u, 0u, 0.0, 1.0, 0ull};  // rtc_scene_set_sampling (a clone starts with its source's)
  DevSampling sampling{0ull, 1.0, 0.0, 1.0, 1u, 1u, 0u};  // ... as the sampling kernels' argument
  bool sampling_on = false;        // not the default: the sampling kernels
  uint32_t sample_pass = 0;        // rtc_scene_set_sample_pass (a clone starts with its source's); not 0: the sampling kernels
  double* d_accum_partials = nullptr;  // rtc_scene_accumulate_device's per-block noise partials, and the total behind them
  size_t accum_partials_capacity = 0;  // doubles
  double* d_adaptive_frame = nullptr;  // rtc_scene_adaptive_step's compact tile frame, and its size in doubles
  size_t adaptive_frame_capacity = 0;
  std::vector<uint32_t> h_adaptive_list;  // ... and the active list it read back
  std::shared_ptr<const MotionTables> motion;  // rtc_scene_set_motion; null: static (a clone starts with its source's)
  std::shared_ptr<const SpotTables> spots;  // rtc_scene_set_spots; null: no cones (a clone starts with its source's)
  std::shared_ptr<const BumpTables> bumps;  // rtc_scene_set_bumps; null: no bumps (a clone starts with its source's)
  bool has_torus = false;          // a leaf of the world is a torus (RTC_TORUS): the torus kernels
  bool has_mesh_map = false;       // a texture map of the scene has mapping RTC_TEX_MESH: the meshuv kernels
  uint32_t n_tris = 0;             // the description's n_tris: what rtc_scene_set_mesh_uvs' table must have
  std::shared_ptr<const MeshUvTables> mesh_uvs;  // rtc_scene_set_mesh_uvs; null: every row six zeros (a clone starts with its source's)
  std::shared_ptr<const GlossTables> gloss;  // rtc_scene_set_gloss; null: no rough row (a clone starts with its source's)
  std::shared_ptr<const OcclusionTables> occlusion;  // rtc_scene_set_occlusion; null: no row with a radius (a clone starts with its source's)
  std::shared_ptr<const ShadowFilterTables> shadow_filters;  // rtc_scene_set_shadow_filters; null: no non-zero row (a clone starts with its source's)
  std::shared_ptr<const MediaTables> media;  // rtc_scene_set_media; null: no absorbing row and no fog (a clone starts with its source's)
  std::shared_ptr<const EnvironmentTables> environment;  // rtc_scene_set_environment; null: no sky and no sun (a clone starts with its source's)
  std::shared_ptr<const SkyLightTable> sky_light;  // rtc_scene_set_sky_light; null: no gain (a clone starts with its source's)
  std::shared_ptr<const IndirectTables> indirect;  // rtc_scene_set_indirect; null: no child and no emission (a clone starts with its source's)
  std::shared_ptr<const EmitterTables> emitters;   // rtc_scene_set_emitters; null: no table (a clone starts with its source's)
  bool simple3_ok = false;         // a simple world whose tables fit the three-waves-per-SIMD kernel's LDS (RTC_LDS3_*)
  void* d_csg_buf = nullptr;       // DevPixelMap::csg_buf, only for scenes with csg nodes
  size_t csg_buf_capacity = 0;     // bytes
  uint32_t csg_entries_ok = RTC_CSG_ENTRIES;  // the list length the buffer was last allocated for (what a failed enlargement falls back to)
  uint32_t csg_needed = 0;         // what the last checked frame said its longest csg list needed (0: no csg list ran out)
  uint32_t max_trav_stack = 0;
  // ---- the general kernel at two or at three waves per SIMD: measured, not guessed (launch(), KernelTune)
  bool box_cull = false;           // a simple world with more cubes than spheres at top level: its kernels reject roots by world boxes (rtc_render_kernel_simple_b / _simple3_b)
  bool general3_ok = false;        // a world with groups, no csg / texture maps, whose tables fit the three-wave kernel's LDS
  uint32_t blocks_per_cu_general3 = 1;
  bool use_three_waves = false;    // the three-wave form of the world's kernel (rtc_render_kernel3 / _simple3 at mid sizes): what the handle's last finished trial DECIDED (clones inherit this, nothing else)
  bool trial_live = false;         // the launch being enqueued is a frame of a running trial ...
  bool trial_three = false;        // ... of this kernel; anything that ends or suspends the trial (a clone made, another pixel map, an option) falls back to the decision
  struct KernelTune {
    enum { kSamples = 3, kRing = 8 };
    int state = 0;                 // 0: no trial yet for this pixel map, 1: trial running, 2: decided
    uint32_t frames = 0;           // trial frames enqueued
    float best[2] = {0.0f, 0.0f};  // fastest frame seen per kernel (two waves, three waves), ms
    uint32_t n[2] = {0, 0};        // samples resolved per kernel
    bool switched = false;         // the frame that changes to the three-wave kernel (and measures for its schedule) has been enqueued
    uint32_t sched_before = 0;     // ... the schedule buffer the two-wave samples ran, and how many schedules had been packed then
    uint32_t packs_at_switch = 0;
    hipEvent_t ev[kRing][2] = {};  // timing events around the render kernel of the trial frames (created on first use)
    int which[kRing] = {};         // which kernel a ring slot timed; -1: slot free / resolved
    std::vector<uint32_t> key;     // the pixel map the trial belongs to
  } tune;
  bool kernel_warm = false;        // the handle's first launch has sent the render kernel ahead once with no work (launch())
  uint32_t n_cus = 0, blocks_per_cu_simple3 = 1;
  FamilyOccupancy occupancy;       // resident work-groups per CU of every family's kernels (BASE: the world's own kernel, two waves per SIMD)
  // ---- the schedule (DevPixelMap::order): two device buffers, used alternately.  d_sched[sched_cur] is what the next
  // launch runs; a measuring launch is followed by the packer's launches, which pack the other buffer from what the
  // launch measured (the first launch of a pixel map: from rtc_estimate_kernel's guesses), and the buffers swap - no host
  // in the loop, nothing is read back.
  uint32_t* d_sched[2] = {nullptr, nullptr};
  size_t sched_capacity = 0;              // words per buffer
  uint32_t sched_cur = 0;
  DevSchedInfo* d_sched_info = nullptr;   // [2], beside the buffers: the packet count of each (DevPixelMap::n_units_dev)
  DevPackState* d_pack_state = nullptr;   // the packer's histogram and totals
  bool sched_valid = false;               // d_sched[sched_cur] holds a schedule for the pixel map `cost_key`
  rtc_camera sched_cam{};                 // the view (and depth) that schedule was measured with: another view measures again
  uint32_t sched_depth = 0;
  uint32_t n_packs = 0;                   // schedules packed on this handle so far
  uint32_t frames_unmeasured = 0;         // frames of a moving view since the last measured one (updateSchedule)
  uint32_t* d_chunk_time = nullptr;       // the packer's scratch: per-chunk times, sorted chunks
  uint32_t* d_sorted = nullptr;
  DevChunkShape* d_chunk_shape = nullptr; // per chunk: how its rays are spread over its pixels (for the chunks the packer cuts)
  size_t pack_capacity = 0;               // chunks
  // ---- measurements: per-pixel ray counts and per-packet times of a measuring launch
  uint32_t* d_cost = nullptr;
  size_t cost_capacity = 0;
  std::vector<uint32_t> cost_key;  // pixel map the costs / the schedule belong to
  uint32_t* d_chunk_cost = nullptr;  // per-chunk sums of d_cost (rtc_chunk_cost_kernel)
#ifdef RTC_PROFILE
  unsigned long long* d_estimate_oob = nullptr;  // root-table indices of rtc_estimate_kernel outside their allocation (diagnostic builds)
#endif
  size_t chunk_cost_capacity = 0;
  uint32_t* d_packet_time = nullptr;  // per packet of the measured schedule: the time its wave needed (DevPixelMap::packet_time)
  size_t packet_time_capacity = 0;
  // mode-2 pixel maps (rtc_render_tile_list_device): the list of the last such launch, on both sides
  std::vector<uint32_t> h_tile_list;
  uint32_t* d_tile_list = nullptr;
  size_t tile_list_capacity = 0;
  uint32_t tile_list_gen = 0;
  uint32_t measured_regions = 0, measured_chunks_per_region = 0;  // what d_chunk_time describes (rtc_get_tile_costs)
  hipStream_t last_stream = nullptr;  // the stream of the last launch (none yet: nullptr)
  bool stats_zeroed = false;          // the first launch has zeroed d_stats on its stream (initLaunchState)
  hipEvent_t launch_done = nullptr;   // recorded behind everything a launch enqueues; a launch on ANOTHER stream waits for it
  void* d_ray_stack = nullptr;     // DevPixelMap::ray_stack
  size_t ray_stack_capacity = 0;   // bytes
  void* d_media_stack = nullptr;   // DevMedia::stack_ext: the media kernels' fifth quarter of every pending ray (ensureScratch)
  size_t media_stack_capacity = 0; // bytes: a quarter of ray_stack_capacity, or 0 while no media kernel has run
  uint32_t emitter_mis = 0;        // rtc_scene_set_emitter_mis: 0 the switch, 1 the balance heuristic (a clone starts with its source's)
  void* d_mis_carry = nullptr;     // DevMis::carry: cos_b of every pending diffuse child of the MIS kernels (ensureScratch)
  size_t mis_carry_capacity = 0;   // bytes: an eighth of ray_stack_capacity, or 0 while no MIS kernel has run
  // ---- host output of a large frame (rtc_render): rendered in horizontal bands one after the other, each copied to the
  // caller while the next renders.  A band is a pixel map of its own: the lower bands run on clones of this handle (made on
  // first use), which keep their band's schedule from frame to frame.
  std::vector<rtc_scene*> band;
  hipStream_t copy_stream = nullptr;
  hipEvent_t band_done[RTC_MAX_HOST_BANDS] = {};
  bool is_band = false;            // this handle is one of another's band clones (not counted in SceneTables::handles)
  uint32_t last_bands = 1;         // bands of the last frame through rtc_render (1: the last launch was an ordinary one)
};
