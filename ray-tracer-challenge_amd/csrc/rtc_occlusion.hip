// rtc_occlusion.hip - the occlusion kernels (rtc_scene_set_occlusion): rtc_render_kernel_occl and
// rtc_render_kernel_occl_bigworld, render_body of rtc_kernels.hip with OCCL (and GLOSS, MESHUV, TORUS, BUMP, SPOT, MOTION,
// MS, AREA).  The unit implies the gloss, meshuv and torus units' code: one family renders a world that holds tori, textured
// meshes, rough materials and materials with an occlusion radius.  A translation unit of their own: every other unit
// compiles in the time and to the code it did.
#define RTC_OCCL_TU
#define RTC_GLOSS_TU
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
