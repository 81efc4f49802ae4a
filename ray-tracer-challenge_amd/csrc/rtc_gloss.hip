// rtc_gloss.hip - the gloss kernels (rtc_scene_set_gloss): rtc_render_kernel_gloss and
// rtc_render_kernel_gloss_bigworld, render_body of rtc_kernels.hip with GLOSS (and MESHUV, TORUS, BUMP, SPOT, MOTION, MS,
// AREA).  The unit implies the meshuv and torus units' code: one family renders a world that holds tori, textured meshes
// and rough materials.  A translation unit of their own: every other unit compiles in the time and to the code it did.
#define RTC_GLOSS_TU
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
