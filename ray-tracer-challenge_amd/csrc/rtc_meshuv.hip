// rtc_meshuv.hip - the meshuv kernels (RTC_TEX_MESH): rtc_render_kernel_meshuv and
// rtc_render_kernel_meshuv_bigworld, render_body of rtc_kernels.hip with MESHUV (and TORUS, BUMP, SPOT, MOTION, MS, AREA).
// The unit implies the torus unit's code - leaf kind 7 and its solver -: one family renders a world that holds tori and
// textured meshes.  A translation unit of their own: every other unit compiles in the time and to the code it did.
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
