// rtc_shadowfilter.hip - the shadow-filter kernels (rtc_scene_set_shadow_filters):
// rtc_render_kernel_sfilter and rtc_render_kernel_sfilter_bigworld, render_body of rtc_kernels.hip with SFILT (and OCCL,
// GLOSS, MESHUV, TORUS, BUMP, SPOT, MOTION, MS, AREA).  The unit implies the occlusion, gloss, meshuv and torus units' code:
// one family renders a world that holds tori, textured meshes, rough materials, occlusion radii and materials that filter
// light.  A translation unit of their own: every other unit compiles in the time and to the code it did.
#define RTC_SFILT_TU
#define RTC_OCCL_TU
#define RTC_GLOSS_TU
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
