// rtc_media.hip - the media kernels (rtc_scene_set_media): rtc_render_kernel_media and
// rtc_render_kernel_media_bigworld, render_body of rtc_kernels.hip with MEDIA (and SFILT, OCCL, GLOSS, MESHUV, TORUS, BUMP,
// SPOT, MOTION, MS, AREA).  The unit implies the shadow-filter, occlusion, gloss, meshuv and torus units' code: one family
// renders a world that holds tori, textured meshes, rough materials, occlusion radii, materials that filter light and
// materials that absorb it.  A translation unit of their own: every other unit compiles in the time and to the code it did.
#define RTC_MEDIA_TU
#define RTC_SFILT_TU
#define RTC_OCCL_TU
#define RTC_GLOSS_TU
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
