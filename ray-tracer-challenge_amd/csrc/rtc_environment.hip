// rtc_environment.hip - the environment kernels (rtc_scene_set_environment): rtc_render_kernel_env and
// rtc_render_kernel_env_bigworld, render_body of rtc_kernels.hip with ENV (and MEDIA, SFILT, OCCL, GLOSS, MESHUV, TORUS,
// BUMP, SPOT, MOTION, MS, AREA).  The unit implies the media, shadow-filter, occlusion, gloss, meshuv and torus units' code:
// one family renders a world under a sky, lit by suns, whatever else it holds.  A translation unit of their own: every other
// unit compiles in the time and to the code it did.
#define RTC_ENV_TU
#define RTC_MEDIA_TU
#define RTC_SFILT_TU
#define RTC_OCCL_TU
#define RTC_GLOSS_TU
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
