// rtc_skylight.hip - the sky-light kernels (rtc_scene_set_sky_light): rtc_render_kernel_skyl and
// rtc_render_kernel_skyl_bigworld, render_body of rtc_kernels.hip with SKYL (and ENV, MEDIA, SFILT, OCCL, GLOSS, MESHUV,
// TORUS, BUMP, SPOT, MOTION, MS, AREA).  The unit implies the environment unit's code and every unit's below it: one family
// renders a world lit by its sky, whatever else it holds.  A translation unit of their own: every other unit compiles in
// the time and to the code it did.
#define RTC_SKYL_TU
#define RTC_ENV_TU
#define RTC_MEDIA_TU
#define RTC_SFILT_TU
#define RTC_OCCL_TU
#define RTC_GLOSS_TU
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
