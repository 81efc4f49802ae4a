// rtc_indirect.hip - the indirect kernels (rtc_scene_set_indirect): rtc_render_kernel_indir and
// rtc_render_kernel_indir_bigworld, render_body of rtc_kernels.hip with INDIRECT (and SKYL, ENV, MEDIA, SFILT, OCCL, GLOSS,
// MESHUV, TORUS, BUMP, SPOT, MOTION, MS, AREA).  The unit implies the sky-light unit's code and every unit's below it: one
// family renders a world with diffuse bounce rays and emissive materials, whatever else it holds.  A translation unit of
// their own: every other unit compiles in the time and to the code it did.
#define RTC_INDIR_TU
#define RTC_SKYL_TU
#define RTC_ENV_TU
#define RTC_MEDIA_TU
#define RTC_SFILT_TU
#define RTC_OCCL_TU
#define RTC_GLOSS_TU
#define RTC_MESHUV_TU
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
