// rtc_mis.hip - the MIS kernels (rtc_scene_set_emitter_mis): rtc_render_kernel_mis and
// rtc_render_kernel_mis_bigworld, render_body of rtc_kernels.hip with MIS (and EMIT, INDIRECT, SKYL, ENV, MEDIA, SFILT, OCCL,
// GLOSS, MESHUV, TORUS, BUMP, SPOT, MOTION, MS, AREA).  The unit implies the emitter unit's code and every unit's below it:
// one family renders a world whose emitter samples and diffuse children are combined by the balance heuristic, whatever else
// it holds.  A translation unit of their own: every other unit compiles in the time and to the code it did.
#define RTC_MIS_TU
#define RTC_EMIT_TU
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
