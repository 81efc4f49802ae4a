// rtc_motion.hip - the motion kernels (rtc_scene_set_motion): rtc_render_kernel_motion and
// rtc_render_kernel_motion_bigworld, render_body of rtc_kernels.hip with MOTION.  A translation unit of their own:
// rtc_kernels.hip, which holds every other kernel, compiles in the time and to the code it did before they existed.
#define RTC_MOTION_TU
#include "rtc_kernels.hip"
