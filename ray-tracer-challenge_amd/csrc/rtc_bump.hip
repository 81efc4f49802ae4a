// rtc_bump.hip - the bump kernels (rtc_scene_set_bumps): rtc_render_kernel_bump and
// rtc_render_kernel_bump_bigworld, render_body of rtc_kernels.hip with BUMP (and SPOT, MOTION, MS, AREA).  A translation
// unit of their own: rtc_kernels.hip, rtc_motion.hip and rtc_spot.hip compile in the time and to the code they did before
// they existed.
#define RTC_BUMP_TU
#include "rtc_kernels.hip"
