// rtc_spot.hip - the spot kernels (rtc_scene_set_spots): rtc_render_kernel_spot and
// rtc_render_kernel_spot_bigworld, render_body of rtc_kernels.hip with SPOT (and MOTION, MS, AREA).  A translation unit of
// their own: rtc_kernels.hip and rtc_motion.hip compile in the time and to the code they did before they existed.
#define RTC_SPOT_TU
#include "rtc_kernels.hip"
