// rtc_torus.hip - the torus kernels (RTC_TORUS): rtc_render_kernel_torus and
// rtc_render_kernel_torus_bigworld, render_body of rtc_kernels.hip with TORUS (and BUMP, SPOT, MOTION, MS, AREA), and the
// quartic solver they call.  A translation unit of their own: rtc_kernels.hip, rtc_motion.hip, rtc_spot.hip and
// rtc_bump.hip compile in the time and to the code they did before they existed.
#define RTC_TORUS_TU
#include "rtc_kernels.hip"
