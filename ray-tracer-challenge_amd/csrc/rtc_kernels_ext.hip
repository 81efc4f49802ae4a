// rtc_kernels_ext.hip - in the -DRTC_PROFILE diagnostic build, the csg / texture-map, flat and area-light render kernels
// (rtc_render_kernel_ext, _simple_ext, _flat, _flat_ext, _bigworld_ext, _area, _area_bigworld): render_body of
// rtc_kernels.hip in a translation unit of their own, so that the instrumented rtc_kernels.hip does not compile all the
// render kernels in one unit.  The product build keeps those kernels in rtc_kernels.hip, to the byte as before: this unit
// then holds none.
#define RTC_EXT_TU
#include "rtc_kernels.hip"
