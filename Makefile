# Top-level build: the HIP render library, the C++ host library, and (test
# infrastructure) the CPU oracle.  __graft_entry__.build() drives this file.
#
#   ray-tracer-challenge_amd/lib/librtc_hip.so   product: HIP kernels + C ABI (include/rtc.h), gfx950
#   ray-tracer-challenge_amd/lib/librtc_multi.so product: single-process multi-GPU render (include/rtc_multi.h): librtc_hip + RCCL
#   ray-tracer-challenge_amd/lib/librtc_host.so  product: scene model, JSON/OBJ loaders, Camera/World/Canvas API
#   ray-tracer-challenge_amd/lib/rtc_host_kat    product unit tests (reference KATs for the build-time helpers)
#   oracle/build/liboracle.so, oracle_kat        test infrastructure only
#   tests/build/libarea_oracle.so                test infrastructure only: the area-light checker (tests/cpp/area_oracle.cpp)
#   tests/build/libcamera_oracle.so              test infrastructure only: the camera-sampling checker (tests/cpp/camera_oracle.cpp)
#   tests/build/libprogressive_oracle.so         test infrastructure only: the sample-pass checker (tests/cpp/progressive_oracle.cpp)
#   tests/build/libmotion_oracle.so              test infrastructure only: the motion-blur checker (tests/cpp/motion_oracle.cpp)
#   tests/build/libadaptive_oracle.so            test infrastructure only: the adaptive-sampling checker (tests/cpp/adaptive_oracle.cpp)
#   tests/build/libspot_oracle.so                test infrastructure only: the spot-light checker (tests/cpp/spot_oracle.cpp)
#   tests/build/libbump_oracle.so                test infrastructure only: the normal-perturbation checker (tests/cpp/bump_oracle.cpp)
#   tests/build/libtorus_oracle.so               test infrastructure only: the torus checker (tests/cpp/torus_oracle.cpp)
#   tests/build/libtorus_bounds.so               test infrastructure only: rtc_bounds.h's leaf bounds behind a C interface (tests/cpp/torus_bounds_shim.hip)
#   tests/build/libmeshuv_oracle.so              test infrastructure only: the mesh-texture checker (tests/cpp/meshuv_oracle.cpp)
#   tests/build/libgloss_oracle.so               test infrastructure only: the glossy reflection / refraction checker (tests/cpp/gloss_oracle.cpp)
#   tests/build/liboccl_oracle.so                test infrastructure only: the ambient-occlusion checker (tests/cpp/occlusion_oracle.cpp)
#   tests/build/libsfilter_oracle.so             test infrastructure only: the shadow-filter checker (tests/cpp/sfilter_oracle.cpp)
#   tests/build/libmedia_oracle.so               test infrastructure only: the participating-media checker (tests/cpp/media_oracle.cpp)
#   tests/build/libenvironment_oracle.so         test infrastructure only: the environment checker (tests/cpp/environment_oracle.cpp)
#   tests/build/libskylight_oracle.so            test infrastructure only: the sky-light checker (tests/cpp/skylight_oracle.cpp)
#   tests/build/libindirect_oracle.so            test infrastructure only: the indirect-light checker (tests/cpp/indirect_oracle.cpp)
#   tests/build/libemitters_oracle.so            test infrastructure only: the emitter-sampling checker (tests/cpp/emitters_oracle.cpp)
#   tests/build/libmis_oracle.so                 test infrastructure only: the multiple-importance-sampling checker (tests/cpp/mis_oracle.cpp)
#   tests/build/libdenoise_oracle.so             test infrastructure only: the denoiser's checker (tests/cpp/denoise_oracle.cpp)
#   tests/build/libfilm_oracle.so                test infrastructure only: the film stage's checker (tests/cpp/film_oracle.cpp)
#   tests/build/librobust_oracle.so              test infrastructure only: robust accumulation's checker (tests/cpp/robust_oracle.cpp)
#   tests/build/meshuv_kat                       product unit tests: the OBJ parser's texture coordinates and ignored lines (tests/cpp/meshuv_kat_main.cpp)
#
# -ffp-contract=off everywhere: the reference's float mode is strict IEEE
# (SURVEY F10); the GPU path and the oracle must round identically.
ROCM    ?= /opt/rocm
HIPCC   ?= $(ROCM)/bin/hipcc
CXX     ?= g++
PKG     := ray-tracer-challenge_amd
LIB     := $(PKG)/lib

# (EXTRA: -D switches of diagnostic / experimental builds, e.g. make hip EXTRA=-DRTC_PROFILE)
HIPFLAGS := --offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wno-unused-result $(EXTRA)
CXXFLAGS := -std=c++17 -O2 -ffp-contract=off -fPIC -Wall -Wextra

HOST_SRC := $(PKG)/host/rtc_scene.cpp $(PKG)/host/rtc_loader.cpp $(PKG)/host/rtc_flatten.cpp \
            $(PKG)/host/rtc_api.cpp $(PKG)/host/rtc_host_capi.cpp
HOST_HDR := $(wildcard $(PKG)/host/*.hpp) include/rtc.h include/rtc_host.h

all: hip host oracle checker

hip: $(LIB)/librtc_hip.so $(LIB)/librtc_multi.so
host: $(LIB)/librtc_host.so $(LIB)/rtc_host_kat
oracle:
	$(MAKE) -C oracle

# (the area-light checker includes the oracle's sources read-only; -pthread and -O3 as the oracle's own build)
checker: tests/build/libarea_oracle.so tests/build/libcamera_oracle.so tests/build/libprogressive_oracle.so tests/build/libmotion_oracle.so \
         tests/build/libadaptive_oracle.so tests/build/libspot_oracle.so tests/build/libbump_oracle.so \
         tests/build/libtorus_oracle.so tests/build/libtorus_bounds.so tests/build/libmeshuv_oracle.so tests/build/meshuv_kat \
         tests/build/libgloss_oracle.so tests/build/liboccl_oracle.so tests/build/libsfilter_oracle.so \
         tests/build/libmedia_oracle.so tests/build/libenvironment_oracle.so tests/build/libskylight_oracle.so \
         tests/build/libindirect_oracle.so tests/build/libemitters_oracle.so tests/build/libmis_oracle.so tests/build/libdenoise_oracle.so \
         tests/build/libfilm_oracle.so tests/build/librobust_oracle.so
tests/build/libarea_oracle.so: tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -pthread -shared -o $@ tests/cpp/area_oracle.cpp
# (the camera-sampling checker includes the area-light checker, read-only)
tests/build/libcamera_oracle.so: tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/camera_oracle.cpp
# (the sample-pass checker includes the camera-sampling checker, read-only)
tests/build/libprogressive_oracle.so: tests/cpp/progressive_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/progressive_oracle.cpp
# (the motion-blur checker includes the camera-sampling checker, read-only)
tests/build/libmotion_oracle.so: tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/motion_oracle.cpp
# (the adaptive-sampling checker includes the sample-pass checker, read-only)
tests/build/libadaptive_oracle.so: tests/cpp/adaptive_oracle.cpp tests/cpp/progressive_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/adaptive_oracle.cpp
# (the spot-light checker includes the motion-blur checker, read-only)
tests/build/libspot_oracle.so: tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/spot_oracle.cpp
# (the normal-perturbation checker includes the spot-light checker, read-only)
tests/build/libbump_oracle.so: tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/bump_oracle.cpp
# (the torus checker includes the normal-perturbation checker, read-only)
tests/build/libtorus_oracle.so: tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/torus_oracle.cpp
# (the mesh-texture checker includes the torus checker, read-only)
tests/build/libmeshuv_oracle.so: tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/meshuv_oracle.cpp
# (the gloss checker includes the mesh-texture checker, read-only)
tests/build/libgloss_oracle.so: tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/gloss_oracle.cpp
# (the occlusion checker includes the gloss checker, read-only)
tests/build/liboccl_oracle.so: tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/occlusion_oracle.cpp
# (the shadow-filter checker includes the occlusion checker, read-only)
tests/build/libsfilter_oracle.so: tests/cpp/sfilter_oracle.cpp tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/sfilter_oracle.cpp
# (the participating-media checker includes the shadow-filter checker, read-only)
tests/build/libmedia_oracle.so: tests/cpp/media_oracle.cpp tests/cpp/sfilter_oracle.cpp tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/media_oracle.cpp
# (the environment checker includes the participating-media checker, read-only)
tests/build/libenvironment_oracle.so: tests/cpp/environment_oracle.cpp tests/cpp/media_oracle.cpp tests/cpp/sfilter_oracle.cpp tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/environment_oracle.cpp
# (the sky-light checker includes the environment checker, read-only)
tests/build/libskylight_oracle.so: tests/cpp/skylight_oracle.cpp tests/cpp/environment_oracle.cpp tests/cpp/media_oracle.cpp tests/cpp/sfilter_oracle.cpp tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/skylight_oracle.cpp
# (the indirect-light checker includes the sky-light checker, read-only)
tests/build/libindirect_oracle.so: tests/cpp/indirect_oracle.cpp tests/cpp/skylight_oracle.cpp tests/cpp/environment_oracle.cpp tests/cpp/media_oracle.cpp tests/cpp/sfilter_oracle.cpp tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/indirect_oracle.cpp
# (the emitter-sampling checker includes the indirect-light checker, read-only)
tests/build/libemitters_oracle.so: tests/cpp/emitters_oracle.cpp tests/cpp/indirect_oracle.cpp tests/cpp/skylight_oracle.cpp tests/cpp/environment_oracle.cpp tests/cpp/media_oracle.cpp tests/cpp/sfilter_oracle.cpp tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/emitters_oracle.cpp
# (the MIS checker includes the emitter-sampling checker, read-only)
tests/build/libmis_oracle.so: tests/cpp/mis_oracle.cpp tests/cpp/emitters_oracle.cpp tests/cpp/indirect_oracle.cpp tests/cpp/skylight_oracle.cpp tests/cpp/environment_oracle.cpp tests/cpp/media_oracle.cpp tests/cpp/sfilter_oracle.cpp tests/cpp/occlusion_oracle.cpp tests/cpp/gloss_oracle.cpp tests/cpp/meshuv_oracle.cpp tests/cpp/torus_oracle.cpp tests/cpp/bump_oracle.cpp tests/cpp/spot_oracle.cpp tests/cpp/motion_oracle.cpp tests/cpp/camera_oracle.cpp tests/cpp/area_oracle.cpp oracle/oracle_capi.cpp oracle/rtc_oracle.hpp oracle/rtc_oracle_scene.hpp include/rtc.h
	mkdir -p tests/build
	$(CXX) -std=c++17 -O3 -ffp-contract=off -fPIC -Wall -Wextra -Wno-subobject-linkage -pthread -shared -o $@ tests/cpp/mis_oracle.cpp
# (the denoiser's checker: include/rtc.h's contract as plain loops in doubles; it links nothing of the product)
tests/build/libdenoise_oracle.so: tests/cpp/denoise_oracle.cpp
	mkdir -p tests/build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fPIC -Wall -Wextra -pthread -shared -o $@ tests/cpp/denoise_oracle.cpp
# (the film stage's checker, likewise)
tests/build/libfilm_oracle.so: tests/cpp/film_oracle.cpp
	mkdir -p tests/build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fPIC -Wall -Wextra -pthread -shared -o $@ tests/cpp/film_oracle.cpp
# (robust accumulation's checker, likewise)
tests/build/librobust_oracle.so: tests/cpp/robust_oracle.cpp
	mkdir -p tests/build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fPIC -Wall -Wextra -pthread -shared -o $@ tests/cpp/robust_oracle.cpp
# (the OBJ parser's `vt` lines at parser level, against the product's host library as rtc_host_kat is)
tests/build/meshuv_kat: tests/cpp/meshuv_kat_main.cpp $(LIB)/librtc_host.so $(HOST_HDR)
	mkdir -p tests/build
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/meshuv_kat_main.cpp -L$(LIB) -lrtc_host -lrtc_hip -Wl,-rpath,'$$ORIGIN/../../$(LIB)'
# (the product's conservative leaf bounds, rtc_bounds.h - host code -, for the test that no checker entry lies outside them)
tests/build/libtorus_bounds.so: tests/cpp/torus_bounds_shim.hip $(PKG)/csrc/rtc_bounds.h $(PKG)/csrc/rtc_host_internal.h $(PKG)/csrc/rtc_device.h include/rtc.h
	mkdir -p tests/build
	$(HIPCC) $(HIPFLAGS) -Wno-unused-function -shared -o $@ tests/cpp/torus_bounds_shim.hip

$(LIB):
	mkdir -p $(LIB)

# (the compiler's resource-usage remarks of the product build are kept: lib/kernel_resources.json - registers, spills,
# scratch bytes per lane, LDS of every kernel - is what bench.py quotes as roofline.scratch_bytes_per_lane)
# (the motion kernels, rtc_motion.hip, the spot kernels, rtc_spot.hip, the bump kernels, rtc_bump.hip, the torus kernels, rtc_torus.hip, the meshuv kernels, rtc_meshuv.hip, the gloss kernels, rtc_gloss.hip, the occlusion kernels, rtc_occlusion.hip, the shadow-filter kernels, rtc_shadowfilter.hip, the media kernels, rtc_media.hip, the environment kernels, rtc_environment.hip, the sky-light kernels, rtc_skylight.hip, the indirect kernels, rtc_indirect.hip, the emitter kernels, rtc_emitters.hip, and the MIS kernels, rtc_mis.hip, are render_body
# of rtc_kernels.hip in translation units of their own: the file of every other kernel compiles as before; the JSON holds the kernels of all)
$(LIB)/rtc_kernels.o: $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_kernels.remarks || (grep -v "remark:" $(LIB)/rtc_kernels.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_kernels.remarks >&2 || true

$(LIB)/rtc_motion.o: $(PKG)/csrc/rtc_motion.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_motion.remarks || (grep -v "remark:" $(LIB)/rtc_motion.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_motion.remarks >&2 || true

$(LIB)/rtc_spot.o: $(PKG)/csrc/rtc_spot.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_spot.remarks || (grep -v "remark:" $(LIB)/rtc_spot.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_spot.remarks >&2 || true

$(LIB)/rtc_bump.o: $(PKG)/csrc/rtc_bump.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_bump.remarks || (grep -v "remark:" $(LIB)/rtc_bump.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_bump.remarks >&2 || true

$(LIB)/rtc_torus.o: $(PKG)/csrc/rtc_torus.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_torus.remarks || (grep -v "remark:" $(LIB)/rtc_torus.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_torus.remarks >&2 || true

$(LIB)/rtc_meshuv.o: $(PKG)/csrc/rtc_meshuv.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_meshuv.remarks || (grep -v "remark:" $(LIB)/rtc_meshuv.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_meshuv.remarks >&2 || true

$(LIB)/rtc_gloss.o: $(PKG)/csrc/rtc_gloss.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_gloss.remarks || (grep -v "remark:" $(LIB)/rtc_gloss.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_gloss.remarks >&2 || true

$(LIB)/rtc_occlusion.o: $(PKG)/csrc/rtc_occlusion.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_occlusion.remarks || (grep -v "remark:" $(LIB)/rtc_occlusion.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_occlusion.remarks >&2 || true

$(LIB)/rtc_shadowfilter.o: $(PKG)/csrc/rtc_shadowfilter.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_shadowfilter.remarks || (grep -v "remark:" $(LIB)/rtc_shadowfilter.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_shadowfilter.remarks >&2 || true

$(LIB)/rtc_media.o: $(PKG)/csrc/rtc_media.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_media.remarks || (grep -v "remark:" $(LIB)/rtc_media.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_media.remarks >&2 || true

$(LIB)/rtc_environment.o: $(PKG)/csrc/rtc_environment.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_environment.remarks || (grep -v "remark:" $(LIB)/rtc_environment.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_environment.remarks >&2 || true

$(LIB)/rtc_skylight.o: $(PKG)/csrc/rtc_skylight.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_skylight.remarks || (grep -v "remark:" $(LIB)/rtc_skylight.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_skylight.remarks >&2 || true

$(LIB)/rtc_indirect.o: $(PKG)/csrc/rtc_indirect.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_indirect.remarks || (grep -v "remark:" $(LIB)/rtc_indirect.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_indirect.remarks >&2 || true

$(LIB)/rtc_emitters.o: $(PKG)/csrc/rtc_emitters.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_emitters.remarks || (grep -v "remark:" $(LIB)/rtc_emitters.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_emitters.remarks >&2 || true

$(LIB)/rtc_mis.o: $(PKG)/csrc/rtc_mis.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_mis.remarks || (grep -v "remark:" $(LIB)/rtc_mis.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_mis.remarks >&2 || true

# (rtc_kernels_ext.hip: in the -DRTC_PROFILE diagnostic build the csg / texture-map, flat and area-light kernels, in a
# unit of their own so that the instrumented render kernels do not compile in one; in the product build it holds none)
$(LIB)/rtc_kernels_ext.o: $(PKG)/csrc/rtc_kernels_ext.hip $(PKG)/csrc/rtc_kernels.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_kernels_ext.remarks || (grep -v "remark:" $(LIB)/rtc_kernels_ext.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_kernels_ext.remarks >&2 || true

$(LIB)/kernel_resources.json: $(LIB)/rtc_kernels.o $(LIB)/rtc_kernels_ext.o $(LIB)/rtc_motion.o $(LIB)/rtc_spot.o $(LIB)/rtc_bump.o $(LIB)/rtc_torus.o $(LIB)/rtc_meshuv.o $(LIB)/rtc_gloss.o $(LIB)/rtc_occlusion.o $(LIB)/rtc_shadowfilter.o $(LIB)/rtc_media.o $(LIB)/rtc_environment.o $(LIB)/rtc_skylight.o $(LIB)/rtc_indirect.o $(LIB)/rtc_emitters.o $(LIB)/rtc_mis.o $(LIB)/rtc_denoise.o $(LIB)/rtc_film.o $(LIB)/rtc_robust.o tools/kernel_resources.py
	cat $(LIB)/rtc_kernels.remarks $(LIB)/rtc_kernels_ext.remarks $(LIB)/rtc_motion.remarks $(LIB)/rtc_spot.remarks $(LIB)/rtc_bump.remarks $(LIB)/rtc_torus.remarks $(LIB)/rtc_meshuv.remarks $(LIB)/rtc_gloss.remarks $(LIB)/rtc_occlusion.remarks $(LIB)/rtc_shadowfilter.remarks $(LIB)/rtc_media.remarks $(LIB)/rtc_environment.remarks $(LIB)/rtc_skylight.remarks $(LIB)/rtc_indirect.remarks $(LIB)/rtc_emitters.remarks $(LIB)/rtc_mis.remarks $(LIB)/rtc_denoise.remarks $(LIB)/rtc_film.remarks $(LIB)/rtc_robust.remarks > $(LIB)/render_kernels.remarks
	python3 tools/kernel_resources.py --from-remarks $(LIB)/render_kernels.remarks --json $@

$(LIB)/rtc_capi.o: $(PKG)/csrc/rtc_capi.hip $(wildcard $(PKG)/csrc/*.h) include/rtc.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# (progressive rendering's accumulation: a translation unit of its own, so that the render kernels' code objects stay)
$(LIB)/rtc_accum.o: $(PKG)/csrc/rtc_accum.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# (adaptive sampling's per-tile accumulation and stopping rule: a translation unit of its own, for the same reason)
$(LIB)/rtc_adaptive.o: $(PKG)/csrc/rtc_adaptive.hip $(PKG)/csrc/rtc_device.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# (the denoiser's kernels: a translation unit of its own, for the same reason; its resource remarks join the JSON)
$(LIB)/rtc_denoise.o: $(PKG)/csrc/rtc_denoise.hip include/rtc.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_denoise.remarks || (grep -v "remark:" $(LIB)/rtc_denoise.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_denoise.remarks >&2 || true

# (the film stage's kernels: a translation unit of its own, likewise)
$(LIB)/rtc_film.o: $(PKG)/csrc/rtc_film.hip include/rtc.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_film.remarks || (grep -v "remark:" $(LIB)/rtc_film.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_film.remarks >&2 || true

# (robust accumulation's resolve kernels: a translation unit of its own, likewise)
$(LIB)/rtc_robust.o: $(PKG)/csrc/rtc_robust.hip include/rtc.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o $@ $< 2> $(LIB)/rtc_robust.remarks || (grep -v "remark:" $(LIB)/rtc_robust.remarks >&2; exit 1)
	@grep -v "remark:\|remarks generated\|\^\|^ *[0-9]* |" $(LIB)/rtc_robust.remarks >&2 || true

$(LIB)/librtc_hip.so: $(LIB)/rtc_kernels.o $(LIB)/rtc_kernels_ext.o $(LIB)/rtc_motion.o $(LIB)/rtc_spot.o $(LIB)/rtc_bump.o $(LIB)/rtc_torus.o $(LIB)/rtc_meshuv.o $(LIB)/rtc_gloss.o $(LIB)/rtc_occlusion.o $(LIB)/rtc_shadowfilter.o $(LIB)/rtc_media.o $(LIB)/rtc_environment.o $(LIB)/rtc_skylight.o $(LIB)/rtc_indirect.o $(LIB)/rtc_emitters.o $(LIB)/rtc_mis.o $(LIB)/rtc_capi.o $(LIB)/rtc_accum.o $(LIB)/rtc_adaptive.o $(LIB)/rtc_denoise.o $(LIB)/rtc_film.o $(LIB)/rtc_robust.o | $(LIB)/kernel_resources.json
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $^

$(LIB)/librtc_multi.so: $(PKG)/csrc/rtc_multi.hip include/rtc_multi.h include/rtc.h $(LIB)/librtc_hip.so
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $< -L$(LIB) -lrtc_hip -L$(ROCM)/lib -lrccl -Wl,-rpath,'$$ORIGIN'

$(LIB)/librtc_host.so: $(HOST_SRC) $(HOST_HDR) $(LIB)/librtc_hip.so
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRC) -L$(LIB) -lrtc_hip -lz -Wl,-rpath,'$$ORIGIN'

$(LIB)/rtc_host_kat: tests/cpp/host_kat_main.cpp $(LIB)/librtc_host.so $(HOST_HDR)
	$(CXX) $(CXXFLAGS) -o $@ tests/cpp/host_kat_main.cpp -L$(LIB) -lrtc_host -lrtc_hip -Wl,-rpath,'$$ORIGIN'

clean:
	rm -rf $(LIB) tests/build
	$(MAKE) -C oracle clean

.PHONY: all hip host oracle checker clean
