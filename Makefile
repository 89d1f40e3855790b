# Native build of the MI355X path tracer.  `make` (or __graft_entry__.build()) builds in-tree:
#   pathtracercuda_amd/lib/libpt_hip.so   HIP kernels + device C ABI (include/pt_hip.h), gfx950
#   pathtracercuda_amd/lib/libpt_host.so  host C++ layer + C ABI (include/pathtracer_amd.hpp, pt_host.h)
#   pathtracercuda_amd/lib/pathtracer     CLI (reference main.cpp headless path)
#   pathtracercuda_amd/lib/fp_exhaustive  all-inputs check of the kernel's fast 1/x and sqrt (GPU)
#   pathtracercuda_amd/lib/dev_functions  the kernel's device functions one by one over input files, for
#                                         tests/test_gpu_dev_functions.py (GPU)
#   pathtracercuda_amd/lib/ssg_stages     the guess, lane and fold code of speculative sample groups stage by
#                                         stage over files, for tests/test_gpu_ssg_stages.py (GPU)
#   pathtracercuda_amd/lib/ray_forms      the slab test, the child-pair test and the object-space transform against
#                                         the packed-FP32 forms they replaced, for tests/test_gpu_ray_forms.py (GPU)
#   pathtracercuda_amd/lib/pk_issue_probe issue cost of packed against plain FP32 instructions (GPU; `make pkprobe`)
#   pathtracercuda_amd/lib/host_sanitize_check  ASan/UBSan mutation check of the host parsers (CPU)
#   pathtracercuda_amd/lib/leaf_forms_check  exact vs fast form of the cube leaf test (CPU; `make leafcheck` runs it)
#   pathtracercuda_amd/lib/launch_plan_check  the launch policy and the build table on the host, for tests/test_launch_plan.py (CPU)
#   pathtracercuda_amd/lib/ctx_state_check  what a context carries between calls on the host, for tests/test_ctx_state.py (CPU)
#   oracle/liboracle.so                   CPU restatement (test infrastructure only)
#   oracle/_ref/libptref.so               the reference's own source built for the host, when a checkout
#                                         of it is at $(REF) (test infrastructure only; oracle/Makefile)
# Every FP unit is built with -ffp-contract=off: the GPU result is compared bit for bit with the
# oracle, and the host-built BVH / transforms / camera feed the GPU directly.
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
ARCH ?= gfx950
LIB := pathtracercuda_amd/lib
SRC := pathtracercuda_amd/csrc
REF ?= $(abspath ../reference)
HOST_SRCS := $(SRC)/host/math_camera.cpp $(SRC)/host/hittable.cpp $(SRC)/host/bvh_build.cpp \
             $(SRC)/host/json_min.cpp $(SRC)/host/scene_json.cpp $(SRC)/host/image_io.cpp \
             $(SRC)/host/renderer.cpp $(SRC)/host/host_capi.cpp
HOST_HDRS := include/pathtracer_amd.hpp include/pt_host.h include/pt_hip.h $(SRC)/host/host_internal.h $(SRC)/host/json_min.h

# -fno-slp-vectorize: the kernel uses no packed FP32 (plain instructions measured faster, DESIGN.md
# §4.1; tools/ray_forms.hip keeps the packed forms as a reference); the SLP
# vectorizer's own pairings bound two scalars of the GGX visibility term into one register tuple
# that the allocator then spilled around a range guard in every GGX shading.  Off: scratch 40 -> 12
# B/lane (no spill inside the loop), +4.6 % on C3 same-box (profiles/r03_slp_ab.json).
# HIPCODEGEN: the flags that decide how a device function compiles.  The stand-alone GPU tools take them
# too, so that pt_math.h and the pt_dev_*.h they include compile there as they do in libpt_hip.so.
HIPCODEGEN ?= --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -mcode-object-version=5
HIPFLAGS ?= $(HIPCODEGEN) -fPIC -fvisibility=hidden -Iinclude -Wall -Wno-unused-result
CXXFLAGS ?= -O2 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC -Iinclude -I$(SRC)/host -Wall -Wextra \
            -Wno-unused-parameter -Wno-missing-field-initializers

all: $(LIB)/libpt_hip.so $(LIB)/libpt_host.so $(LIB)/pathtracer $(LIB)/fp_exhaustive $(LIB)/dev_functions $(LIB)/ssg_stages $(LIB)/ray_forms $(LIB)/pk_issue_probe $(LIB)/host_sanitize_check $(LIB)/leaf_forms_check $(LIB)/launch_plan_check $(LIB)/ctx_state_check oracle

$(LIB):
	mkdir -p $(LIB)

$(LIB)/libpt_hip.so: $(SRC)/pt_kernels.hip $(wildcard $(SRC)/*.h) include/pt_hip.h | $(LIB)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(SRC)/pt_kernels.hip -lrccl

$(LIB)/libpt_host.so: $(HOST_SRCS) $(HOST_HDRS) $(LIB)/libpt_hip.so
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRCS) -L$(LIB) -lpt_hip -lz -Wl,-rpath,'$$ORIGIN'

$(LIB)/pathtracer: $(SRC)/host/cli_main.cpp $(LIB)/libpt_host.so
	$(CXX) $(CXXFLAGS) -o $@ $(SRC)/host/cli_main.cpp -L$(LIB) -lpt_host -lpt_hip -lpthread -Wl,-rpath,'$$ORIGIN'

$(LIB)/fp_exhaustive: tools/fp_exhaustive.hip $(SRC)/pt_math.h | $(LIB)
	$(HIPCC) $(HIPCODEGEN) -o $@ tools/fp_exhaustive.hip

# The kernel's device functions, one operation per launch, over raw input words (tools/dev_functions.hip).
$(LIB)/dev_functions: tools/dev_functions.hip $(SRC)/pt_math.h $(SRC)/pt_dev_tex.h $(SRC)/pt_dev_tonemap.h | $(LIB)
	$(HIPCC) $(HIPCODEGEN) -Wall -o $@ tools/dev_functions.hip

# The sample-group stages on a toy stream (tools/ssg_stages.hip): the kernel's own headers, in its order.
$(LIB)/ssg_stages: tools/ssg_stages.hip $(wildcard $(SRC)/*.h) include/pt_hip.h | $(LIB)
	$(HIPCC) $(HIPCODEGEN) -Wall -o $@ tools/ssg_stages.hip

# The slab test, cb_pair and to_local against their packed-FP32 forms (tools/ray_forms.hip): the kernel's own
# headers, in its order.
$(LIB)/ray_forms: tools/ray_forms.hip $(wildcard $(SRC)/*.h) include/pt_hip.h | $(LIB)
	$(HIPCC) $(HIPCODEGEN) -Wall -o $@ tools/ray_forms.hip

# Cycles per packed and per plain FP32 instruction at 1, 2 and 6 waves per SIMD (tools/pk_issue_probe.hip).
$(LIB)/pk_issue_probe: tools/pk_issue_probe.hip | $(LIB)
	$(HIPCC) $(HIPCODEGEN) -Wall -o $@ tools/pk_issue_probe.hip
pkprobe: $(LIB)/pk_issue_probe
	$(LIB)/pk_issue_probe

oracle:
	$(MAKE) -C oracle REF=$(REF)

# CPU-only sanitizer build of the host parsers (scene JSON, RGBE/PNG decode, BVH build) with a
# mutation driver; run by tests/test_host.py.  Links libpt_hip.so for the symbols only (no GPU call).
SAN_SRCS := $(filter-out $(SRC)/host/host_capi.cpp,$(HOST_SRCS))
$(LIB)/host_sanitize_check: tools/host_sanitize_check.cpp $(SAN_SRCS) $(HOST_HDRS) $(LIB)/libpt_hip.so
	$(CXX) -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -fno-omit-frame-pointer -Iinclude -I$(SRC)/host -o $@ tools/host_sanitize_check.cpp $(SAN_SRCS) \
	  -L$(LIB) -lpt_hip -lz -lpthread -Wl,-rpath,'$$ORIGIN'
sanitize: $(LIB)/host_sanitize_check

# Host check of the cube leaf test's two forms (csrc/pt_leaf_forms.h): a directed grid of special values
# and 10^8 random rays, under ASan/UBSan; about a minute on one core.
$(LIB)/leaf_forms_check: tools/leaf_forms_check.cpp $(SRC)/pt_leaf_forms.h | $(LIB)
	$(CXX) -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -o $@ tools/leaf_forms_check.cpp
leafcheck: $(LIB)/leaf_forms_check
	$(LIB)/leaf_forms_check

# Host view of the launch policy (csrc/pt_launch_plan.h, csrc/pt_builds.h) under ASan/UBSan; run by
# tests/test_launch_plan.py.
$(LIB)/launch_plan_check: tools/launch_plan_check.cpp $(SRC)/pt_launch_plan.h $(SRC)/pt_builds.h | $(LIB)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -o $@ tools/launch_plan_check.cpp

# Host view of the state a context carries between calls (csrc/pt_ctx_state.h) under ASan/UBSan; run by
# tests/test_ctx_state.py.
$(LIB)/ctx_state_check: tools/ctx_state_check.cpp $(SRC)/pt_ctx_state.h $(SRC)/pt_launch_plan.h $(SRC)/pt_builds.h include/pt_hip.h | $(LIB)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	  -o $@ tools/ctx_state_check.cpp

clean:
	rm -f $(LIB)/libpt_hip.so $(LIB)/libpt_host.so $(LIB)/pathtracer
	$(MAKE) -C oracle clean
clean-ref:
	$(MAKE) -C oracle clean-ref

.PHONY: all oracle clean clean-ref sanitize leafcheck pkprobe

# `make -s print-HIPFLAGS`: the flags snapshot builds (tools/snap_rev.sh) reuse
print-%:
	@echo $($*)
