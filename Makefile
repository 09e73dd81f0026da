# Build of the fifteen shared libraries (no cmake: plain make + hipcc/g++).
#   v-img_amd/lib/libvimg_hip.so   hand-written gfx950 kernels + C ABI   (the product)
#   v-img_amd/lib/libvimg_filter.so  scene-free filters over device frames (the a-trous denoiser)       }
#   v-img_amd/lib/libvimg_temporal.so  scene-free temporal accumulation over device frames (reprojection) } the frame
#   v-img_amd/lib/libvimg_varfilter.so  scene-free variance-guided a-trous filter over device frames      } libraries
#   v-img_amd/lib/libvimg_moments.so  scene-free temporal accumulation with luminance moments and variance }
#   v-img_amd/lib/libvimg_infill.so  scene-free reconstruction of sparsely sampled frames from the guides }
#   v-img_amd/lib/libvimg_wtemporal.so  scene-free temporal accumulation with a weight per pixel          }
#   v-img_amd/lib/libvimg_antilag.so  scene-free shortening of a history where the picture has changed    }
#   v-img_amd/lib/libvimg_motion.so  scene-free previous-world positions of moved geometry, from tables    }
#   v-img_amd/lib/libvimg_despeckle.so  scene-free clamp of fireflies in a frame before it is filtered     }
#   v-img_amd/lib/libvimg_exposure.so  scene-free histogram auto-exposure, its state in device memory     }
#   v-img_amd/lib/libvimg_demand.so  scene-free sampling mask of a sparse preview, from the history's lengths }
#   v-img_amd/lib/libvimg_rectify.so  scene-free clamp of a long history to a short history beside it      }
#   v-img_amd/lib/libvimg_host.so  host side: scene loading, SAH BVH, post (the product's host)
#   oracle/liboracle.so            CPU restatement of the reference path  (test infrastructure)
ROOT    := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
ARCH    ?= gfx950

LIBDIR  := v-img_amd/lib
HOSTSRC := $(wildcard v-img_amd/host/*.cpp)
HOSTHDR := $(wildcard v-img_amd/host/*.hpp) $(wildcard include/*.h)
HIPSRC  := $(wildcard v-img_amd/csrc/*.hip)
HIPHDR  := $(wildcard v-img_amd/csrc/*.h) $(wildcard include/*.h)
ORASRC  := $(wildcard oracle/*.cpp)
ORAHDR  := $(wildcard oracle/*.h) $(wildcard include/*.h)
FRAMELIBS := filter temporal varfilter
FRAMELIBS += moments
FRAMELIBS += infill
FRAMELIBS += wtemporal
FRAMELIBS += antilag
FRAMELIBS += motion
FRAMELIBS += despeckle
FRAMELIBS += exposure
FRAMELIBS += demand
FRAMELIBS += rectify

# -ffp-contract=off everywhere: +,-,*,/,sqrt must round identically on CPU and GPU; fused
# multiply-adds appear only where the reference writes std::fma.
HOSTFLAGS := -std=c++20 -O2 -fPIC -shared -ffp-contract=off -fopenmp -Wall -Iinclude
ORAFLAGS  := -std=c++20 -O3 -march=x86-64-v3 -fPIC -shared -ffp-contract=off -pthread -Wall -Iinclude
HIPFLAGS  := --offload-arch=$(ARCH) -std=c++20 -O3 -fPIC -shared -ffp-contract=off -fno-slp-vectorize \
             -fno-fast-math -Iinclude -Wall -Wno-unused-function

all: host hip $(FRAMELIBS) oracle oracle-avx2 cli
host: $(LIBDIR)/libvimg_host.so
hip: $(LIBDIR)/libvimg_hip.so
oracle: oracle/liboracle.so
cli: v-img_amd/bin/vimg-amd

$(LIBDIR)/libvimg_host.so: $(HOSTSRC) $(HOSTHDR) Makefile
	@mkdir -p $(LIBDIR)
	$(CXX) $(HOSTFLAGS) $(HOSTSRC) -o $@

# one object per translation unit (make -j compiles them side by side): the host units of the ABI, one
# unit per render kernel family, the BVH builders
HIPCFLAGS := $(filter-out -shared,$(HIPFLAGS)) -c
OBJDIR    := build/hip
HIPOBJ    := $(patsubst v-img_amd/csrc/%.hip,$(OBJDIR)/%.o,$(HIPSRC))
$(OBJDIR)/%.o: v-img_amd/csrc/%.hip $(HIPHDR) Makefile
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPCFLAGS) $< -o $@
# render_cu_kernel is ONE persistent loop around every stage: MachineLICM hoists the constants of all
# of them (the f64 polynomial coefficients of acos / atan2 / pow ...) in front of the loop, where they
# no longer fit the register file: 533 spilled registers and 700 bytes of scratch per lane with the
# pass, 80 / 72 without (tools/kres.sh)
$(OBJDIR)/k_cu.o $(OBJDIR)/k_cu_early.o $(OBJDIR)/k_cu_diag.o $(OBJDIR)/k_cu_plain.o $(OBJDIR)/k_cu_plain_early.o \
$(OBJDIR)/k_cu_plain_other.o $(OBJDIR)/k_cu_plain_other_early.o: \
    HIPCFLAGS += -mllvm -disable-machine-licm
# feature_kernel: the same pass hoists the constants of generate_ray, the hit record and the texture lookup in
# front of the sample loop: 201 / 182 registers (TEX / not) and two waves per SIMD with it, 99 / 84 and four /
# five without, no scratch either way
$(OBJDIR)/k_feature.o: HIPCFLAGS += -mllvm -disable-machine-licm
$(LIBDIR)/libvimg_hip.so: $(HIPOBJ)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(HIPOBJ) -o $@

# the frame libraries, one per name in FRAMELIBS: libvimg_<name>.so from its own sources
# v-img_amd/<name>/*.hip (NOT the csrc wildcard of libvimg_hip.so), the shared host skeleton v-img_amd/frames/*.h and
# the public headers; each links the HIP runtime and nothing of the other libraries.  The same HIPFLAGS: their
# bit-level contracts rest on -ffp-contract=off, -fno-fast-math and hipcc's correctly rounded divide.  No
# -disable-machine-licm: their kernels have no loop left after unrolling
FRAMEHDR  := $(wildcard v-img_amd/frames/*.h) $(wildcard include/*.h)
$(FRAMELIBS): %: $(LIBDIR)/libvimg_%.so
.SECONDEXPANSION:
$(FRAMELIBS:%=$(LIBDIR)/libvimg_%.so): $(LIBDIR)/libvimg_%.so: $$(wildcard v-img_amd/$$*/*.hip) $(FRAMEHDR) Makefile
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) $(filter %.hip,$^) -o $@

# C++ host program (the counterpart of the reference's main): links the three product libraries by rpath
v-img_amd/bin/vimg-amd: v-img_amd/cli/main.cpp $(LIBDIR)/libvimg_host.so $(LIBDIR)/libvimg_hip.so $(LIBDIR)/libvimg_filter.so Makefile
	@mkdir -p v-img_amd/bin
	$(HIPCC) -std=c++20 -O2 -Iinclude v-img_amd/cli/main.cpp -L$(LIBDIR) -lvimg_host -lvimg_hip -lvimg_filter \
	  -Wl,-rpath,'$$ORIGIN/../lib' -o $@

oracle/liboracle.so: $(ORASRC) $(ORAHDR) Makefile
	$(CXX) $(ORAFLAGS) $(ORASRC) -o $@

# same oracle with the reference's own float libm calls (cosf, acosf ...) instead of the
# double-evaluated forms the GPU can reproduce bit for bit; used by one CPU test.
oracle/liboracle_libmf.so: $(ORASRC) $(ORAHDR) Makefile
	$(CXX) $(ORAFLAGS) -DORACLE_LIBM_FLOAT=1 $(ORASRC) -o $@

# TIMING build of the oracle (never a parity partner): the reference's AVX2 two-sibling slab path
# (include/simd_hit.h:121-156, include/bvh.h:109-116) with the optimisation level and contraction
# default of the reference's release build; x86-64-v3 (AVX2 + FMA) instead of -march=native because
# the library is built in the build container and timed on the GPU box's host CPU.
oracle-avx2: oracle/liboracle_avx2.so
oracle/liboracle_avx2.so: $(ORASRC) $(ORAHDR) Makefile
	$(CXX) -std=c++20 -O3 -march=x86-64-v3 -fPIC -shared -pthread -Wall -Iinclude -DORACLE_AVX2_TIMING=1 $(ORASRC) -o $@

clean:
	rm -rf $(LIBDIR)/*.so oracle/*.so build/hip

.PHONY: all host hip $(FRAMELIBS) oracle oracle-avx2 cli clean
