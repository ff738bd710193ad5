# Builds the in-tree shared libraries:
#   clraytracer_amd/csrc/libcrt_hip.so   HIP kernels + C-ABI (include/crt_api.h), gfx950 only
#   clraytracer_amd/denoise/libcrt_denoise.so   the a-trous denoiser on device buffers (include/crt_denoise.h), gfx950 only, stateless
#   clraytracer_amd/temporal/libcrt_temporal.so   temporal reprojection and accumulation on device buffers (include/crt_temporal.h), gfx950 only, stateless
#   clraytracer_amd/vfilter/libcrt_vfilter.so   the variance-guided a-trous filter on device buffers (include/crt_vfilter.h), gfx950 only, stateless
#   clraytracer_amd/motion/libcrt_motion.so   temporal accumulation that follows moving instances (include/crt_motion.h), gfx950 only, stateless
#   clraytracer_amd/upsample/libcrt_upsample.so   guided upsampling of a low-resolution pass on device buffers (include/crt_upsample.h), gfx950 only, stateless
#   clraytracer_amd/select/libcrt_select.so   selective re-tracing on device buffers: compact, gather, scatter (include/crt_select.h), gfx950 only, stateless
#   clraytracer_amd/present/libcrt_present.so   the chain's last step on device buffers: compose, tone-map, FXAA, RGBA8, and the G-buffer's ID views (include/crt_present.h), gfx950 only, stateless
#   clraytracer_amd/meter/libcrt_meter.so   metering and auto-exposure on device buffers: a log-luminance histogram resolved to an exposure in device memory, and the multiply by it (include/crt_meter.h), gfx950 only, stateless
#   clraytracer_amd/host/libcrt_host.so  C++ host mirror of Renderer/ResourceManager/AssetManager (+ include/crt_host.h)
#   oracle/libcrt_oracle.so              CPU oracle (test infrastructure only)
# The eight stateless image libraries are one .hip unit each over the headers of clraytracer_amd/image/ (the steps they share; no library of its own);
# libcrt_present.so also compiles clraytracer_amd/csrc/crt_post.h, the frame's per-pixel stages, which libcrt_hip.so compiles from the same text.
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
ARCH ?= gfx950
# -fno-slp-vectorize: the SLP vectoriser turns the slab tests into v_pk_* with splat operands that cost the trace kernel 20+ VGPRs
# (96 -> 73) and spilled the 6-waves/SIMD flavour to scratch (290 MB per frame); without it the kernel fits 7 waves/SIMD.
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall -Wno-unused-function
CXXFLAGS = -O2 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC -Wall -Wextra -pthread

HIP_SO = clraytracer_amd/csrc/libcrt_hip.so
# The translation units of libcrt_hip.so in link order, crt_shim.hip (the C-ABI and every frame kernel) first; each unit's first lines say what it holds.
# The list is written here only: tools/kernel_resources.py reads it and HIPFLAGS from this file, tools/ab_build.sh and tools/ab_define.sh build their
# variants through the $(HIP_SO) rule (HIP_SO=<their output> EXTRA_HIPFLAGS="<the variant's flags>"), tests/test_kernel_resources.py checks the rest.
HIP_UNITS = crt_shim.hip crt_rays.hip crt_ao.hip crt_inclusive.hip crt_recip.hip crt_shade.hip
HIP_SRC = $(addprefix clraytracer_amd/csrc/,$(HIP_UNITS))
EXTRA_HIPFLAGS ?=
HOST_SO = clraytracer_amd/host/libcrt_host.so
HOST_SRC = $(addprefix clraytracer_amd/host/,AssetManager.cpp MeshCache.cpp JpegDecode.cpp BVH.cpp CPURayTrace.cpp Renderer.cpp ResourceManager.cpp crt_host_c.cpp ShmBarrier.cpp)
HOST_HDR = $(wildcard clraytracer_amd/host/*.hpp) $(wildcard include/*.h)

# a library of its own: a pure function of device buffers, and its kernels are no rows of libcrt_hip.so's resource ledger
DENOISE_SO = clraytracer_amd/denoise/libcrt_denoise.so
# likewise: the accumulation stage in front of the filter
TEMPORAL_SO = clraytracer_amd/temporal/libcrt_temporal.so
# likewise: the filter that reads the accumulation stage's moments plane
VFILTER_SO = clraytracer_amd/vfilter/libcrt_vfilter.so
# likewise: the accumulation stage again, reprojecting through each instance's own motion
MOTION_SO = clraytracer_amd/motion/libcrt_motion.so
# likewise: a low-resolution pass brought to the frame's resolution, guided by the frame's planes
UPSAMPLE_SO = clraytracer_amd/upsample/libcrt_upsample.so
# likewise: what lies between the image libraries and the point queries -- an ordered index list of selected pixels, their points, the way back
SELECT_SO = clraytracer_amd/select/libcrt_select.so
# likewise: the end of the chain -- the stages that follow Trace in a frame, on any image of the caller's, and the views of the guides
PRESENT_SO = clraytracer_amd/present/libcrt_present.so
# likewise: what the end of the chain is exposed by -- an image metered on the device, the exposure left in device memory
METER_SO = clraytracer_amd/meter/libcrt_meter.so

# the headers they share, compiled into each: device and host steps; the environment switches (not motion's); the accumulate kernel of
# temporal and motion
IMAGE_HDR = clraytracer_amd/image/crt_image_device.h clraytracer_amd/image/crt_image_host.h
IMAGE_ENV_HDR = clraytracer_amd/image/crt_image_env.h
ACCUMULATE_HDR = clraytracer_amd/image/crt_accumulate.h include/crt_temporal.h include/crt_motion.h
# the per-pixel stages behind Trace (PostProcess, the RGBA8 target, FXAA), written once for libcrt_hip.so (whose rule takes every header of csrc/) and libcrt_present.so
POST_HDR = clraytracer_amd/csrc/crt_post.h clraytracer_amd/csrc/crt_vec3.h

EXAMPLE = examples/crt_headless

UBENCH = tools/ubench/gather tools/ubench/chain tools/ubench/cumask tools/ubench/sky_index

all: $(HIP_SO) $(HOST_SO) $(DENOISE_SO) $(TEMPORAL_SO) $(VFILTER_SO) $(MOTION_SO) $(UPSAMPLE_SO) $(SELECT_SO) $(PRESENT_SO) $(METER_SO) $(EXAMPLE) $(UBENCH) oracle

# vector-L1 gather microbenchmark (profiles/r01_ubench_gather.txt)
tools/ubench/gather: tools/ubench/gather.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<
# dependent-chain 64-B gather microbenchmark: the ceiling bench.py's roofline.chain is taken against (profiles/r03_ubench_chain.*)
tools/ubench/chain: tools/ubench/chain.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -ffp-contract=off -fno-slp-vectorize -Wno-unused-value -Wno-uninitialized -Wno-sometimes-uninitialized -o $@ $<

# CU-mask probe: hipExtStreamCreateWithCUMask on this part, and which CU each mask bit names (round 4's reserved-CU experiment)
tools/ubench/cumask: tools/ubench/cumask.hip
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-value -o $@ $<

# device self-check of the guarded float skybox index (crt_device.h: sample_skybox_guarded) over the library's own header, with the library's flags:
# a program of its own, so that its two kernels are no rows of the library's resource ledger (tests/test_gpu_sky_index.py runs it)
tools/ubench/sky_index: tools/ubench/sky_index.hip clraytracer_amd/csrc/crt_device.h include/crt_api.h include/crt_types.h
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -Wno-unused-value -o $@ $<

# the reference's EngineMain loop over the mirrored C++ API
$(EXAMPLE): examples/headless_main.cpp $(HOST_SO)
	$(CXX) $(CXXFLAGS) -o $@ examples/headless_main.cpp -Lclraytracer_amd/host -lcrt_host -Lclraytracer_amd/csrc -lcrt_hip -Wl,-rpath,'$$ORIGIN/../clraytracer_amd/host' -Wl,-rpath,'$$ORIGIN/../clraytracer_amd/csrc'

# every unit of HIP_UNITS in one compiler call (crt_ao.hip's direction table crt_ao_table.h is written by tools/make_ao_table.py and committed)
$(HIP_SO): $(wildcard clraytracer_amd/csrc/*.h) $(HIP_SRC) include/crt_api.h include/crt_debug.h include/crt_types.h
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $(HIP_SRC)

$(DENOISE_SO): clraytracer_amd/denoise/crt_denoise.hip include/crt_denoise.h $(IMAGE_HDR) $(IMAGE_ENV_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(TEMPORAL_SO): clraytracer_amd/temporal/crt_temporal.hip $(ACCUMULATE_HDR) $(IMAGE_HDR) $(IMAGE_ENV_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(VFILTER_SO): clraytracer_amd/vfilter/crt_vfilter.hip include/crt_vfilter.h $(IMAGE_HDR) $(IMAGE_ENV_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(MOTION_SO): clraytracer_amd/motion/crt_motion.hip $(ACCUMULATE_HDR) $(IMAGE_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(UPSAMPLE_SO): clraytracer_amd/upsample/crt_upsample.hip include/crt_upsample.h $(IMAGE_HDR) $(IMAGE_ENV_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(SELECT_SO): clraytracer_amd/select/crt_select.hip include/crt_select.h include/crt_temporal.h $(IMAGE_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(PRESENT_SO): clraytracer_amd/present/crt_present.hip include/crt_present.h $(POST_HDR) $(IMAGE_HDR) $(IMAGE_ENV_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(METER_SO): clraytracer_amd/meter/crt_meter.hip include/crt_meter.h $(IMAGE_HDR) $(IMAGE_ENV_HDR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA_HIPFLAGS) -shared -o $@ $<

$(HOST_SO): $(HOST_SRC) $(HOST_HDR) $(HIP_SO)
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRC) -Lclraytracer_amd/csrc -lcrt_hip -lrt -Wl,-rpath,'$$ORIGIN/../csrc'

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(HIP_SO) $(HOST_SO) $(DENOISE_SO) $(TEMPORAL_SO) $(VFILTER_SO) $(MOTION_SO) $(UPSAMPLE_SO) $(SELECT_SO) $(PRESENT_SO) $(METER_SO) $(EXAMPLE) $(UBENCH)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
