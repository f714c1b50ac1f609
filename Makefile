# Build of the MI355X approximate counter (gfx950).  `make` builds:
#   approx_counter_amd/lib/libapprox_counter_amd.so   C-ABI + HIP kernel (the hot path)
#   approx_counter_amd/lib/libac_host.so              host stages' C ABI (tests of the CLI's CPU stages)
#   approx_counter_amd/bin/adaptFinder                the drop-in CLI (host C++ + the C-ABI library)
#   oracle/_build/libac_oracle.so                     CPU oracle (tests only)
#
# A/B builds (tools/variants.sh, variant_dir.sh, variant_rev.sh) build the first of these only, from
# another source tree and / or with more flags, into a directory of their own:
#   make lib SRC=<tree holding include/ and approx_counter_amd/csrc/> OUT=<dir> EXTRA_FLAGS="-DFLAG=.."
# puts OUT/libapprox_counter_amd.so (objects in OUT/obj).
ROCM_PATH ?= /opt/rocm
HIPCC ?= $(ROCM_PATH)/bin/hipcc
ARCH ?= gfx950
EXTRA_FLAGS ?=
SRC ?= .
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -Wall $(EXTRA_FLAGS)
# wm_count: keep the queue-claim atomic a plain returning atomic (the optimizer's wave-aggregated
# form waits for the result at once, exposing the claim latency the kernel hides behind a window)
WM_FLAGS ?= -mllvm -amdgpu-atomic-optimizer-strategy=None
PKG := approx_counter_amd
INC := $(SRC)/include
CSRC := $(SRC)/$(PKG)/csrc
LIBDIR := $(PKG)/lib
ifdef OUT
LIB := $(OUT)/libapprox_counter_amd.so
OBJDIR := $(OUT)/obj
else
LIB := $(LIBDIR)/libapprox_counter_amd.so
OBJDIR := build/obj
endif

# the C-ABI layer: host code over the HIP runtime (hipcc as a C++ compiler: no kernel in these) ...
CAPI := capi count_launch capi_exact capi_comm capi_cooc capi_cross capi_span capi_flank capi_edit
# ... and plain host C++ (g++): the worker pool + AVX packer, the jobs stage's plan
HOSTONLY := host_pack stage_plan
HDRS := $(INC)/approx_counter_amd.h $(INC)/approx_counter_amd_testing.h $(CSRC)/wm_count.h $(CSRC)/exact_count.h \
	$(CSRC)/host_pack.h $(CSRC)/nrec.h $(CSRC)/ctx.h $(CSRC)/stage_plan.h $(CSRC)/bs_nfa.h $(CSRC)/bs_nfa_r.h \
	$(CSRC)/hit_levels.h $(CSRC)/bs_pos.h $(CSRC)/hit_cooc.h $(CSRC)/hit_cross.h $(CSRC)/hit_span.h \
	$(CSRC)/hit_flank.h $(CSRC)/hit_edit.h
INCS := -I$(INC) -I$(CSRC)
# host-only code that includes the HIP headers (no kernel, no <<<>>>)
HIP_HOST := -D__HIP_PLATFORM_AMD__ -I$(ROCM_PATH)/include

CXX ?= g++
HOST_CXXFLAGS ?= -O3 -std=c++17 -fPIC -Wall -Wextra $(EXTRA_FLAGS)
HOSTDIR := $(CSRC)/host
HOST_SRC := $(HOSTDIR)/host_stages.cpp
HOST_HDRS := $(HOSTDIR)/host_stages.h include/approx_counter_host.h include/approx_counter_amd.h
HOSTLIB := $(LIBDIR)/libac_host.so
BINDIR := $(PKG)/bin
CLI := $(BINDIR)/adaptFinder

all: $(LIB) $(HOSTLIB) $(CLI) oracle

lib: $(LIB)

# the count kernels' translation unit: wm_count.hip and the files it includes
WM_SRC := $(CSRC)/wm_count.hip $(CSRC)/wm_tid_blocks.inc $(CSRC)/stage_dev.inc $(CSRC)/count_frame.inc \
	$(CSRC)/wm_window_loop.inc $(CSRC)/bs_count.inc

$(OBJDIR)/wm_count.o: $(WM_SRC) $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(WM_FLAGS) $(INCS) -c $< -o $@

# the other families of the bit-sliced kernels (E = 3; hits; hits and positions; the staged forms of those
# two), with the reduction kernels that live beside them: the same frame and body through bs_family.inc,
# each a translation unit of its own (they compile beside wm_count.o)
BS_UNITS := bs3_count bsh_count bsp_count bshs_count bsps_count
BS_INCS := $(CSRC)/bs_family.inc $(CSRC)/stage_dev.inc $(CSRC)/count_frame.inc $(CSRC)/bs_count.inc

$(BS_UNITS:%=$(OBJDIR)/%.o): $(OBJDIR)/%.o: $(CSRC)/%.hip $(BS_INCS) $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(WM_FLAGS) $(INCS) -c $< -o $@

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(INCS) -c $< -o $@

# the jobs stage holds a kernel (the stage's copy kernel)
$(OBJDIR)/jobs_stage.o: $(CSRC)/jobs_stage.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -x hip $(INCS) -c $< -o $@

$(CAPI:%=$(OBJDIR)/%.o): $(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(filter-out --offload-arch=%,$(HIPFLAGS)) -x c++ $(HIP_HOST) $(INCS) -c $< -o $@

# (stage_plan.cpp reads the kernel's constants from wm_count.h, which includes the HIP headers)
$(HOSTONLY:%=$(OBJDIR)/%.o): $(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(CXX) $(HOST_CXXFLAGS) $(HIP_HOST) $(INCS) -c $< -o $@

$(LIB): $(OBJDIR)/wm_count.o $(BS_UNITS:%=$(OBJDIR)/%.o) $(OBJDIR)/hit_cooc.o $(OBJDIR)/hit_cross.o $(OBJDIR)/hit_span.o $(OBJDIR)/hit_flank.o $(OBJDIR)/hit_edit.o $(OBJDIR)/exact_count.o $(OBJDIR)/jobs_stage.o $(CAPI:%=$(OBJDIR)/%.o) $(HOSTONLY:%=$(OBJDIR)/%.o)
	@mkdir -p $(dir $@)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -pthread

$(HOSTLIB): $(HOST_SRC) $(HOSTDIR)/host_capi.cpp $(HOST_HDRS)
	@mkdir -p $(LIBDIR)
	$(CXX) $(HOST_CXXFLAGS) -Iinclude -I$(HOSTDIR) -shared -o $@ $(HOST_SRC) $(HOSTDIR)/host_capi.cpp

$(CLI): $(HOSTDIR)/adaptfinder.cpp $(HOST_SRC) $(HOST_HDRS) $(CSRC)/hit_levels.h $(CSRC)/bs_nfa.h $(CSRC)/bs_nfa_r.h $(CSRC)/bs_pos.h $(CSRC)/hit_cooc.h $(CSRC)/hit_flank.h $(CSRC)/hit_edit.h $(LIB)
	@mkdir -p $(BINDIR)
	$(CXX) $(HOST_CXXFLAGS) -Iinclude -I$(HOSTDIR) -o $@ $(HOSTDIR)/adaptfinder.cpp $(HOST_SRC) \
		-L$(LIBDIR) -lapprox_counter_amd -Wl,-rpath,'$$ORIGIN/../lib' -pthread

oracle:
	$(MAKE) -s -C oracle

# the device assembly of every kernel unit, into build/asm
ASM_WM := wm_count $(BS_UNITS)
asm: $(ASM_WM:%=build/asm/%.s) build/asm/hit_cooc.s build/asm/hit_cross.s build/asm/hit_span.s build/asm/hit_flank.s build/asm/hit_edit.s

$(ASM_WM:%=build/asm/%.s): build/asm/%.s: $(CSRC)/%.hip $(WM_SRC) $(BS_INCS) $(HDRS)
	@mkdir -p build/asm
	$(HIPCC) $(HIPFLAGS) $(WM_FLAGS) $(INCS) --cuda-device-only -S $< -o $@

build/asm/%.s: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build/asm
	$(HIPCC) $(HIPFLAGS) $(INCS) --cuda-device-only -S $< -o $@

# the stand-alone host check of hit_edit.h (tests/test_edits_cpu.py builds its own, with the sanitizers on)
build/hit_edit_check: tools/hit_edit_check.cpp $(CSRC)/hit_edit.h $(CSRC)/hit_flank.h $(CSRC)/hit_span.h $(CSRC)/bs_pos.h
	@mkdir -p build
	$(CXX) $(HOST_CXXFLAGS) -I$(CSRC) -o $@ $<

clean:
	rm -rf build $(LIBDIR) $(BINDIR) oracle/_build

.PHONY: all lib oracle asm clean
