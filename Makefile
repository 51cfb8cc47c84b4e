# Builds the product library octreeraytracer_amd/lib/libort.so (host scene stage + gfx950
# kernel + C ABI) and the test-only oracle (oracle/liboracle.so, oracle/_ref/ref_octree).
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
ARCH ?= gfx950
SRC := octreeraytracer_amd/csrc
OBJ := build/obj
LIB := octreeraytracer_amd/lib/libort.so
CXXFLAGS := -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC -Wall -Wextra -Wno-unused-parameter
HIPFLAGS := -O3 -std=c++17 --offload-arch=$(ARCH) -ffp-contract=off -fno-fast-math -fno-slp-vectorize -fPIC -Wall -Wno-unused-parameter

HOST_SRCS := octree.cpp scene.cpp host_abi.cpp layout.cpp raytracer.cpp
HOST_OBJS := $(addprefix $(OBJ)/,$(HOST_SRCS:.cpp=.o))
HIP_OBJS := $(OBJ)/ort_kernel.o $(OBJ)/gpu_build.o $(OBJ)/group.o
HDRS := $(wildcard $(SRC)/*.h) $(SRC)/prebuilt_scene.inc $(SRC)/ray_query.inc $(SRC)/accum.inc $(SRC)/camera_query.inc $(SRC)/ray_modes.inc $(SRC)/radiance_query.inc $(SRC)/denoise.inc $(SRC)/host_emulation.inc include/ort.h include/ort_math.h

# The analysis library (test/analysis surface: ort_debug_* host emulation and walk statistics,
# ORT_OPT_DEBUG_FLAGS) -- the same sources with -DORT_ANALYSIS=1; the CPU suite and tools/
# load it, the product library does not carry it.
ALIB := octreeraytracer_amd/lib/libort_analysis.so
AOBJ := build/obj_analysis

.PHONY: all lib analysis oracle ref examples san clean
all: lib analysis oracle examples

lib: $(LIB)

analysis: $(ALIB)

$(AOBJ)/%.o: $(SRC)/%.hip $(HDRS)
	@mkdir -p $(AOBJ)
	$(HIPCC) $(HIPFLAGS) -DORT_ANALYSIS=1 -c $< -o $@

$(ALIB): $(HOST_OBJS) $(AOBJ)/ort_kernel.o $(OBJ)/gpu_build.o $(AOBJ)/group.o
	@mkdir -p $(dir $(ALIB))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl -Wl,-soname,libort_analysis.so -Wl,-Bsymbolic

$(OBJ)/%.o: $(SRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJ)
	$(CXX) $(CXXFLAGS) -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -c $< -o $@

$(OBJ)/ort_kernel.o: $(SRC)/ort_kernel.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/gpu_build.o: $(SRC)/gpu_build.hip $(HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -Wno-unused-result -c $< -o $@

$(OBJ)/group.o: $(SRC)/group.hip $(SRC)/group_map.h $(SRC)/ort_internal.h include/ort.h
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(HOST_OBJS) $(HIP_OBJS)
	@mkdir -p $(dir $(LIB))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -ldl -Wl,-soname,libort.so

examples: build/ort_main build/stats_row build/trace_rays build/progressive build/pick build/visibility build/radiance_probe build/denoise

build/denoise: tests/cpp/denoise.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ tests/cpp/denoise.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/radiance_probe: tests/cpp/radiance_probe.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ tests/cpp/radiance_probe.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/visibility: tests/cpp/visibility.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ tests/cpp/visibility.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/pick: tests/cpp/pick.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ tests/cpp/pick.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/progressive: tests/cpp/progressive.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ tests/cpp/progressive.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/trace_rays: tests/cpp/trace_rays.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ tests/cpp/trace_rays.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/stats_row: tests/cpp/stats_row.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ tests/cpp/stats_row.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

build/ort_main: examples/main.cpp $(LIB) $(HDRS)
	$(CXX) -O2 -std=c++17 -I$(SRC) -o $@ examples/main.cpp -L$(dir $(LIB)) -lort -Wl,-rpath,'$$ORIGIN/../$(dir $(LIB))'

oracle:
	$(MAKE) -C oracle all

# Host AddressSanitizer + UndefinedBehaviorSanitizer build (CPU only; GPU sanitizers are not
# available): every host object -- scene stage, octree builder, layout compilers, host ABI,
# the kernel's per-pixel code compiled for the host, the group row map, the oracle -- built
# with clang and instrumented, linked into build/san/san_check (tests/cpp/san_check.cpp),
# which renders small frames through the emulation and the oracle and compares bits.
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1
SANOBJ := build/san
CLANGXX := /opt/rocm/bin/amdclang++
CLANG := /opt/rocm/bin/amdclang
SAN_HOST := $(addprefix $(SANOBJ)/,$(HOST_SRCS:.cpp=.o))
SAN_HIP := $(SANOBJ)/ort_kernel.o $(SANOBJ)/gpu_build.o $(SANOBJ)/group.o
HIP_SAN := $(foreach f,address undefined,-Xarch_host -fsanitize=$(f)) -Xarch_host -fno-sanitize-recover=undefined

san: build/san/san_check build/san/san_query build/san/san_camera build/san/san_query_modes build/san/san_radiance build/san/san_denoise
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 ./build/san/san_check
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 ./build/san/san_query
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 ./build/san/san_camera
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 ./build/san/san_query_modes
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 ./build/san/san_radiance
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 ./build/san/san_denoise

$(SANOBJ)/%.o: $(SRC)/%.cpp $(HDRS)
	@mkdir -p $(SANOBJ)
	$(CLANGXX) $(SAN) -std=c++17 -ffp-contract=off -fno-fast-math -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -c $< -o $@

$(SANOBJ)/%.o: $(SRC)/%.hip $(HDRS) $(SRC)/gpu_build.h $(SRC)/group_map.h
	@mkdir -p $(SANOBJ)
	$(HIPCC) -O1 -g -std=c++17 --offload-arch=$(ARCH) -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-result -DORT_ANALYSIS=1 $(HIP_SAN) -c $< -o $@

$(SANOBJ)/ort_oracle.o: oracle/ort_oracle.c oracle/ort_oracle.h include/ort_math.h
	@mkdir -p $(SANOBJ)
	$(CLANG) $(SAN) -std=c11 -ffp-contract=off -fno-fast-math -c $< -o $@

$(SANOBJ)/san_check.o: tests/cpp/san_check.cpp $(HDRS) oracle/ort_oracle.h
	@mkdir -p $(SANOBJ)
	$(CLANGXX) $(SAN) -std=c++17 -I$(SRC) -Ioracle -c $< -o $@

# the ray queries' host code (ort_debug_query_rays: render_core.h query_ray) under the same sanitizers
$(SANOBJ)/san_query.o: tests/cpp/san_query.cpp $(HDRS)
	@mkdir -p $(SANOBJ)
	$(CLANGXX) $(SAN) -std=c++17 -I$(SRC) -c $< -o $@

# the camera queries' host code (ort_debug_camera_query: camera_query.inc camera_query_ray) likewise
$(SANOBJ)/san_camera.o: tests/cpp/san_camera.cpp $(HDRS)
	@mkdir -p $(SANOBJ)
	$(CLANGXX) $(SAN) -std=c++17 -I$(SRC) -c $< -o $@

# the query modes' host code (ort_debug_query_rays_ex: render_core.h query_ray_mode) likewise
$(SANOBJ)/san_query_modes.o: tests/cpp/san_query_modes.cpp $(HDRS)
	@mkdir -p $(SANOBJ)
	$(CLANGXX) $(SAN) -std=c++17 -I$(SRC) -c $< -o $@

# the radiance queries' host code (ort_debug_radiance_rays: radiance_query.inc radiance_chain) likewise
$(SANOBJ)/san_radiance.o: tests/cpp/san_radiance.cpp $(HDRS)
	@mkdir -p $(SANOBJ)
	$(CLANGXX) $(SAN) -std=c++17 -I$(SRC) -c $< -o $@

# the denoiser's host code (ort_debug_denoise: denoise.inc denoise_pixel) likewise
$(SANOBJ)/san_denoise.o: tests/cpp/san_denoise.cpp $(HDRS)
	@mkdir -p $(SANOBJ)
	$(CLANGXX) $(SAN) -std=c++17 -I$(SRC) -c $< -o $@

build/san/san_denoise: $(SANOBJ)/san_denoise.o $(SAN_HOST) $(SAN_HIP)
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) -o $@ $^ -ldl

build/san/san_radiance: $(SANOBJ)/san_radiance.o $(SAN_HOST) $(SAN_HIP)
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) -o $@ $^ -ldl

build/san/san_query_modes: $(SANOBJ)/san_query_modes.o $(SAN_HOST) $(SAN_HIP)
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) -o $@ $^ -ldl

build/san/san_camera: $(SANOBJ)/san_camera.o $(SAN_HOST) $(SAN_HIP)
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) -o $@ $^ -ldl

build/san/san_query: $(SANOBJ)/san_query.o $(SAN_HOST) $(SAN_HIP)
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) -o $@ $^ -ldl

build/san/san_check: $(SANOBJ)/san_check.o $(SAN_HOST) $(SAN_HIP) $(SANOBJ)/ort_oracle.o
	$(HIPCC) --offload-arch=$(ARCH) $(SAN) -o $@ $^ -ldl

ref:
	$(MAKE) -C oracle ref

clean:
	rm -rf build $(LIB) $(ALIB)
	$(MAKE) -C oracle clean
