# Builds the product library, the CLI and the test-only helpers. gfx950 only.
HIPCC ?= hipcc
ARCH ?= gfx950
CSRC := demucs_cpp_amd/csrc
SHELL := /bin/bash
# No packed fp32 VALU arithmetic in device code. On gfx950 a v_pk_{add,mul,fma}_f32 whose LOW lane takes the HIGH half of
# src1 (op_sel:[0,1,..]) returns wrong results in lanes 48-63 while another wave of the CU executes 16-bit-input MFMAs
# (tools/micro/pk_f32_erratum.hip reproduces it in isolation; profiles/DESIGN_history_r5.md section 7.1). The compiler's SLP vectoriser produces
# such forms (complex butterflies of the FFT, paired epilogue math), and every kernel of this library can share a CU with the
# exact-split kernels' bf16 MFMAs. Scalar fp32 VALU code computes the same bits and is 1.5 % FASTER beside MFMAs (measured,
# profiles/r05_ab_packed_fp32.txt). tests/test_isa_rules.py asserts that the shipped code objects contain none.
# (the feature switch is seen by the host pass too, which prints one "not a recognized feature" line per file: filtered)
NOPK := -Xclang -target-feature -Xclang -packed-fp32-ops
QUIET := 2> >(grep -v "packed-fp32-ops' is not a recognized feature" >&2)
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-result $(NOPK)
LIB := demucs_cpp_amd/lib/libdemucs_hip.so
OBJS := $(addprefix build/,igemm.o igemm_split.o igemm_lin256.o dgemm.o dconv_row.o fft.o misc.o tracks.o attention.o attention_split.o resample.o pcm.o loudness.o meters.o limiter.o flac.o flac_in.o v3.o api.o exec.o tracks_exec.o codec_api.o debug_api.o engine.o plan.o model_pack.o tracks_plan.o gemm_select.o)

all: $(LIB) cli oracle interp op_step plan_harness chain_harness rates_harness att_harness flac_in_host flac_host loudness_host meters_host limiter_host harness micro

build/%.o: $(CSRC)/%.hip $(CSRC)/kernels.h $(CSRC)/pcm_gather.h $(CSRC)/loudness_plan.h $(CSRC)/meters_plan.h $(CSRC)/limiter_plan.h $(CSRC)/loud_chain.h $(CSRC)/tp_phases.h $(CSRC)/plan.h $(CSRC)/gemm_tiles.h $(CSRC)/gemm_select.h $(CSRC)/api_internal.h $(CSRC)/igemm_common.h $(CSRC)/attention_common.h $(CSRC)/attention_select.h
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@ $(QUIET)
# the limiter's products are separate roundings: contraction off for the whole file
build/limiter.o: HIPFLAGS += -ffp-contract=off
build/%.o: $(CSRC)/%.cpp $(CSRC)/kernels.h $(CSRC)/loudness_plan.h $(CSRC)/meters_plan.h $(CSRC)/limiter_plan.h $(CSRC)/loud_chain.h $(CSRC)/plan.h $(CSRC)/plan_describe.h $(CSRC)/attention_select.h $(CSRC)/gemm_tiles.h $(CSRC)/gemm_select.h $(CSRC)/api_internal.h $(CSRC)/tracks_plan.h include/demucs_hip.h
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@ $(QUIET)

$(LIB): $(OBJS)
	@mkdir -p demucs_cpp_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -ldl -lpthread

cli: cli/demucs.cpp.main cli/demucs_ft.cpp.main cli/demucs_mt.cpp.main cli/demucs_ft_mt.cpp.main cli/demucs_v3.cpp.main cli/demucs_v3_mt.cpp.main cli/demucs_batch.cpp.main
cli/%.cpp.main: cli/%_main.cpp $(LIB) demucs_cpp_amd/host/demucscpp_hip.hpp demucs_cpp_amd/host/threaded_inference_hip.hpp cli/wav.hpp
	g++ -O2 -std=c++17 -Iinclude -Idemucs_cpp_amd/host -o $@ $< -Ldemucs_cpp_amd/lib -ldemucs_hip -lpthread -Wl,-rpath,'$$ORIGIN/../demucs_cpp_amd/lib'

oracle:
	$(MAKE) -C oracle
interp:
	@mkdir -p tests/_build
	g++ -O2 -march=native -fopenmp -std=c++17 -fPIC -shared -o tests/_build/libcpu_interp.so tests/cpu_interp.cpp
# the interpreter's step interface as a stand-alone program (tests/test_op_reference_cpu.py; CXXFLAGS_OP_STEP=-fsanitize=address,undefined
# OP_STEP_OUT=... builds the sanitizer form)
OP_STEP_OUT ?= tests/_build/op_step_main
op_step: $(OP_STEP_OUT)
$(OP_STEP_OUT): tests/op_step_main.cpp tests/cpu_interp.cpp $(CSRC)/plan.cpp $(CSRC)/plan.h $(CSRC)/plan_describe.h $(CSRC)/model_pack.cpp $(CSRC)/gemm_select.cpp $(CSRC)/gemm_select.h $(CSRC)/gemm_tiles.h
	@mkdir -p $(dir $@)
	g++ -O2 -g -std=c++17 -fopenmp $(CXXFLAGS_OP_STEP) -o $@ tests/op_step_main.cpp
# the multi-track plan (csrc/tracks_plan.cpp: host arithmetic, no HIP) as a stand-alone CPU program that prints it as JSON
plan_harness: tests/_build/tracks_plan_harness
tests/_build/tracks_plan_harness: tests/tracks_plan_harness.cpp $(CSRC)/tracks_plan.cpp $(CSRC)/tracks_plan.h include/demucs_hip.h
	@mkdir -p tests/_build
	g++ -O2 -std=c++17 -Wall -o $@ tests/tracks_plan_harness.cpp $(CSRC)/tracks_plan.cpp
# the workspace layout of the loudness / limiter output chain (csrc/loud_chain.h: host arithmetic, no HIP), printed as JSON
# (tests/test_loud_chain_layout_cpu.py; chain_harness_asan builds the sanitizer form, run as its own program)
CHAIN_OUT ?= tests/_build/loud_chain_harness
chain_harness: $(CHAIN_OUT)
$(CHAIN_OUT): tests/loud_chain_harness.cpp $(CSRC)/loud_chain.h $(CSRC)/loudness_plan.h $(CSRC)/meters_plan.h $(CSRC)/limiter_plan.h
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -Wall $(CXXFLAGS_CHAIN) -o $@ tests/loud_chain_harness.cpp
chain_harness_asan:
	$(MAKE) chain_harness CHAIN_OUT=tests/_build/loud_chain_harness_asan CXXFLAGS_CHAIN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
# the same plan for tracks at other sample rates (native-rate ranges), printed by a program of its own (tests/test_track_rates_cpu.py;
# CXXFLAGS_RATES=-fsanitize=address,undefined RATES_OUT=... builds the sanitizer form)
RATES_OUT ?= tests/_build/track_rates_harness
rates_harness: $(RATES_OUT)
$(RATES_OUT): tests/track_rates_harness.cpp $(CSRC)/tracks_plan.cpp $(CSRC)/tracks_plan.h include/demucs_hip.h
	@mkdir -p $(dir $@)
	g++ -O2 -g -std=c++17 -Wall $(CXXFLAGS_RATES) -o $@ tests/track_rates_harness.cpp $(CSRC)/tracks_plan.cpp
# the attention form rule (csrc/attention_select.h: host arithmetic, no HIP) over the plans a context builds, as a stand-alone CPU program
att_harness: tests/_build/attention_select_harness
tests/_build/attention_select_harness: tests/attention_select_harness.cpp $(CSRC)/attention_select.h $(CSRC)/plan.cpp $(CSRC)/plan.h $(CSRC)/model_pack.cpp $(CSRC)/gemm_select.cpp $(CSRC)/gemm_select.h $(CSRC)/gemm_tiles.h
	@mkdir -p tests/_build
	g++ -O2 -std=c++17 -Wall -o $@ tests/attention_select_harness.cpp

# the FLAC input stage's kernel text (csrc/flac_in.hip) as host code in a stand-alone CPU program (tests/test_flac_in_cpu.py;
# CXXFLAGS_FLAC_IN=-fsanitize=address,undefined FLAC_IN_OUT=... builds the sanitizer form, as flac_in_host_asan does)
FLAC_IN_OUT ?= tests/_build/flac_in_host_main
flac_in_host: $(FLAC_IN_OUT)
$(FLAC_IN_OUT): tests/flac_in_host_main.cpp $(CSRC)/flac_in.hip include/demucs_hip.h
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -Wall -DDMX_FLAC_IN_HOST $(CXXFLAGS_FLAC_IN) -o $@ tests/flac_in_host_main.cpp
# (the plain form comes with it: the tests that run either of them build through this target)
flac_in_host_asan: flac_in_host
	$(MAKE) flac_in_host FLAC_IN_OUT=tests/_build/flac_in_host_main_asan CXXFLAGS_FLAC_IN="-fsanitize=address,undefined -fno-sanitize-recover=undefined"

# the FLAC output stage's kernel text (csrc/flac.hip) as host code in a stand-alone CPU program (tests/test_flac_lpc_cpu.py;
# CXXFLAGS_FLAC=-fsanitize=address,undefined FLAC_OUT=... builds the sanitizer form, as flac_host_asan does). Contraction is
# off, as it is in the kernel's Levinson-Durbin and quantisation: every binary64 operation is rounded once
FLAC_OUT ?= tests/_build/flac_host_main
flac_host: $(FLAC_OUT)
$(FLAC_OUT): tests/flac_host_main.cpp $(CSRC)/flac.hip
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -ffp-contract=off -DDMX_FLAC_HOST $(CXXFLAGS_FLAC) -o $@ tests/flac_host_main.cpp
flac_host_asan:
	$(MAKE) flac_host FLAC_OUT=tests/_build/flac_host_main_asan CXXFLAGS_FLAC="-fsanitize=address,undefined -fno-sanitize-recover=undefined"

# the loudness stage's kernel text (csrc/loudness.hip) as host code in a stand-alone CPU program (tests/test_loudness_cpu.py): the
# chunked scan, the hop straddle and the fixed-order sums, lane by lane. Contraction is off: every binary64 operation is rounded once
LOUD_OUT ?= tests/_build/loudness_host_main
loudness_host: $(LOUD_OUT)
$(LOUD_OUT): tests/loudness_host_main.cpp $(CSRC)/loudness.hip $(CSRC)/loudness_plan.h
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -ffp-contract=off -DDMX_LOUDNESS_HOST $(CXXFLAGS_LOUD) -o $@ tests/loudness_host_main.cpp
loudness_host_asan:
	$(MAKE) loudness_host LOUD_OUT=tests/_build/loudness_host_main_asan CXXFLAGS_LOUD="-fsanitize=address,undefined -fno-sanitize-recover=undefined"

# the meters' kernel text (csrc/meters.hip) as host code in a stand-alone CPU program (tests/test_meters_cpu.py): the staged tiles
# and their halo, the lane's window, the integer histogram and its walk; the hop energies through loudness.hip compiled the same
# way. Contraction is off, as it is in the kernel: every product and every sum is rounded once
METERS_OUT ?= tests/_build/meters_host_main
meters_host: $(METERS_OUT)
$(METERS_OUT): tests/meters_host_main.cpp $(CSRC)/meters.hip $(CSRC)/meters_plan.h $(CSRC)/tp_phases.h $(CSRC)/loudness.hip $(CSRC)/loudness_plan.h
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -ffp-contract=off $(CXXFLAGS_METERS) -o $@ tests/meters_host_main.cpp
meters_host_asan:
	$(MAKE) meters_host METERS_OUT=tests/_build/meters_host_main_asan CXXFLAGS_METERS="-fsanitize=address,undefined -fno-sanitize-recover=undefined"

# the limiter's kernel text (csrc/limiter.hip) as host code in a stand-alone CPU program (tests/test_limiter_cpu.py): the level,
# the required reduction, the tiles' aggregates, the carry sweeps and the two scans, thread by thread; the true-peak phases
# through meters.hip compiled the same way. Contraction is off, as it is in the kernel
LIMITER_OUT ?= tests/_build/limiter_host_main
limiter_host: $(LIMITER_OUT)
$(LIMITER_OUT): tests/limiter_host_main.cpp $(CSRC)/limiter.hip $(CSRC)/limiter_plan.h $(CSRC)/meters.hip $(CSRC)/meters_plan.h $(CSRC)/tp_phases.h
	@mkdir -p $(dir $@)
	g++ -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -Wno-unused-function -ffp-contract=off $(CXXFLAGS_LIMITER) -o $@ tests/limiter_host_main.cpp
limiter_host_asan:
	$(MAKE) limiter_host LIMITER_OUT=tests/_build/limiter_host_main_asan CXXFLAGS_LIMITER="-fsanitize=address,undefined -fno-sanitize-recover=undefined"

# GPU test harnesses of the C++ shim (re-entrancy; Eigen-typed overloads against tests/eigen_stub, which is NOT Eigen)
harness: tests/_build/shim_harness tests/_build/shim_harness_eigen tests/_build/wav_harness tests/_build/pcm_wav_harness tests/_build/remix_parse_harness
tests/_build/remix_parse_harness: tests/remix_parse_harness.cpp $(LIB) demucs_cpp_amd/host/demucscpp_hip.hpp
	@mkdir -p tests/_build
	g++ -O2 -std=c++17 -Iinclude -Idemucs_cpp_amd/host -o $@ $< -Ldemucs_cpp_amd/lib -ldemucs_hip -lpthread -Wl,-rpath,'$$ORIGIN/../../demucs_cpp_amd/lib'
tests/_build/pcm_wav_harness: tests/pcm_wav_harness.cpp cli/wav.hpp $(LIB) demucs_cpp_amd/host/demucscpp_hip.hpp
	@mkdir -p tests/_build
	g++ -O2 -std=c++17 -Iinclude -Idemucs_cpp_amd/host -Icli -o $@ $< -Ldemucs_cpp_amd/lib -ldemucs_hip -lpthread -Wl,-rpath,'$$ORIGIN/../../demucs_cpp_amd/lib'
tests/_build/wav_harness: tests/wav_harness.cpp cli/wav.hpp $(LIB) demucs_cpp_amd/host/demucscpp_hip.hpp
	@mkdir -p tests/_build
	g++ -O2 -std=c++17 -Iinclude -Idemucs_cpp_amd/host -Icli -o $@ $< -Ldemucs_cpp_amd/lib -ldemucs_hip -lpthread -Wl,-rpath,'$$ORIGIN/../../demucs_cpp_amd/lib'
tests/_build/shim_harness: tests/shim_harness.cpp $(LIB) demucs_cpp_amd/host/demucscpp_hip.hpp
	@mkdir -p tests/_build
	g++ -O2 -std=c++17 -Iinclude -Idemucs_cpp_amd/host -o $@ $< -Ldemucs_cpp_amd/lib -ldemucs_hip -lpthread -Wl,-rpath,'$$ORIGIN/../../demucs_cpp_amd/lib'
tests/_build/shim_harness_eigen: tests/shim_harness.cpp $(LIB) demucs_cpp_amd/host/demucscpp_hip.hpp
	@mkdir -p tests/_build
	g++ -O2 -std=c++17 -DDEMUCSCPP_HIP_WITH_EIGEN -Itests/eigen_stub -Iinclude -Idemucs_cpp_amd/host -o $@ $< -Ldemucs_cpp_amd/lib -ldemucs_hip -lpthread -Wl,-rpath,'$$ORIGIN/../../demucs_cpp_amd/lib'

# hardware-semantics checks the kernels rely on (run by the GPU tests)
micro: tests/_build/lds_dma tests/_build/fft_mfma_repro tests/_build/fft_mfma_repro_pk tests/_build/pk_f32_erratum
# the packed-fp32 erratum (NOPK above): the product's stft_kernel beside a bare MFMA loop, built like the product (immune) and
# with packed fp32 arithmetic switched back on (what round 4 shipped: wrong frames); the single-instruction reproducer
tests/_build/fft_mfma_repro: tools/micro/fft_mfma_repro.hip $(CSRC)/fft.hip $(CSRC)/kernels.h
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -I$(CSRC) $(NOPK) -Wno-unused-result -o $@ $< $(QUIET)
tests/_build/fft_mfma_repro_pk: tools/micro/fft_mfma_repro.hip $(CSRC)/fft.hip $(CSRC)/kernels.h
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -I$(CSRC) -Wno-unused-result -o $@ $<
tests/_build/pk_f32_erratum: tools/micro/pk_f32_erratum.hip
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fno-slp-vectorize -Wno-unused-result -o $@ $<
tests/_build/lds_dma: tools/micro/lds_dma.hip
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result -o $@ $<

clean:
	rm -rf build $(LIB) tests/_build cli/*.main
	$(MAKE) -C oracle clean
.PHONY: all cli oracle interp op_step plan_harness chain_harness chain_harness_asan rates_harness att_harness flac_in_host flac_in_host_asan flac_host flac_host_asan loudness_host loudness_host_asan meters_host meters_host_asan limiter_host limiter_host_asan harness micro clean

# experiment builds: make variant NAME=timing FLAGS="-DDMX_TIMING -DDMX_PIN_LOADS=1"
variant:
	@mkdir -p build/$(NAME)
	for f in igemm igemm_split igemm_lin256 dgemm dconv_row fft misc tracks attention attention_split resample pcm loudness meters limiter flac flac_in v3; do $(HIPCC) $(HIPFLAGS) $(FLAGS) $$([ $$f = limiter ] && echo -ffp-contract=off) -c $(CSRC)/$$f.hip -o build/$(NAME)/$$f.o & done; \
	for f in api exec tracks_exec codec_api debug_api engine plan model_pack tracks_plan gemm_select; do $(HIPCC) $(HIPFLAGS) $(FLAGS) -x hip -c $(CSRC)/$$f.cpp -o build/$(NAME)/$$f.o & done; wait
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o demucs_cpp_amd/lib/libdemucs_hip_$(NAME).so build/$(NAME)/*.o
# one file rebuilt with other flags, the rest of the product's objects unchanged:
#   make variant1 NAME=fftnoslp FILE=fft FLAGS=-fno-slp-vectorize   ->  demucs_cpp_amd/lib/libdemucs_hip_fftnoslp.so
variant1: $(LIB)
	@mkdir -p build/$(NAME)
	$(HIPCC) $(HIPFLAGS) $(if $(filter limiter,$(FILE)),-ffp-contract=off) $(FLAGS) -c $(CSRC)/$(FILE).hip -o build/$(NAME)/$(FILE).o $(QUIET)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o demucs_cpp_amd/lib/libdemucs_hip_$(NAME).so $(filter-out build/$(FILE).o,$(OBJS)) build/$(NAME)/$(FILE).o -ldl -lpthread
# the same with the one file taken from another path (generated, instrumented copies: tools/micro/dconv_row_timing.py)
variant1src: $(LIB)
	@mkdir -p build/$(NAME)
	$(HIPCC) $(HIPFLAGS) $(FLAGS) -I$(CSRC) -c $(SRC) -o build/$(NAME)/$(FILE).o $(QUIET)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o demucs_cpp_amd/lib/libdemucs_hip_$(NAME).so $(filter-out build/$(FILE).o,$(OBJS)) build/$(NAME)/$(FILE).o -ldl -lpthread
# two files taken from other paths (tools/micro/lin_variants.py: a kernel variant together with the plan choice that exercises it)
variant2src: $(LIB)
	@mkdir -p build/$(NAME)
	$(HIPCC) $(HIPFLAGS) $(FLAGS) -I$(CSRC) -c $(SRC) -o build/$(NAME)/$(FILE).o $(QUIET)
	$(HIPCC) $(HIPFLAGS) $(FLAGS) -I$(CSRC) -Iinclude -x hip -c $(SRC2) -o build/$(NAME)/$(FILE2).o $(QUIET)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o demucs_cpp_amd/lib/libdemucs_hip_$(NAME).so $(filter-out build/$(FILE).o build/$(FILE2).o,$(OBJS)) build/$(NAME)/$(FILE).o build/$(NAME)/$(FILE2).o -ldl -lpthread
