# Build of the MI355X loop-detection core (gfx950 only) and of the CPU oracle (test infrastructure).
#   make            -> cerebro_amd/lib/libcerebro_hip.so  + oracle/_build/liboracle.so  (+ oracle/_ref/libgms_ref.so, see `ref`)
#   make lib / make oracle / make ref / make ref_modes / make clean
ROCM       ?= /opt/rocm
HIPCC      ?= $(ROCM)/bin/hipcc
ARCH       ?= gfx950
# -ffp-contract=off: the PnP kernels must round exactly like the oracle (no FMA contraction);
# the scan kernel uses explicit fma() where the product is exact.
HIPFLAGS   ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -Wall -Wno-unused-function $(EXTRA_HIPFLAGS)
CC         ?= gcc
# -mfma only makes __builtin_fmaf a single vfmadd (exact either way); -ffp-contract=off forbids any other fusion
ORCFLAGS   ?= -O2 -mfma -ffp-contract=off -fopenmp -fPIC -Wall -Wextra

LIBDIR     := cerebro_amd/lib
CSRC       := cerebro_amd/csrc
HIP_SRCS   := $(CSRC)/kernels.hip $(CSRC)/chip_api.hip $(CSRC)/resident.hip $(CSRC)/chip_multi.hip $(CSRC)/pnp.hip $(CSRC)/icp.hip $(CSRC)/batch.hip $(CSRC)/match.hip $(CSRC)/frames.hip $(CSRC)/orb.hip $(CSRC)/project.hip $(CSRC)/vlad.hip $(CSRC)/pass_merge.hip
HIP_OBJS   := $(HIP_SRCS:$(CSRC)/%.hip=$(LIBDIR)/%.o)
ORC_SRCS   := $(wildcard oracle/*.c)

all: lib oracle host testlibs verify ref ref_modes
lib: $(LIBDIR)/libcerebro_hip.so
oracle: oracle/_build/liboracle.so oracle/_build/liboracle_eispack.so oracle/_build/liboracle_stats.so oracle/_build/liboracle_flops.so
host: $(LIBDIR)/libcerebro_host.so $(LIBDIR)/cerebro_replay $(LIBDIR)/minimal_loop_detector $(LIBDIR)/sync_tick_latency $(LIBDIR)/verify_candidate $(LIBDIR)/verify_candidates $(LIBDIR)/verify_candidates_stored $(LIBDIR)/verify_candidates_composed $(LIBDIR)/verify_candidates_modes $(LIBDIR)/verify_pairs_stored $(LIBDIR)/frame_put_disparity $(LIBDIR)/frame_put_stereo $(LIBDIR)/orb_detect $(LIBDIR)/orb_frame_put $(LIBDIR)/frame_put_raw_stereo $(LIBDIR)/frame_put_batch $(LIBDIR)/append_projected $(LIBDIR)/append_vlad $(LIBDIR)/append_batch $(LIBDIR)/self_join $(LIBDIR)/bulk_ticks
# test infrastructure that needs hipcc: the shared-memory stand-in for librccl (N ranks on one device, tests/test_fakerccl_gpu.py)
testlibs: tests/fakerccl/_build/libfakerccl.so $(LIBDIR)/norows/libcerebro_hip.so $(LIBDIR)/hooks/libcerebro_hip.so
# The TEST build of the library (-DCHIP_TEST_HOOKS): the fault-injection hooks (CHIP_TEST_COMM_INIT, CHIP_TEST_FAIL_SHARD,
# CHIP_TEST_BATCH_OOM, CHIP_TEST_RESIDENT_SKIP_MASTER) and the knobs that change what a kernel computes (CHIP_PNP_BACKSUB,
# CHIP_PNP_DEBUG_STOP) exist ONLY here.  `make lib` -- the product -- compiles none of them in (chip_get_info().test_hooks == 0);
# tests/ load this one for the tests that inject faults (cerebro_amd.capi.use_hooks_library).  Never deploy it.
HOOK_SRCS  := chip_api resident chip_multi pnp
HOOK_OBJS  := $(HOOK_SRCS:%=$(LIBDIR)/hooks/%.o)
$(LIBDIR)/hooks/%.o: $(CSRC)/%.hip $(CSRC)/chip_internal.h $(CSRC)/frame_store.h $(CSRC)/ransac_common.h $(CSRC)/topk_merge.h $(wildcard $(CSRC)/*.inc) include/cerebro_hip.h
	@mkdir -p $(LIBDIR)/hooks
	$(HIPCC) $(HIPFLAGS) -DCHIP_TEST_HOOKS -c $< -o $@
$(LIBDIR)/hooks/libcerebro_hip.so: $(HOOK_OBJS) $(HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(HOOK_OBJS) $(filter-out $(HOOK_SRCS:%=$(LIBDIR)/%.o),$(HIP_OBJS)) -o $@ -lpthread -ldl
# the degraded build (-DCHIP_NO_ROWS_FORM: what scripts/verify_codeobj.sh falls back to), kept next to the real one so that the GPU
# suite proves BOTH builds (tests/test_norows_build_gpu.py): only kernels.hip differs, the other objects are shared
$(LIBDIR)/norows/libcerebro_hip.so: $(CSRC)/kernels.hip $(HIP_OBJS)
	@mkdir -p $(LIBDIR)/norows
	$(HIPCC) $(HIPFLAGS) -DCHIP_NO_ROWS_FORM -c $(CSRC)/kernels.hip -o $(LIBDIR)/norows/kernels.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(LIBDIR)/norows/kernels.o $(filter-out $(LIBDIR)/kernels.o,$(HIP_OBJS)) -o $@ -lpthread -ldl
tests/fakerccl/_build/libfakerccl.so: tests/fakerccl/fakerccl.cc
	@mkdir -p tests/fakerccl/_build
	$(HIPCC) -O2 -std=c++17 -fPIC -shared $< -o $@ -lrt -lpthread

$(LIBDIR)/%.o: $(CSRC)/%.hip $(CSRC)/chip_internal.h $(CSRC)/frame_store.h $(CSRC)/ransac_common.h $(CSRC)/topk_merge.h $(wildcard $(CSRC)/*.inc) include/cerebro_hip.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/libcerebro_hip.so: $(HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ -lpthread -ldl

# ---- ROS-free C++ host side (mirror of the Cerebro / StaticTheiaPoseCompute::PNP surface) + replay harness ----
HOSTDIR    := cerebro_amd/host
CXX        ?= g++
$(LIBDIR)/libcerebro_host.so: $(HOSTDIR)/cerebro_host.cc $(HOSTDIR)/state_json.cc $(HOSTDIR)/cerebro_host.h $(HOSTDIR)/state_json.h include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Wextra $(HOSTDIR)/cerebro_host.cc $(HOSTDIR)/state_json.cc -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

$(LIBDIR)/cerebro_replay: $(HOSTDIR)/cerebro_replay.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra $(HOSTDIR)/cerebro_replay.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

oracle/_build/liboracle.so: $(ORC_SRCS) oracle/cerebro_oracle.h
	@mkdir -p oracle/_build
	$(CC) $(ORCFLAGS) -shared $(ORC_SRCS) -o $@ -lm

# The same oracle with EISPACK's original overflow-guard DIVISION in the Francis QR step (what Eigen::EigenSolver runs) instead
# of the exact power-of-two scaling: test infrastructure for tests/test_oracle_pnp_departures.py only.
oracle/_build/liboracle_eispack.so: $(ORC_SRCS) oracle/cerebro_oracle.h
	@mkdir -p oracle/_build
	$(CC) $(ORCFLAGS) -DORC_EISPACK_DIVIDE -shared $(ORC_SRCS) -o $@ -lm

# The same oracle counting, per pivot column of the DLS elimination, the candidates that tie (test infrastructure for
# tests/test_fuzz_scenes_reach_tie_paths.py only: which inputs reach the tie paths of the GPU's pivot search).
oracle/_build/liboracle_stats.so: $(ORC_SRCS) oracle/cerebro_oracle.h
	@mkdir -p oracle/_build
	$(CC) $(ORCFLAGS) -DORC_LU_TIE_STATS -shared $(ORC_SRCS) -o $@ -lm

# The same oracle counting the fp64 operations the PnP solver executes, per stage (test infrastructure: tests/test_oracle_flops.py pins
# the count, bench.py prices the PnP kernels' fp64-vector roofline from it -- VERDICT r4 next 1a).
oracle/_build/liboracle_flops.so: $(ORC_SRCS) oracle/cerebro_oracle.h
	@mkdir -p oracle/_build
	$(CC) $(ORCFLAGS) -DORC_FLOP_COUNT -shared $(ORC_SRCS) -o $@ -lm

# ---- plain-C-ABI example (the INTEGRATION.md call sequence without ROS / Eigen) ----
$(LIBDIR)/minimal_loop_detector: examples/minimal_loop_detector.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- build-time check of what the inline asm of the scan kernels relies on: the physical-VGPR partition of
# db_scan_topk_rows (amdgpu_num_vgpr(40) -> 80 ArchVGPRs on this hipcc; v[80:127] written by the asm loads only), no touch of an
# in-flight load register in the one-row kernel, pnp_build_solve <= 128 VGPRs.  scripts/verify_codeobj.sh DEGRADES instead of
# failing: a toolchain that allocates differently gets a library rebuilt with -DCHIP_NO_ROWS_FORM (loud line; chip_get_info says
# so); a machine without pytest / llvm-objdump gets a loud warning and the library as built.  `make lib` never runs it.
verify: $(LIBDIR)/.codeobj_verified
$(LIBDIR)/.codeobj_verified: $(LIBDIR)/libcerebro_hip.so tests/test_codeobj_registers.py scripts/verify_codeobj.sh $(LIBDIR)/libcerebro_host.so $(LIBDIR)/cerebro_replay $(LIBDIR)/minimal_loop_detector
	@ROCM="$(ROCM)" MAKE="$(MAKE)" bash scripts/verify_codeobj.sh; rc=$$?; \
	if [ $$rc -eq 0 ]; then touch $@; elif [ $$rc -eq 3 ]; then echo "make verify: NOT verified (no stamp written)"; else exit $$rc; fi

$(LIBDIR)/sync_tick_latency: examples/sync_tick_latency.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- one candidate through matching, GMS, the correspondence sets and the three poses: C++ against the two .so
$(LIBDIR)/verify_candidate: examples/verify_candidate.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/verify_candidate.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- B candidates of one keyframe in one call: verify_candidates against B x verify_candidate, field for field
$(LIBDIR)/verify_candidates: examples/verify_candidates.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/verify_candidates.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- the same B candidates on frames kept on the device: verify_candidates_stored against verify_candidates, field for field
$(LIBDIR)/verify_candidates_stored: examples/verify_candidates_stored.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/verify_candidates_stored.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- verify_candidates_stored against the same answer composed from single C calls (ICP per survivor), bit for bit
$(LIBDIR)/verify_candidates_composed: examples/verify_candidates_composed.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/verify_candidates_composed.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- the stored path with GMS scale / rotation (gms_modes = 3) against the same call with 0, on candidates that include a rolled one
$(LIBDIR)/verify_candidates_modes: examples/verify_candidates_modes.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/verify_candidates_modes.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- a backlog of (query, candidate) pairs on stored frames in one call: verify_pairs_stored against the loop of verify_candidates_stored with B = 1
$(LIBDIR)/verify_pairs_stored: examples/verify_pairs_stored.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/verify_pairs_stored.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- the same backlog with every frame put from its disparity map and, next to it, from the 3-D image a host loop makes of it: same bits.
# -ffp-contract=off: the example's host loop restates the reference's, which is built without FMA
$(LIBDIR)/frame_put_disparity: examples/frame_put_disparity.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -ffp-contract=off -Wall -Wextra examples/frame_put_disparity.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- the same backlog with every frame put from its rectified stereo pair and, next to it, from the int16 map a host restatement of the
# block matcher makes of that pair: same bits.  -ffp-contract=off for the host loop of the timed 3-D image, as above
$(LIBDIR)/frame_put_stereo: examples/frame_put_stereo.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -ffp-contract=off -Wall -Wextra examples/frame_put_stereo.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- chip_orb_detect against a plain C++ restatement of its definition, record for record (and, with an argument, the time of both)
$(LIBDIR)/orb_detect: examples/orb_detect.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- the same backlog with every frame put straight from its pair (detector, descriptor and block matcher on the device) and, next to
# it, composed on the host from chip_orb_detect_describe and chip_frame_put_stereo: same bits
$(LIBDIR)/orb_frame_put: examples/orb_frame_put.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/orb_frame_put.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- the same backlog with every frame put straight from its RAW pair (rectification, detector, descriptor and block matcher on the
# device) and, next to it, from the pair a plain C++ restatement of the rectification makes of it: same bits
$(LIBDIR)/frame_put_raw_stereo: examples/frame_put_raw_stereo.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/frame_put_raw_stereo.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- the same backlog put twice: by ONE chip_frame_put_raw_orb_stereo_batch and by the loop of single puts -- same bits, same matches --
# then read, dropped and put back from its records alone (chip_frame_put_records): the same matches again (with an argument, the times)
$(LIBDIR)/frame_put_batch: examples/frame_put_batch.cc $(LIBDIR)/libcerebro_host.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra examples/frame_put_batch.cc -o $@ -L$(LIBDIR) -lcerebro_host -lcerebro_hip -Wl,-rpath,'$$ORIGIN' -lpthread

# ---- the descriptor projection: a DB appended through chip_db_append_projected_f32 and, next to it, through a plain C++ restatement of
# the definition and chip_db_append_f64: same rows, same ticks (and, with an argument, the time of both at 32768 -> 4096).
# -ffp-contract=off: the restatement fuses where it says std::fma and nowhere else
$(LIBDIR)/append_projected: examples/append_projected.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -ffp-contract=off -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- the NetVLAD pooling: a DB appended through chip_db_append_vlad_f32 (directly, and through a projection) and, next to it, through a
# plain C++ restatement of the definition and chip_db_append_f64 / chip_db_append_projected_f32: same rows, same ticks (and, with an
# argument, the time of both).  -ffp-contract=off: the restatement fuses where it says std::fma and nowhere else
$(LIBDIR)/append_vlad: examples/append_vlad.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -ffp-contract=off -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- batched ingest: a DB filled by one chip_db_append_vlad_batch_f32 and, next to it, by the loop of chip_db_append_vlad_f32, straight to
# 8192-D and through a projection: same rows, same ticks (and, with an argument, the time of both)
$(LIBDIR)/append_batch: examples/append_batch.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- the causal self-join of a DB: ONE chip_query_batch_rows_f32 (a prefix per query, the queries gathered from DB rows on the device)
# against the loop of chip_query_batch_f32 with Q = 1 on rows read back: same bits (and, with an argument, the time of both)
$(LIBDIR)/self_join: examples/self_join.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- the tick records of a whole schedule: ONE chip_loop_ticks_bulk (many-query groups, certificate, exact rescoring, the accept rule)
# against the loop of chip_loop_tick and chip_query_rows: same bits in every field (and, with an argument, the time of both)
$(LIBDIR)/bulk_ticks: examples/bulk_ticks.cc include/cerebro_hip.h $(LIBDIR)/libcerebro_hip.so
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Iinclude $< -o $@ -L$(LIBDIR) -lcerebro_hip -Wl,-rpath,'$$ORIGIN'

# ---- the reference's own GMS matcher as a compiled checker (test infrastructure: tests/gms_ref_lib.py, tests/test_gms_ref_mirror.py).
# gms_matcher.{h,cpp} are compiled BY PATH from the reference tree against the stand-in oracle/ref_gms/opencv2/opencv.hpp; nothing of
# them is in this repository and oracle/_ref/ is git-ignored.  Plain IEEE arithmetic: no contraction, no fast-math, no -march.
# Where there is no reference tree the goal does nothing and succeeds (a library built elsewhere travels with the checkout;
# `make clean` leaves it alone for that reason).  -D_GLIBCXX_ASSERTIONS: a std::vector index outside its vector aborts.
REFERENCE  ?= /root/reference
REF_GMS    := $(REFERENCE)/src/utils/GMSMatcher
REFFLAGS   ?= -O2 -std=c++14 -ffp-contract=off -fPIC -D_GLIBCXX_ASSERTIONS
ifneq ($(wildcard $(REF_GMS)/gms_matcher.cpp),)
ref: oracle/_ref/libgms_ref.so
oracle/_ref/libgms_ref.so: oracle/ref_gms/gms_ref.cc oracle/ref_gms/opencv2/opencv.hpp $(REF_GMS)/gms_matcher.cpp $(REF_GMS)/gms_matcher.h
	@mkdir -p oracle/_ref
	$(CXX) $(REFFLAGS) -shared -Ioracle/ref_gms -I$(REF_GMS) oracle/ref_gms/gms_ref.cc $(REF_GMS)/gms_matcher.cpp -o $@
# the same matcher with its scale / rotation variants (tests/gms_modes_ref_lib.py, tests/test_gms_modes_mirror.py): this project's own
# wrapper tests/ref_gms_modes/gms_ref_modes.cc, the same two reference files by path, the same stand-in header
ref_modes: oracle/_ref/libgms_ref_modes.so
oracle/_ref/libgms_ref_modes.so: tests/ref_gms_modes/gms_ref_modes.cc oracle/ref_gms/opencv2/opencv.hpp $(REF_GMS)/gms_matcher.cpp $(REF_GMS)/gms_matcher.h
	@mkdir -p oracle/_ref
	$(CXX) $(REFFLAGS) -shared -Ioracle/ref_gms -I$(REF_GMS) tests/ref_gms_modes/gms_ref_modes.cc $(REF_GMS)/gms_matcher.cpp -o $@
else
ref:
	@echo "make ref: no reference tree at $(REFERENCE): nothing to build"
ref_modes:
	@echo "make ref_modes: no reference tree at $(REFERENCE): nothing to build"
endif

clean:
	rm -rf $(LIBDIR) oracle/_build tests/fakerccl/_build

.PHONY: all lib oracle host testlibs verify ref ref_modes clean
