# Build recipe for librm (HIP, gfx950), the CPU oracle and the headless driver.
#   make            -> librm.so + oracle + rm_frameloop
#   make librm      -> opengl-raymarching-in-compute-shader_amd/librm.so
#   make oracle     -> oracle/_build/librm_oracle.so (test infrastructure)
#   make goldens    -> oracle/_ref/gen_camera_goldens (needs /root/reference; container only)
#   make glsl_ref   -> oracle/_ref/glsl_ref{,_glm,_ubsan}: the reference's shader as C++ (same condition)
# Built artefacts stay in-tree (git-ignored) so they travel to the GPU box.

HIPCC    ?= /opt/rocm/bin/hipcc
CC       ?= gcc
CXX      ?= g++
PKG      := opengl-raymarching-in-compute-shader_amd
CSRC     := $(PKG)/csrc
ARCH     ?= gfx950
# -ffp-contract=off: no FMA contraction (HIP's device default is 'fast'), so every
# float op is one IEEE op in source order; HIP keeps correctly-rounded f32
# sqrt/div by default (-fhip-fp32-correctly-rounded-divide-sqrt).
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
            -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-result
OFLAGS   := -std=c11 -O3 -ffp-contract=off -fno-fast-math -fopenmp -fPIC -Wall -Wextra

LIBRM    := $(PKG)/librm.so
ORACLE   := oracle/_build/librm_oracle.so
DRIVER   := $(PKG)/rm_frameloop

# librm's objects, in link order: the link line and the sanitizer build's objects
# come from this one list.
RM_OBJS  := rm_api rm_api_comm rm_api_graph rm_frame_math rm_kernels rm_kernels_aa rm_table rm_jit rm_host rm_comm \
            rm_api_trace rm_trace rm_table_trace rm_api_gbuffer rm_gbuffer rm_table_gbuffer \
            rm_api_sdf rm_sdf rm_table_sdf rm_api_adaptive rm_adaptive rm_table_adaptive rm_adaptive_edges \
            rm_api_mesh rm_mesh rm_api_query rm_api_pattern rm_pattern rm_table_pattern \
            rm_adaptive_pattern rm_table_adaptive_pattern
RM_HDRS  := $(CSRC)/rm_scene.hpp $(CSRC)/rm_shard.hpp $(CSRC)/rm_fastmath.hpp $(CSRC)/rm_internal.hpp $(CSRC)/rm_jit.hpp $(CSRC)/rm_comm.hpp \
            $(CSRC)/rm_ctx.hpp $(CSRC)/rm_frame_math.hpp $(CSRC)/rm_trace.hpp $(CSRC)/rm_builtin_fast.hpp $(CSRC)/rm_table_lit.hpp $(CSRC)/rm_sdf.hpp $(CSRC)/rm_sdf_args.hpp $(CSRC)/rm_adaptive_args.hpp $(CSRC)/rm_adaptive_tile.hpp \
            $(CSRC)/rm_mesh_args.hpp $(CSRC)/rm_pattern_args.hpp $(CSRC)/rm_adaptive_pattern.hpp \
            include/rm_api.h Makefile
# The table kernel's sources, embedded in librm.so for hiprtc (rm_jit.hip), under
# the names they #include each other by.
JIT_SRCS := rm_table.hip=$(CSRC)/rm_table.hip rm_internal.hpp=$(CSRC)/rm_internal.hpp \
            rm_scene.hpp=$(CSRC)/rm_scene.hpp rm_shard.hpp=$(CSRC)/rm_shard.hpp \
            rm_fastmath.hpp=$(CSRC)/rm_fastmath.hpp \
            ../../include/rm_api.h=include/rm_api.h

.PHONY: all librm oracle driver goldens glsl_ref asan clean
all: librm oracle driver
librm: $(LIBRM)
oracle: $(ORACLE)
driver: $(DRIVER)

$(PKG)/build/%.o: $(CSRC)/%.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# rm_kernels.hip is built twice: k_pixel + k_unshard (rm_kernels.o),
# and k_sample alone (rm_kernels_aa.o), both without SLP vectorisation: pairing
# f32 adds / muls into packed v_pk_* ops costs register moves to form the pairs
# (k_sample: 3.9 % slower per cfg3 frame), and since round 3's issue-slot changes
# it makes k_pixel spill 9 VGPRs (32 B of scratch per lane; none without SLP,
# round 4).  Both at -O2, which measured 0.4-2 % faster than -O3 for each (round
# 3, profiles/r03_compiler_ab.txt).  k_sample's object alone takes the lean forms
# of the once-per-wave and once-per-hit code (-DRM_LEAN_FIXED_WORK=1, DESIGN §4.4
# item 23; rm_kernels.hip) and the downward step loop as a wave-uniform loop
# (-DRM_FAST_STEPS=1, item 24).
KFLAGS   := $(HIPFLAGS) -O2 -fno-slp-vectorize
$(PKG)/build/rm_kernels.o: $(CSRC)/rm_kernels.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(KFLAGS) -DRM_KERNELS_PIXEL_ONLY -c $< -o $@

$(PKG)/build/rm_kernels_aa.o: $(CSRC)/rm_kernels.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(KFLAGS) -DRM_KERNELS_AA_ONLY -DRM_LEAN_FIXED_WORK=1 -DRM_FAST_STEPS=1 -c $< -o $@

# the scene-table kernels without SLP vectorisation too (generic -2.7 %, the
# hiprtc-specialised ones get the same flag in rm_jit.hip: -6.5 % per cfg3 frame)
$(PKG)/build/rm_table.o: $(CSRC)/rm_table.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize -c $< -o $@

# The query and output families in objects of their own, so
# that rm_kernels.o / rm_kernels_aa.o / rm_table.o are what they are without
# them.  The built-in scene's (ray queries, the G-buffer frame kernels, SDF field
# queries, adaptive supersampling, sample-pattern frames, pattern refinement) include the render kernels' source for its
# device code alone and take that source's flags; the scene-independent ones
# (the geometry-edge classifier, mesh extraction) take the same flags.
BUILTIN_FAMS := rm_trace rm_gbuffer rm_sdf rm_adaptive rm_pattern rm_adaptive_pattern
PLAIN_FAMS   := rm_adaptive_edges rm_mesh
$(BUILTIN_FAMS:%=$(PKG)/build/%.o): $(CSRC)/rm_kernels.hip
$(BUILTIN_FAMS:%=$(PKG)/build/%.o) $(PLAIN_FAMS:%=$(PKG)/build/%.o): $(PKG)/build/%.o: $(CSRC)/%.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(KFLAGS) -c $< -o $@

# The scene-table halves include rm_table.hip in the same way, with rm_table.o's
# flags and one more: k_table_trace holds the table march twice over (the fast
# lanes' and the literal path's): past the AMDGPU inliner's default cap on a
# caller's basic blocks (1100) tmarch stays a call, and a call takes the staged
# Table and its result through scratch memory (432 B per lane; none with the cap
# raised).
TRACE_INLINE := -mllvm -amdgpu-inline-max-bb=8000
TABLE_FAMS   := rm_table_trace rm_table_gbuffer rm_table_sdf rm_table_adaptive rm_table_pattern \
                rm_table_adaptive_pattern
$(TABLE_FAMS:%=$(PKG)/build/%.o): $(PKG)/build/%.o: $(CSRC)/%.hip $(CSRC)/rm_table.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -fno-slp-vectorize $(TRACE_INLINE) -c $< -o $@

$(PKG)/build/rm_jit_src.inc: $(CSRC)/rm_table.hip $(RM_HDRS) $(PKG)/tools/embed_sources.py
	@mkdir -p $(dir $@)
	python3 $(PKG)/tools/embed_sources.py $@ $(JIT_SRCS)

$(PKG)/build/rm_jit.o: $(CSRC)/rm_jit.hip $(RM_HDRS) $(PKG)/build/rm_jit_src.inc
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -I$(PKG)/build -c $< -o $@

$(PKG)/build/rm_host.o: $(CSRC)/rm_host.cpp $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -x c++ -c $< -o $@

# RCCL is bound at run time (dlopen, rm_comm.cpp): librm does not link it.
$(PKG)/build/rm_comm.o: $(CSRC)/rm_comm.cpp $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(LIBRM): $(RM_OBJS:%=$(PKG)/build/%.o)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -lhiprtc -ldl

$(ORACLE): oracle/rm_oracle.c oracle/rm_oracle.h include/rm_api.h
	@mkdir -p $(dir $@)
	$(CC) $(OFLAGS) -shared -o $@ oracle/rm_oracle.c -lm

$(DRIVER): $(PKG)/tools/rm_frameloop.cpp include/rm/camera.hpp include/rm/input.hpp include/rm/texture.hpp $(LIBRM)
	$(CXX) -std=c++17 -O2 -Wall -Iinclude -o $@ $< -L$(PKG) -lrm -Wl,-rpath,'$$ORIGIN'

# Camera goldens from the reference's vendored GLM 0.9.8.5 (third-party, in
# /root/reference/includes/glm).  Output binary only under oracle/_ref/.
REF ?= /root/reference
goldens: oracle/_ref/gen_camera_goldens oracle/_ref/gen_input_goldens oracle/_ref/glsl_ref oracle/_ref/glsl_ref_glm
	oracle/_ref/gen_camera_goldens > tests/golden/camera_goldens.json
	oracle/_ref/gen_input_goldens > tests/golden/input_goldens.json

oracle/_ref/gen_input_goldens: oracle/gen_input_goldens.cpp
	@mkdir -p oracle/_ref
	$(CXX) -std=c++11 -O2 -ffp-contract=off -I$(REF)/includes -o $@ $<

oracle/_ref/gen_camera_goldens: oracle/gen_camera_goldens.cpp
	@mkdir -p oracle/_ref
	$(CXX) -std=c++11 -O2 -ffp-contract=off -I$(REF)/includes -o $@ $<

# The reference's compute shader run as C++: its text, rewritten by
# token rules only (oracle/glsl_rewrite.py) into oracle/_ref/, compiled against
# the reference's GLM behind oracle/glsl_prelude.hpp.  The rewritten text and the
# binaries are the reference's program: they stay under oracle/_ref/ (git-ignored).
#   glsl_ref        GLM's built-ins, except those DESIGN §2 defines otherwise
#   glsl_ref_glm    GLM's built-ins only (glsl_ref_glm_mix / _minmax: one family
#                   handed back, for tools/ref_builtin_diff.py)
#   glsl_ref_ubsan  glsl_ref under UBSan; a stand-alone host program, run by
#                   tests/golden/make_reference_goldens.py only
GLSL_SRC   := $(REF)/shaders/computeShader.glsl
GLSL_INC   := oracle/_ref/computeShader.inc
GLSL_DEPS  := oracle/glsl_ref_main.cpp oracle/glsl_prelude.hpp include/rm_api.h $(GLSL_INC)
GLSL_FLAGS := -std=c++20 -O2 -ffp-contract=off -isystem $(REF)/includes -DGLSL_REF_SHADER='"_ref/computeShader.inc"'
glsl_ref: oracle/_ref/glsl_ref oracle/_ref/glsl_ref_glm oracle/_ref/glsl_ref_ubsan

$(GLSL_INC): $(GLSL_SRC) oracle/glsl_rewrite.py
	@mkdir -p oracle/_ref
	python3 oracle/glsl_rewrite.py $< $@

oracle/_ref/glsl_ref: $(GLSL_DEPS)
	$(CXX) $(GLSL_FLAGS) -o $@ $<
oracle/_ref/glsl_ref_glm: $(GLSL_DEPS)
	$(CXX) $(GLSL_FLAGS) -DGLSL_REF_PURE_GLM -o $@ $<
oracle/_ref/glsl_ref_glm_mix: $(GLSL_DEPS)
	$(CXX) $(GLSL_FLAGS) -DGLSL_REF_GLM_MIX -o $@ $<
oracle/_ref/glsl_ref_glm_minmax: $(GLSL_DEPS)
	$(CXX) $(GLSL_FLAGS) -DGLSL_REF_GLM_MINMAX -o $@ $<
oracle/_ref/glsl_ref_ubsan: $(GLSL_DEPS)
	$(CXX) $(GLSL_FLAGS) -g -fsanitize=undefined,float-cast-overflow -o $@ $<

# ---- host sanitizer build: CPU suite under ASan + UBSan ---------
# librm's host code (the C-ABI, the table compiler and its bounds, the uniform
# lookup, input replay, the shard map, the hiprtc driver) and the oracle, built
# with AddressSanitizer + UndefinedBehaviorSanitizer, every report fatal.  The
# sanitizers are on the host side only (-Xarch_host; the device code is the
# production build's): this build is for the CPU container, where no kernel runs
# anyway (GPU sanitizers are not available).  tests/test_sanitizers.py runs the
# host-logic CPU tests against it (LD_PRELOAD of clang's ASan runtime, RM_LIBRM,
# RM_ORACLE).
LLVM     ?= /opt/rocm/lib/llvm
ASAN_DIR := $(PKG)/build/asan
ASANLIB  := $(ASAN_DIR)/librm.so
ASANORC  := oracle/_build/librm_oracle_asan.so
SANHOST  := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
            -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer
SANFLAGS := -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer
ASAN_OBJS := $(RM_OBJS:%=$(ASAN_DIR)/%.o)
asan: $(ASANLIB) $(ASANORC)

$(BUILTIN_FAMS:%=$(ASAN_DIR)/%.o): $(CSRC)/rm_kernels.hip
$(TABLE_FAMS:%=$(ASAN_DIR)/%.o): $(CSRC)/rm_table.hip
$(ASAN_DIR)/%.o: $(CSRC)/%.hip $(RM_HDRS) $(PKG)/build/rm_jit_src.inc
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -O1 -g $(SANHOST) -I$(PKG)/build -c $< -o $@
$(ASAN_DIR)/rm_kernels.o: $(CSRC)/rm_kernels.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -O1 -g $(SANHOST) -DRM_KERNELS_PIXEL_ONLY -c $< -o $@
$(ASAN_DIR)/rm_kernels_aa.o: $(CSRC)/rm_kernels.hip $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -O1 -g $(SANHOST) -DRM_KERNELS_AA_ONLY -DRM_LEAN_FIXED_WORK=1 -DRM_FAST_STEPS=1 -c $< -o $@
$(ASAN_DIR)/rm_host.o: $(CSRC)/rm_host.cpp $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(LLVM)/bin/clang++ -std=c++17 -O1 -g -fPIC -ffp-contract=off $(SANFLAGS) -c $< -o $@
$(ASAN_DIR)/rm_comm.o: $(CSRC)/rm_comm.cpp $(RM_HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -O1 -g $(SANHOST) -x hip -c $< -o $@
$(ASANLIB): $(ASAN_OBJS)
	$(LLVM)/bin/clang++ -shared -fPIC $(SANFLAGS) -shared-libsan -o $@ $^ -L/opt/rocm/lib -lamdhip64 -lhiprtc -ldl \
	  -Wl,-rpath,/opt/rocm/lib
$(ASANORC): oracle/rm_oracle.c oracle/rm_oracle.h include/rm_api.h
	@mkdir -p $(dir $@)
	$(LLVM)/bin/clang -std=c11 -O1 -g -ffp-contract=off -fno-fast-math -fopenmp -fPIC -Wall $(SANFLAGS) \
	  -shared -shared-libsan -o $@ oracle/rm_oracle.c -lm -L$(LLVM)/lib -Wl,-rpath,$(LLVM)/lib

clean:
	rm -rf $(PKG)/build $(LIBRM) $(DRIVER) oracle/_build oracle/_ref
