#!/bin/bash
# Build a librm variant with extra -D flags for A/B timing (tools/ab_kernel.py).
#   tools/build_variant.sh NAME [-DFOO=1 ...]   -> tools/variants/librm_NAME.so
#   tools/build_variant.sh NAME --rev GITREV    -> librm built from a committed revision
#   tools/build_variant.sh NAME --patch F.diff  -> librm built with a patch applied
#   KOPT=-O3 tools/build_variant.sh NAME         -> the built-in kernels at another -O level
# Cost probes (a phase run twice, rm_kernels.hip): -DRM_DBL_MARCH, _BMARCH, _NORMAL, _SHADOW,
# _LIGHT, _GAMMA, _CAST (uv, castRay and the primary march's per-ray set-up) and _STORE (the
# AA sum, quantise and pack); -DRM_STATS=1 builds the counters of tools/stats_probe.py.
#                                                 (experiments live as patches, not knobs)
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/variants; mkdir -p "$out"
src=$root
if [ "$1" = "--rev" ]; then
  src=$(mktemp -d); git -C "$root" archive "$2" | tar -x -C "$src"; shift 2
fi
if [ "$1" = "--patch" ]; then
  p=$(cd "$(dirname "$2")" && pwd)/$(basename "$2")
  if [ "$src" = "$root" ]; then src=$(mktemp -d); (cd "$root" && tar -c --exclude=.git --exclude=gpurun_out --exclude=tools/variants .) | tar -x -C "$src"; fi
  (cd "$src" && patch -s -p1 < "$p"); shift 2
fi
pkg=opengl-raymarching-in-compute-shader_amd
flags="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -I$src/include $*"
b=$(mktemp -d)
for f in "$src/$pkg"/csrc/rm_api*.hip "$src/$pkg/csrc/rm_frame_math.hip"; do  # the C-ABI's files, whichever the revision has
  [ -f "$f" ] && { /opt/rocm/bin/hipcc $flags -c "$f" -o "$b/$(basename "$f" .hip).o" & }
done
/opt/rocm/bin/hipcc $flags -fno-slp-vectorize -c "$src/$pkg/csrc/rm_table.hip" -o "$b/rm_table.o" &
# rm_kernels.hip as the Makefile builds it (both objects without SLP; RM_PIXEL_SLP=1
# builds k_pixel with it, the round-3 flags), except
# for the RM_STATS build, whose counters must live in one code object
for d in "$@"; do  # a misspelt probe would silently time the plain build
  case "$d" in
    -DRM_DBL_*) case "${d%%=*}" in
        -DRM_DBL_MARCH|-DRM_DBL_BMARCH|-DRM_DBL_NORMAL|-DRM_DBL_SHADOW|-DRM_DBL_LIGHT|-DRM_DBL_GAMMA|-DRM_DBL_CAST|-DRM_DBL_STORE) ;;
        *) echo "build_variant: unknown cost probe $d" >&2; exit 1 ;;
      esac ;;
  esac
done
case "$*" in
  *RM_STATS*) /opt/rocm/bin/hipcc $flags -c "$src/$pkg/csrc/rm_kernels.hip" -o "$b/rm_kernels.o" & ;;
  *) lean=-DRM_LEAN_FIXED_WORK=1; case "$*" in *RM_LEAN_FIXED_WORK*) lean=;; esac  # as the Makefile, unless given
     grep -q RM_LEAN_FIXED_WORK "$src/$pkg/csrc/rm_kernels.hip" || lean=
     fast=-DRM_FAST_STEPS=1; case "$*" in *RM_FAST_STEPS*) fast=;; esac
     grep -q RM_FAST_STEPS "$src/$pkg/csrc/rm_kernels.hip" || fast=
     pslp=-fno-slp-vectorize; [ -n "$RM_PIXEL_SLP" ] && pslp=-fslp-vectorize
     /opt/rocm/bin/hipcc $flags ${KOPT:--O2} $pslp -DRM_KERNELS_PIXEL_ONLY -c "$src/$pkg/csrc/rm_kernels.hip" -o "$b/rm_kernels.o" &
     /opt/rocm/bin/hipcc $flags ${KOPT:--O2} -fno-slp-vectorize -DRM_KERNELS_AA_ONLY $lean $fast -c "$src/$pkg/csrc/rm_kernels.hip" -o "$b/rm_kernels_aa.o" & ;;
esac
# the ray-query, G-buffer, SDF-query, adaptive and mesh kernels, as the Makefile builds them
# (absent in older revisions)
for f in rm_trace rm_gbuffer rm_sdf rm_adaptive rm_adaptive_edges rm_mesh rm_pattern rm_adaptive_pattern; do
  [ -f "$src/$pkg/csrc/$f.hip" ] && { /opt/rocm/bin/hipcc $flags ${KOPT:--O2} -fno-slp-vectorize -c "$src/$pkg/csrc/$f.hip" -o "$b/$f.o" & }
done
for f in rm_table_trace rm_table_gbuffer rm_table_sdf rm_table_adaptive rm_table_pattern rm_table_adaptive_pattern; do
  [ -f "$src/$pkg/csrc/$f.hip" ] && { /opt/rocm/bin/hipcc $flags -fno-slp-vectorize -mllvm -amdgpu-inline-max-bb=8000 -c "$src/$pkg/csrc/$f.hip" -o "$b/$f.o" & }
done
/opt/rocm/bin/hipcc $flags -x c++ -c "$src/$pkg/csrc/rm_host.cpp" -o "$b/rm_host.o" &
[ -f "$src/$pkg/csrc/rm_comm.cpp" ] && { /opt/rocm/bin/hipcc $flags -x hip -c "$src/$pkg/csrc/rm_comm.cpp" -o "$b/rm_comm.o" & }
if [ -f "$src/$pkg/csrc/rm_jit.hip" ]; then  # per-table hiprtc kernels: embed the table sources
  c=$src/$pkg/csrc
  python3 "$src/$pkg/tools/embed_sources.py" "$b/rm_jit_src.inc" rm_table.hip=$c/rm_table.hip \
    rm_internal.hpp=$c/rm_internal.hpp rm_scene.hpp=$c/rm_scene.hpp rm_fastmath.hpp=$c/rm_fastmath.hpp \
    $( [ -f "$c/rm_shard.hpp" ] && echo rm_shard.hpp=$c/rm_shard.hpp ) \
    ../../include/rm_api.h=$src/include/rm_api.h
  /opt/rocm/bin/hipcc $flags -I"$b" -c "$c/rm_jit.hip" -o "$b/rm_jit.o" &
fi
for j in $(jobs -p); do wait "$j" || { echo "build_variant: a compile failed" >&2; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out/librm_$name.so" "$b"/*.o -lhiprtc -ldl
rm -rf "$b"; [ "$src" != "$root" ] && rm -rf "$src"
echo "$out/librm_$name.so"
