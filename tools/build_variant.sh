#!/bin/bash
# Build a librm variant for A/B timing (tools/ab_kernel.py), by the Makefile's own recipe.
#   tools/build_variant.sh NAME [-DFOO=1 ...]   -> tools/variants/librm_NAME.so
#   tools/build_variant.sh NAME --rev GITREV    -> librm built from a committed revision
#   tools/build_variant.sh NAME --patch F.diff  -> librm built with a patch applied
#   KOPT=-O3 tools/build_variant.sh NAME         -> the built-in kernels at another -O level
#   RM_PIXEL_SLP=1 tools/build_variant.sh NAME   -> k_pixel with SLP vectorisation (round 3)
#   BUILD=DIR                                    -> the objects go there and stay (default: a
#                                                   temporary directory, removed afterwards)
#   VARIANTS=DIR                                 -> the library goes there, not to tools/variants
# Cost probes (a phase run twice, rm_kernels.hip): -DRM_DBL_MARCH, _BMARCH, _NORMAL, _SHADOW,
# _LIGHT, _GAMMA, _CAST (uv, castRay and the primary march's per-ray set-up) and _STORE (the
# AA sum, quantise and pack); -DRM_STATS=1 builds the counters of tools/stats_probe.py.
#                                                 (experiments live as patches, not knobs)
# The -D flags reach every object as the Makefile's XFLAGS.  A revision or a patched tree is
# built by its own Makefile: the parent of an A/B is built the way the parent shipped.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=${VARIANTS:-$root/tools/variants}; mkdir -p "$out"; out=$(cd "$out" && pwd)
src=$root; b=
trap '[ -n "$BUILD" ] || [ -z "$b" ] || rm -rf "$b"; [ "$src" = "$root" ] || rm -rf "$src"' EXIT
if [ "$1" = "--rev" ]; then
  src=$(mktemp -d); git -C "$root" archive "$2" | tar -x -C "$src"; shift 2
fi
if [ "$1" = "--patch" ]; then
  p=$(cd "$(dirname "$2")" && pwd)/$(basename "$2")
  if [ "$src" = "$root" ]; then src=$(mktemp -d); (cd "$root" && tar -c --exclude=.git --exclude=gpurun_out --exclude=tools/variants .) | tar -x -C "$src"; fi
  (cd "$src" && patch -s -p1 < "$p"); shift 2
fi
for d in "$@"; do  # a misspelt probe would silently time the plain build
  case "$d" in
    -DRM_DBL_*) case "${d%%=*}" in
        -DRM_DBL_MARCH|-DRM_DBL_BMARCH|-DRM_DBL_NORMAL|-DRM_DBL_SHADOW|-DRM_DBL_LIGHT|-DRM_DBL_GAMMA|-DRM_DBL_CAST|-DRM_DBL_STORE) ;;
        *) echo "build_variant: unknown cost probe $d" >&2; exit 1 ;;
      esac ;;
  esac
done
b=${BUILD:-$(mktemp -d)}; mkdir -p "$b"; b=$(cd "$b" && pwd)
pkg=opengl-raymarching-in-compute-shader_amd
if ! grep -q XFLAGS "$src/Makefile"; then
  # a revision from before the one recipe: its Makefile takes LIBRM but neither XFLAGS, KOPT
  # nor BUILD, and builds in its own tree
  if [ -n "$*$KOPT$RM_PIXEL_SLP" ]; then
    echo "build_variant: this revision's Makefile has no XFLAGS: it would ignore '$* $KOPT $RM_PIXEL_SLP' and build the plain library" >&2
    exit 1
  fi
  ln -s "$b" "$src/$pkg/build"
fi
make -C "$src" -j"${MAX_JOBS:-8}" librm BUILD="$b" LIBRM="$out/librm_$name.so" XFLAGS="$*" \
  ${KOPT:+KOPT="$KOPT"} ${RM_PIXEL_SLP:+RM_PIXEL_SLP="$RM_PIXEL_SLP"} >&2
echo "$out/librm_$name.so"
