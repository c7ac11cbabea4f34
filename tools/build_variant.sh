#!/bin/bash
# usage: tools/build_variant.sh <commit|WORK> <tag> [extra compiler flags]  -> ra-slam_amd/csrc/build/libratsdf_<tag>.so (same C ABI; select with RATSDF_LIB)
# e.g. tools/build_variant.sh WORK wt3 -DRATSDF_WT_STORES=3 (store flavours of the bulk streams, kernels_alloc.h; `make wt WT=3` builds the same)
# Same-box A/B of engine variants: bash tools/ab_env.sh N "<bench args>" RATSDF_LIB=$PWD/ra-slam_amd/csrc/build/libratsdf_a.so RATSDF_LIB=...
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
c=$1; tag=$2; shift 2; extra="$*"
T=$(mktemp -d)
if [ "$c" = WORK ]; then cp -r $ROOT/ra-slam_amd/csrc $T/csrc; mkdir -p $T/include; cp $ROOT/include/ratsdf.h $T/include/; mv $T/csrc $T/x; mkdir -p $T/ra-slam_amd; mv $T/x $T/ra-slam_amd/csrc
else (cd $ROOT && git archive $c ra-slam_amd/csrc include) | tar -x -C $T; fi
rm -rf $T/ra-slam_amd/csrc/build
make -C $T/ra-slam_amd/csrc ${extra:+HIPCC="${HIPCC:-/opt/rocm/bin/hipcc} $extra"} > $T/log 2>&1 || { tail $T/log; exit 1; }
cp $T/ra-slam_amd/csrc/build/libratsdf.so $ROOT/ra-slam_amd/csrc/build/libratsdf_$tag.so
rm -rf $T
echo "built libratsdf_$tag.so from $c"
