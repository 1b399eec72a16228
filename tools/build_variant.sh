#!/bin/bash
# Build an experimental variant of the HIP library next to the in-tree one:
#   tools/build_variant.sh NAME "-DFLAG1 -DFLAG2=3" [plan indices ... | main | side_N]
# Only the listed translation units are recompiled with the flags (default: 3 6 11 = the 8192-,
# 28672- and 7168-point plans of the Llama-3-70B shapes); every other object comes from the
# in-tree build (run `make -C shardmerge_amd/csrc -j8` first).  Result: exp_libs/lib_NAME.so
# (git-ignored, travels with gpurun); use with SHARDMERGE_HIP_LIB=... (tools/ab_kprof.sh).
set -e
NAME=$1; FLAGS=$2; shift 2
UNITS=${@:-3 6 11}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=$ROOT/shardmerge_amd/csrc
OUT=$ROOT/exp_libs; mkdir -p $OUT/obj_$NAME
# the Makefile's own rules and per-unit flags, objects into a folder of this variant
targets=""
for u in $UNITS; do
    case $u in
        main|side_*) targets="$targets $OUT/obj_$NAME/$u.o" ;;
        *) targets="$targets $OUT/obj_$NAME/inst_$u.o" ;;
    esac
done
rm -f $targets      # (the flags may differ from this variant's last build)
make -C $SRC -j8 BUILD=$OUT/obj_$NAME EXTRA="$FLAGS" $targets
objs=""
for f in $SRC/build/main.o $SRC/build/side_[0-9]*.o $SRC/build/inst_*.o; do
    b=$(basename $f)
    if [ -f $OUT/obj_$NAME/$b ]; then objs="$objs $OUT/obj_$NAME/$b"; else objs="$objs $f"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $OUT/lib_$NAME.so
echo "built $OUT/lib_$NAME.so ($UNITS with: $FLAGS)"
