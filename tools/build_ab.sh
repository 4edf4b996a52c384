#!/bin/bash
# Build an A/B library of some kernel sources: errors.cpp + SRC (default
# head_exact.hip; several sources separated by spaces) and the headers HDRS
# (default: every csrc/*.h of the revision) from a git revision, or from the
# working tree ("-"), into tools/_lib/libab_<name>.so, for
# tools/xbench_exact.py / tools/xbench_hgbwd.py / tools/ab_ray_reduce.py.
#   [SRC="render_fwd.hip render_bwd.hip"] [HDRS="common.h ray_stream.h"] \
#       bash tools/build_ab.sh NAME REV|- [extra hipcc flags...]
set -e
NAME=$1; REV=$2; shift 2
SRC=${SRC:-head_exact.hip}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=/tmp/avr_ab_$NAME
rm -rf $W && mkdir -p $W/src $W/inc
if [ -z "$HDRS" ]; then
  if [ "$REV" = "-" ]; then HDRS=$(cd $ROOT/avr_amd/csrc && ls *.h)
  else HDRS=$(git -C $ROOT ls-tree --name-only $REV:avr_amd/csrc | grep '\.h$'); fi
fi
for f in errors.cpp $SRC $HDRS; do
  if [ "$REV" = "-" ]; then cp $ROOT/avr_amd/csrc/$f $W/src/$f; else git -C $ROOT show $REV:avr_amd/csrc/$f > $W/src/$f; fi
done
if [ "$REV" = "-" ]; then cp $ROOT/include/avr_hip.h $W/inc/; else git -C $ROOT show $REV:include/avr_hip.h > $W/inc/avr_hip.h; fi
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -fno-gpu-rdc -Wno-unused-function -Wno-inline-asm --offload-compress -I$W/inc"
mkdir -p $ROOT/tools/_lib
OBJS=
for f in errors.cpp $SRC; do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c $W/src/$f -o $W/$f.o
  OBJS="$OBJS $W/$f.o"
done
/opt/rocm/bin/hipcc $FLAGS -shared $OBJS -o $ROOT/tools/_lib/libab_$NAME.so
echo built tools/_lib/libab_$NAME.so
