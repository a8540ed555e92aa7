#!/bin/bash
# Build a libpong_ga.so variant with extra defines for one translation unit
# (default pong_ga.hip: k_service & co.; PG_TU=pg_wide.hip for k_wide),
# linking the main build's other objects: ab/lib_NAME.so.
# usage: [PG_TU=pg_wide.hip] tools/build_variant.sh NAME [-DFLAG=VALUE ...]   (run the main build first)
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
C=$ROOT/neuro-genetic-pong-self-play_amd/csrc
TU=${PG_TU:-pong_ga.hip}
mkdir -p $ROOT/ab
# the main build's per-source flags for this unit (pong_amd/build.py SOURCE_FLAGS: the machine scheduler);
# PG_SCHED names another scheduler
SFLAG=$(cd $ROOT/neuro-genetic-pong-self-play_amd && python3 -c "from pong_amd import build as B; print(' '.join(B.SOURCE_FLAGS.get('$TU', [])))")
[ -n "$PG_SCHED" ] && SFLAG="-mllvm -amdgpu-sched-strategy=$PG_SCHED"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall \
  -Wno-unused-function -I $ROOT/include $SFLAG "$@" -c -o /tmp/pg_variant_$NAME.o $C/$TU
OBJS="/tmp/pg_variant_$NAME.o"
for o in $C/*.o; do
  [ "$(basename $o .o).hip" = "$TU" ] || OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $ROOT/ab/lib_$NAME.so $OBJS
echo $ROOT/ab/lib_$NAME.so
