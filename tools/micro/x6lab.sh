#!/bin/bash
# lab builds of the library with F2G_X6LAB ablations (gemm_common.h lists the bits) -> tools/micro/libx6lab<N>.so,
# loaded through F2G_LIB_PATH.  Only the sources whose code depends on the switch are compiled again -- they name
# it, or use what gemm_common.h derives from it; the other objects are the product build's.  Run `make` in csrc first.
set -e
cd "$(dirname "$0")/../../flow2gan_amd/csrc"
OUT=../../tools/micro
LABSRCS=$(grep -lE 'F2G_X6LAB|X6LAB_|X6PROF_|lds_barrier|split3x4' *.hip)
OBJS=$(ls *.o | grep -vxF "$(printf '%s\n' $LABSRCS | sed 's/\.hip$/.o/')")
for v in "$@"; do
  ( LABOBJS=
    for s in $LABSRCS; do
      o=$OUT/x6lab$v.${s%.hip}.o
      /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -DF2G_X6LAB=$v -c $s -o $o
      LABOBJS="$LABOBJS $o"
    done
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT/libx6lab$v.so $OBJS $LABOBJS && rm -f $LABOBJS ) &
done
wait
ls -la $OUT/libx6lab*.so
