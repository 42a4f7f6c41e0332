#!/bin/bash
# Builds an A/B variant of lib/libndnet_amd.so with extra compile flags into
# lib/variants/libndnet_amd_NAME.so (select it with NDNET_AMD_LIB=...).
#   bash tools/build_variant.sh NAME "-DFLAG ..." ["pointnet-only flags"]
# The NDT, point-MLP and train units are compiled with the flags; every other
# object of the Makefile's OBJS is the default build's.
set -e
NAME=$1
FLAGS=$2
PNFLAGS=${3:-}
R=$(cd "$(dirname "$0")/.." && pwd)
P=$R/ndt-net_amd
V=build/v_$NAME
mkdir -p $P/$V $P/lib/variants
OBJS=$(sed -n 's/^OBJS = //p' $P/Makefile)
[ -n "$OBJS" ] || { echo "no 'OBJS = ...' line in $P/Makefile" >&2; exit 1; }
LINK=
SHARED=
for o in $OBJS; do
  case $o in
    build/ndt_kernels.o|build/pointnet_kernels.o|build/train_kernels.o) LINK="$LINK $V/$(basename $o)" ;;
    *) LINK="$LINK $o"; SHARED="$SHARED $o" ;;
  esac
done
make -C $P $SHARED
C="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable"
/opt/rocm/bin/hipcc $C -ffp-contract=off -fno-fast-math $FLAGS -c -o $P/$V/ndt_kernels.o $P/csrc/ndt_kernels.hip &
/opt/rocm/bin/hipcc $C $FLAGS $PNFLAGS -c -o $P/$V/pointnet_kernels.o $P/csrc/pointnet_kernels.hip &
/opt/rocm/bin/hipcc $C $FLAGS -c -o $P/$V/train_kernels.o $P/csrc/train_kernels.hip &
wait
(cd $P && /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o lib/variants/libndnet_amd_$NAME.so $LINK -lpthread)
echo "built $P/lib/variants/libndnet_amd_$NAME.so"
