#!/bin/bash
# A VARIANT of libl2o_hip.so with extra compiler flags (A/B and ablation builds): the same translation units and flags as
# open_l2o_amd/csrc/Makefile (SRCS there; the kernels of csrc/l2o_ilp_kernels.h under max-ilp), the compiles in parallel.
#   bash scripts/build_lib.sh build/var/lib_x.so -DL2O_SOMETHING=1 [more flags]      (l2o_build_id() of the result = the file's name)
# A variant is only worth measuring if it is what its name says: the object directory starts empty (no object of an earlier,
# failed build can be linked), each compile's exit status is checked on its own (a bare `wait` returns 0 whatever the
# jobs did), the output is replaced only by a successful link, and the object directory goes away on every exit.
set -e
OUT=$(realpath -m "$1"); shift
cd "$(dirname "$0")/../open_l2o_amd/csrc"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -mllvm -amdgpu-mfma-vgpr-form -fno-slp-vectorize"
UNITS="l2o_core l2o_unroll l2o_bwd l2o_mlp l2o_nets l2o_confocal l2o_twin l2o_kernels_ilp"
OBJ=$(dirname "$OUT")/obj_$(basename "$OUT" .so)
rm -rf "$OBJ"
mkdir -p "$OBJ"
trap 'rm -rf "$OBJ"' EXIT
PIDS=""
for u in $UNITS; do
  EXTRA=""
  [ $u = l2o_core ] && EXTRA="-DL2O_BUILD_ID=\"$(basename "$OUT" .so)\""          # (the unit that defines l2o_build_id)
  [ $u = l2o_kernels_ilp ] && EXTRA="-Wno-unused-variable -mllvm -amdgpu-sched-strategy=max-ilp"
  /opt/rocm/bin/hipcc $FLAGS $EXTRA "$@" -c $u.hip -o "$OBJ/$u.o" &
  PIDS="$PIDS $!"
done
RC=0
for p in $PIDS; do wait $p || RC=$?; done
if [ $RC -ne 0 ]; then echo "build_lib.sh: a compile failed (status $RC): $OUT not written" >&2; exit $RC; fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -Wl,--no-undefined "$OBJ"/*.o -o "$OBJ/out.so"
mv -f "$OBJ/out.so" "$OUT"
