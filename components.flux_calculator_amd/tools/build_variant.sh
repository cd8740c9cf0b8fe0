#!/bin/bash
# build_variant.sh OUTDIR [hipcc -D flags...] -- an A/B copy of libfcx.so built with extra
# compile-time flags (measurement tool; the product library is built by the Makefile).
set -e
HERE="$(cd "$(dirname "$0")/.." && pwd)"
OUT="$1"; shift
mkdir -p "$OUT/obj"
FLAGS="-DFCX_AB_BUILD --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -I$HERE/csrc -I$HERE/../include"
# the Makefile's translation units, side by side; each job is waited for by its pid, so a
# failed compile fails the script
UNITS="fcx_kernels fcx_kernels_wide fcx_kernels_cr fcx_integrals fcx_atmos_terms fcx_engine"
OBJS=""
PIDS=""
for u in $UNITS; do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c "$HERE/csrc/$u.hip" -o "$OUT/obj/$u.o" &
  PIDS="$PIDS $!"
  OBJS="$OBJS $OUT/obj/$u.o"
done
for p in $PIDS; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT/libfcx.so" $OBJS
python3 "$HERE/tools/unversion_needed.py" "$OUT/libfcx.so"
