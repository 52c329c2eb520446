#!/bin/bash
# Static ISA stats of the CMUX loop of the P-GATE pair kernel (blind_rotate_fft_pair_kernel<2, false, true>, the
# instantiation bench.py runs): resources of the kernel, then the f64, non-f64 VALU, scalar, LDS, wait, M0-write, LDS-DMA and register key-load counts of the loop body (both
# branches of the partial-sum exchange counted).  Compiles with the Makefile's flags for pbs_fft.o; needs no GPU.
# usage: tools/isa_pair_stats.sh [-k out.s] [extra hipcc flags, e.g. -DFFT_DMASTAMP=1 ...]
#   -k out.s: keep the loop body (its line numbers are those of the kernel's listing) for reading
set -eu
cd "$(dirname "$0")/.."
KEEP=
if [ "${1:-}" = "-k" ]; then KEEP=$2; shift 2; fi
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SCHED=$(make -s -C tfhe_amd -pn 2>/dev/null | sed -n 's/^SCHED_FFT ?*= //p' | head -1)
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
$HIPCC "$@" -O3 -fPIC -std=c++17 --offload-arch=gfx950 -mcode-object-version=5 -Wall -Wno-unused-function $SCHED \
  --cuda-device-only -S tfhe_amd/csrc/pbs_fft.hip -o "$D/k.s" 2> "$D/err.txt" || { tail -20 "$D/err.txt"; exit 1; }
SYM=_ZN4tfhe4fftk28blind_rotate_fft_pair_kernelILi2ELb0ELb1E
# the kernel: from its label to the end of its resource comment block
awk -v sym="$SYM" 'index($0, sym) == 1 && /:/ { on = 1 } on { print } on && /^; Occupancy/ { exit }' "$D/k.s" > "$D/kern.s"
[ -s "$D/kern.s" ] || { echo "kernel $SYM... not found"; exit 1; }
# the CMUX loop: the widest backward branch of the kernel (label line .. branch line)
awk '/^\.LBB[0-9_]+:/ { l = $1; sub(/:.*/, "", l); at[l] = NR }
     /^\ts_c?branch[a-z0-9_]* \.LBB/ { t = $2; if (t in at && NR - at[t] > best) { best = NR - at[t]; lo = at[t]; hi = NR } }
     END { print lo, hi }' "$D/kern.s" > "$D/range.txt"
read LO HI < "$D/range.txt"
sed -n "${LO},${HI}p" "$D/kern.s" > "$D/loop.s"
cnt() { grep -cE "^\s+($1)(_e32|_e64)?(\s|$)" "$D/loop.s" || true; }
num() { sed -n "s/^; $1: \([0-9]*\).*/\1/p" "$D/kern.s" | head -1; }
SPILL=$(grep -A40 "\.name: *$SYM" "$D/k.s" | sed -n 's/.*\.vgpr_spill_count: *\([0-9]*\).*/\1/p' | head -1)
echo "kernel: VGPRs $(num NumVgprs), spilled ${SPILL:-?}, scratch $(num ScratchSize) B, LDS $(num LDSByteSize) B, occupancy $(num Occupancy)"
echo "CMUX loop: lines $LO-$HI of the kernel's listing"
echo "  v_add_f64 $(cnt v_add_f64)  v_mul_f64 $(cnt v_mul_f64)  v_fma_f64+v_fmac_f64 $(cnt 'v_fma_f64|v_fmac_f64')  v_floor_f64 $(cnt v_floor_f64)"
echo "  non-f64 VALU $(grep -E '^\s+v_' "$D/loop.s" | grep -cvE '^\s+v_(add|mul|fma|fmac|floor)_f64(_e32|_e64)?(\s|$)' || true)  (every v_* but the four above)  scalar $(grep -cE '^\s+s_' "$D/loop.s" || true)  (every s_*, waits and s_nop included)"
echo "  ds_read_b128 $(cnt ds_read_b128)  ds_write_b128 $(cnt ds_write_b128)  ds_read_b64 $(cnt ds_read_b64)  ds_write_b64 $(cnt ds_write_b64)"
echo "  s_waitcnt $(cnt s_waitcnt)  of which lgkmcnt(0) $(grep -cE '^\s+s_waitcnt.*lgkmcnt\(0\)' "$D/loop.s" || true)  s_barrier $(cnt s_barrier)"
echo "  s_waitcnt vmcnt $(grep -cE '^\s+s_waitcnt.*vmcnt' "$D/loop.s" || true)  s_mov_b32 m0 $(grep -cE '^\s+s_mov_b32 m0,' "$D/loop.s" || true)  LDS-DMA (buffer_load / global_load ... lds) $(grep -cE '^\s+(buffer_load|global_load_lds)_.*\slds(\s|$)|^\s+global_load_lds_' "$D/loop.s" || true)  buffer_load_dwordx4 into registers $(grep -E '^\s+buffer_load_dwordx4\s' "$D/loop.s" | grep -cvE '\slds(\s|$)' || true)  global_load $(grep -cE '^\s+global_load_dword' "$D/loop.s" || true)"
if [ -n "$KEEP" ]; then cp "$D/loop.s" "$KEEP"; echo "loop body kept in $KEEP"; fi
