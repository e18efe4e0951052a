#!/bin/bash
# Variant builds of the general-M synthesis kernel (chan_syn_gen.hip) into $OUT (default
# tools/experiments/abl/, never the product library), for the A/Bs of DESIGN.md 3.4b "general M":
#   thr1024 = the 512-lane / 16384-point tile from M = 1024 only, chan_gen.hip's threshold
#            (shipped: from M = 250)
#   thr512 = from M = 512
#   small  = the 256-lane / 4096-point tile for every M (M = 1536, 3000 on the small tile)
#   allbig = the 512-lane / 16384-point tile for every M
#   nofft  = no transform passes (load, transposition, overlap-add and store only; outputs wrong)
#   noload = constant frames instead of the row loads (outputs wrong)
#   nooa   = one sample per lane and round instead of the overlap-add (outputs wrong)
# Run: python tools/experiments/run_with_lib.py $OUT/libsg_<v>.so bench_configs.py --config synth --chan-nch 1000
# (nofft / noload / nooa: add --no-check); outputs of the tile variants: tools/diag/synth_hash.py
set -e
cd "$(dirname "$0")/../.."
OUT=${OUT:-tools/experiments/abl}
mkdir -p $OUT
make -C unnamed-rust-sdr_amd -s
OBJS=$(ls unnamed-rust-sdr_amd/build/*.o | grep -v chan_syn_gen.o)
for v in ${VARIANTS:-thr1024 thr512 small allbig nofft noload nooa}; do
  src=$OUT/chan_syn_gen_$v.hip
  cp unnamed-rust-sdr_amd/csrc/chan_syn_gen.hip $src
  def=""
  case $v in
    thr1024) def="-DSDRGPU_SYNTH_GEN_BIG_MIN_M=1024" ;;
    thr512) def="-DSDRGPU_SYNTH_GEN_BIG_MIN_M=512" ;;
    small) def="-DSDRGPU_SYNTH_GEN_BIG_MIN_M=4097" ;;
    allbig) def="-DSDRGPU_SYNTH_GEN_BIG_MIN_M=2" ;;
  esac
  python3 - $src $v <<'PY'
import sys
p, v = sys.argv[1], sys.argv[2]; s = open(p).read()
if v == "nofft":
    old = "[[clang::always_inline]] gen_engine<BLK, TILE>(lds, M, F, g.rl, a.tw);"
    assert old in s; s = s.replace(old, "")
elif v == "noload":
    old = "float2 v = synth_frame(a, k, j);"
    assert old in s; s = s.replace(old, "float2 v = make_float2((float)k, (float)j);")
elif v == "nooa":
    old = "                if (ua <= ub) {"
    assert old in s
    s = s.replace(old, "                if (i == 0) acc[0] = lds[lp<TILE>(min(o, FM - 1))];\n                if (false) {")
open(p, 'w').write(s)
PY
  /opt/rocm/bin/hipcc -O3 -std=c++20 -fPIC --offload-arch=gfx950 $def -Iunnamed-rust-sdr_amd/csrc -Iinclude -x hip -c $src -o $OUT/chan_syn_gen_$v.o
  /opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o $OUT/libsg_$v.so $OBJS $OUT/chan_syn_gen_$v.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
done
echo built
