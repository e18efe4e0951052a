#!/bin/bash
# Variant builds of the general-M channelizer kernel (chan_gen.hip) into $OUT (default
# tools/experiments/abl/, never the product library), for the A/Bs of DESIGN.md 3.4a "general M":
#   big512 = the 1024-lane / 16384-point tile from M = 512 (M = 1000 on the big tile)
#   small  = the 256-lane / 4096-point tile for every M (M = 1536, 3000 on the small tile)
#   ch4, ch8 = 4 / 8 points of a lane per pass over the tap rows on both tiles (shipped: 8 on
#            the 4096-point tile, 4 on the 16384-point one)
#   nofft  = no transform passes (sums, transposition and store only; outputs wrong)
#   noload = constant samples instead of the stream loads (outputs wrong)
# Run: python tools/experiments/run_with_lib.py $OUT/libcg_<v>.so bench_configs.py --config chan --chan-nch 1000
# (nofft / noload: add --no-check)
set -e
cd "$(dirname "$0")/../.."
OUT=${OUT:-tools/experiments/abl}
mkdir -p $OUT
make -C unnamed-rust-sdr_amd -s
OBJS=$(ls unnamed-rust-sdr_amd/build/*.o | grep -v chan_gen.o)
for v in ${VARIANTS:-big512 small ch4 ch8 nofft noload}; do
  src=$OUT/chan_gen_$v.hip
  cp unnamed-rust-sdr_amd/csrc/chan_gen.hip $src
  def=""
  case $v in
    big512) def="-DSDRGPU_CHAN_GEN_BIG_MIN_M=512" ;;
    small) def="-DSDRGPU_CHAN_GEN_BIG_MIN_M=4097" ;;
    ch4) def="-DSDRGPU_CHAN_GEN_CHUNK=4" ;;
    ch8) def="-DSDRGPU_CHAN_GEN_CHUNK=8" ;;
  esac
  python3 - $src $v <<'PY'
import sys
p, v = sys.argv[1], sys.argv[2]; s = open(p).read()
if v == "nofft":
    old = "gen_engine<BLK, TILE>(lds, M, F, g.rl, a.tw);"
    assert old in s; s = s.replace(old, "")
elif v == "noload":
    old = "if (off[i] >= 0) x[i] = stream_sample<U8>(a, b + off[i]);"
    assert old in s; s = s.replace(old, "if (off[i] >= 0) x[i] = make_float2((float)off[i], (float)q);")
open(p, 'w').write(s)
PY
  /opt/rocm/bin/hipcc -O3 -std=c++20 -fPIC --offload-arch=gfx950 $def -Iunnamed-rust-sdr_amd/csrc -Iinclude -x hip -c $src -o $OUT/chan_gen_$v.o
  /opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o $OUT/libcg_$v.so $OBJS $OUT/chan_gen_$v.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
done
echo built
