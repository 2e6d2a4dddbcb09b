#!/bin/bash
# Runs ON THE GPU BOX: kernel times of gemm_hp on the step's shapes, a variant library (csrc/librnnt_hip_<variant>.so, e.g. the parent
# commit built in a git worktree) against the in-tree build, interleaved, one process per library and round.
# usage: tools/gemm_hp_epilogue_ab.sh <variant> [rounds=3] [outfile=build/gemm_hp_epilogue_ab.txt]
# Per shape the median over the rounds, and the fixed cost of one round of 256 x 256 tiles, (proj - dX) / 6 (tools/gemm_hp_time.py).
set -o pipefail
V=$1; R=${2:-3}
cd "$(dirname "$0")/.."
OUT=${3:-build/gemm_hp_epilogue_ab.txt}
mkdir -p "$(dirname "$OUT")"; : > $OUT
for r in $(seq $R); do
  for w in $V main; do
    if [ $w = main ]; then L=; else L=$PWD/rnntransducer_amd/csrc/librnnt_hip_$w.so; fi
    RNNT_HIP_LIB=$L timeout -k 10 240 python3 tools/gemm_hp_time.py $w --step-shapes 2>&1 | grep -v "amdgpu.ids" >> $OUT || { cat $OUT; exit 1; }
  done
done
python3 - $OUT $V main >> $OUT <<'P'
import statistics, sys
rows = {}
for l in open(sys.argv[1]):
    if l.startswith("#us "):
        w = l.split()
        for kv in w[2:]:
            k, v = kv.split("=")
            rows.setdefault(w[1], {}).setdefault(k, []).append(float(v))
print("medians over the rounds, us")
for lib in sys.argv[2:]:
    med = {k: statistics.median(v) for k, v in rows[lib].items()}
    print(f"{lib:>10} | " + " | ".join(f"{k} {v:.0f} ({min(rows[lib][k]):.0f}..{max(rows[lib][k]):.0f})" for k, v in med.items())
          + f" | fixed cost per round (proj - dX) / 6 = {(med['proj'] - med['dX']) / 6:.1f}")
P
cat $OUT
