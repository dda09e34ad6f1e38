#!/bin/bash
# round-6 evidence in one gpurun call: kernel stats of the bench command (+ the two PMC passes), beam 5 x 128, BUTDSpatial XE, the AoA
# SCST step, AoA beam 5 x 64 -> $OUT (what is judged is copied into profiles/r06_*), then the bench line itself (--full)
export ROUND=r06
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd $ROOT
OUT=${OUT:?OUT=<output directory> bash tools/r6_profiles.sh}
mkdir -p "$OUT"
bash tools/collect_profiles.sh > "$OUT"/collect.log 2>&1
bash tools/prof_any.sh beam5_b128 tools/perf_eval.py 128 > "$OUT"/beam.top 2>&1
bash tools/prof_any.sh xe_spatial49 tools/perf_xe_spatial.py > "$OUT"/xe.top 2>&1
bash tools/prof_aoa_engine.sh > "$OUT"/aoa.top 2>&1
bash tools/prof_any.sh aoa_beam5_b64 tools/perf_aoa_beam.py 64 > "$OUT"/aoa_beam.top 2>&1
timeout -k 10 900 python3 bench.py --full > "$OUT"/bench_line.json 2> "$OUT"/bench.err
ls "$OUT"
tail -c 600 "$OUT"/bench_line.json
# round 5 additions: the SCST step of a model that ends its captions (early-out of the steps behind the reference's break) and of
# an 8-image batch (merged greedy + sampled chain)
ICZ_PERF_BREAK=11 ICZ_PERF_ROUNDS=1 bash tools/prof_any.sh scst_end_biased tools/perf_options.py early_out=1 > "$OUT"/end_biased.top 2>&1
ICZ_PERF_B=8 bash tools/prof_any.sh scst_b8 tools/perf_small_one.py > "$OUT"/b8.top 2>&1
