#!/bin/bash
# usage: tools/rj_chunks.sh [SIZE] — number of z-chunks of the fused projection head (WL_RJ_CHUNKS), ms per step of the head (both solves)
OUT=${OUT:-bench_out}; mkdir -p "$OUT"      # the bench lines and their stderr
SIZE=${1:-512}
run() { python bench.py --full --phases --steps 8 --warmup 3 --size $SIZE --no-cpu-baseline > $OUT/cg.json 2> $OUT/cg.err; python - <<PY
import json
j=json.loads(open("$OUT/cg.json").read().strip().splitlines()[-1]); p=j["phases_ms_per_step"]
print("$SIZE", "$1", "step", round(j["ms_per_step"],3), "head", round(p.get("residual",0),3))
PY
}
run model
for c in 5 8 11 14 17 18 24; do WL_RJ_CHUNKS=$c run ch$c; done
run model
