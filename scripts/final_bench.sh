#!/bin/bash
export GRAFT_REPO_ROOT="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"   # the repo root when not run through gpurun
# The round's committed bench line: bash scripts/final_bench.sh <tag> <output dir>   (on the GPU box; the line is
# <output dir>/bench_<tag>.json, committed as profiles/<tag>_bench.json)
cd "$GRAFT_REPO_ROOT"
tag=${1:?usage: final_bench.sh <tag> <output dir>}
out=${2:?usage: final_bench.sh <tag> <output dir>}
mkdir -p "$out"
python bench.py --full > "$out/bench_$tag.json" 2> "$out/bench_$tag.err"
tail -1 "$out/bench_$tag.err"
python - "$out/bench_$tag.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d["value"], d["ms_per_step"], {k: d["roofline"][k] for k in ("frac", "frac_model_8d", "frac_traffic", "traffic", "l2_hit_rate")})
e = d["extra"]
for k, v in e["optical_flow_small_batches"].items():
    if isinstance(v, dict):
        print(k, {a: round(b, 1) for a, b in v.items()})
print({k: (round(v["frames_per_s"]) if isinstance(v, dict) and "frames_per_s" in v else "") for k, v in e.items()})
PY
