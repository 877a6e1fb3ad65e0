#!/bin/bash
# full check of the tree on the GPU box: GPU tests, `bench.py --full` -> <out>/<tag>_*   usage: tools/full_check.sh <tag> [out, default check_out]
cd ${GRAFT_REPO_ROOT:-.}
tag=${1:-check}
out=${2:-check_out}
mkdir -p $out
timeout 1500 python -m pytest tests -x -q -m gpu 2>&1 | grep -E "passed|failed|error" | tail -3 > $out/${tag}_gputests.txt
cat $out/${tag}_gputests.txt
timeout 1200 python bench.py --full > $out/${tag}_bench_full.json 2> $out/${tag}_bench_full.err
python - <<PY
import json
for l in open("$out/${tag}_bench_full.json"):
    l=l.strip()
    if l.startswith("{"):
        d=json.loads(l); p=d["phases"]; o=d["one_batch_in_flight"]
        print("headline %.2f images/s, %.1f ms/step, ids equal %s; solo %.2f images/s enc %.2f ms (%.4f) step %.4f ms roofline %.4f" % (d["value"], d["ms_per_step"], d["config"].get("ids_equal_one_batch_calls"), o["images_per_s"], o["phases"]["encoder_ms"], o["phases"]["enc_mfma_frac"], o["phases"]["decode_step_ms"], o["roofline"]["frac"]))
        print("   whole_job", p["whole_job"])
        for k,v in d["extra_runs"].items():
            print("  ", k, v.get("images_per_s", v.get("pages_per_s")), v.get("ids_equal_batch_calls", ""))
PY
