#!/bin/bash
# A/B timing of library variants (tools/build_variant.sh) in ONE GPU call: for every variant and config a short bench run;
# prints ms/step, the per-kernel HIP-event times and results_sha1 (equal fingerprints = bit-identical results of the step).
#   gpurun --timeout 900 -- 'bash tools/gpu_ab.sh <tag> "base q8" "2 4" [extra bench args]'
# REPEATS=6: every config runs its variants ALTERNATELY that many times (a, b, c, a, b, c, ...), every run a process of its own, and
# a summary per (config, variant) follows the runs: median, min, max and spread (max - min) of us/step.
# A run that ends like a GPU fault or at its time limit (exit 124, 134, 137, 139) ends the call: nothing more is started.  Any other
# non-zero exit of a run is reported on its line, the runs go on, and the script exits with the last such status.
# The line of a run: us/step (profiles older than tile_pairs.txt quote this tool's earlier line: ms/step, and a `prepare` field
# behind `finalize`), the per-kernel HIP-event times in us, results_sha1, the library's source hash; r<k> is the repeat.
set -u
TAG=${1:-ab}; LIBS=${2:-base}; CFGS=${3:-"2 4"}; EXTRA=${4:-}
REPEATS=${REPEATS:-1}
REPO=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$REPO/gpurun_out
mkdir -p $OUT
cd $REPO
RUNS=$OUT/${TAG}_runs.txt
: > $RUNS
WORST=0
for cfg in $CFGS; do
  steps=200; [ "$cfg" == "2" ] && steps=1000
  for r in $(seq 1 $REPEATS); do
  for lib in $LIBS; do
    base=${lib%%@*}; envs=""; [ "$base" != "$lib" ] && envs=$(echo "${lib#*@}" | tr ',' ' ')   # name@VAR=val,VAR2=val2
    so=$REPO/tools/ab/libkt_engine_$base.so
    [ "$base" == "tree" ] && so=$REPO/kube_throttler_amd/csrc/libkt_engine.so
    name=${TAG}_$(echo "$lib" | tr -c 'A-Za-z0-9\n' '_')_cfg${cfg}_r${r}
    env $envs KT_ENGINE_LIB=$so timeout -k 10 400 python bench.py --full --config $cfg --steps $steps --warmup 10 --no-cpu-baseline --no-latency --no-extra $EXTRA > $OUT/$name.json 2> $OUT/$name.err
    rc=$?
    python - "$OUT/$name.json" "$lib" "$cfg" "$rc" "$r" <<'PY' | tee -a $RUNS
import json, sys
f, lib, cfg, rc, r = sys.argv[1:6]
try:
    d = json.loads(open(f).read().strip().splitlines()[-1])
    k = d["roofline"]["per_kernel_ms"]
    print("cfg%s %-32s r%s us/step %8.2f | check %.2f agg %.2f reduce %.2f finalize %.2f | sha1 %s | %s" % (
        cfg, lib, r, d["ms_per_step"] * 1e3, k["check"] * 1e3, k["aggregate"] * 1e3, k["reduce"] * 1e3, k["finalize"] * 1e3,
        d["config"]["results_sha1"], d["config"]["engine_version"].split("src=")[-1]))
except Exception as ex:
    print("cfg%s %-32s r%s exit %s: no bench line (%s)" % (cfg, lib, r, rc, ex))
PY
    [ $rc -ne 0 ] && { WORST=$rc; tail -3 $OUT/$name.err; }
    case $rc in 124|134|137|139) echo "exit $rc: stopping here"; exit $rc;; esac
  done
  done
done
[ "$REPEATS" -gt 1 ] && python - "$RUNS" <<'PY'
import statistics, sys
runs = {}
for line in open(sys.argv[1]):
    w = line.split()
    if "us/step" not in w:
        continue
    cfg, lib, us = w[0], w[1], float(w[w.index("us/step") + 1])
    agg, sha = float(w[w.index("agg") + 1]), w[w.index("sha1") + 1]
    runs.setdefault((cfg, lib), []).append((us, agg, sha))
for (cfg, lib), v in runs.items():
    us = [x[0] for x in v]
    print("  %s  %-32s n=%d  median %7.2f  min %7.2f  max %7.2f  spread %.2f  agg(ev) median %.2f  results_sha1 %s" % (
        cfg, lib, len(v), statistics.median(us), min(us), max(us), max(us) - min(us), statistics.median(x[1] for x in v),
        ",".join(sorted(set(x[2] for x in v)))))
PY
exit $WORST
