# Same-box A/B of the headline: _ab/old (a worktree of an earlier commit, built in place; OLD_DIR=.
# for this tree) vs this tree, alternating rounds, with OLD_ENV / NEW_ENV (VAR=value ...) set for
# each side; one JSON summary line per run in $OUT/ab.log (OUT: default bench_out).  Each side runs
# `bench.py --full` without the extras and the CPU baseline: the headline + its layer times.
set -o pipefail
OUT=$(realpath -m "${OUT:-bench_out}")
mkdir -p "$OUT"
: > "$OUT/ab.log"
for r in ${ROUNDS:-1 2 3}; do
  for t in old new; do
    d=$([ $t = old ] && echo "${OLD_DIR:-_ab/old}" || echo .)
    e=$([ $t = old ] && echo "${OLD_ENV:-}" || echo "${NEW_ENV:-}")
    full=$(grep -q -e '"--full"' $d/bench.py && echo --full)   # a tree from before the option times its layers anyway
    (cd $d && env $e timeout -k 10 300 python -u bench.py --steps ${STEPS:-8} --warmup 2 $full --no-extras --no-cpu-baseline) > "$OUT/ab_$t.json" 2> "$OUT/ab_err.log" || exit $?
    python - $t "$OUT" >> "$OUT/ab.log" <<'PY'
import json, sys
t, out = sys.argv[1:3]
s = open(f"{out}/ab_{t}.json").read()
d = json.loads(s[s.index('{"metric'):].split("\n")[0])
print(json.dumps({"tree": t, "value": round(d["value"], 1), "ms": round(d["ms_per_step"], 2),
                  "layers": {k: round(v, 2) for k, v in d["layer_ms_per_step"].items() if "delta" not in k}}))
PY
  done
done
