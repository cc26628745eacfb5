# usage: ab.sh "<ENV for B>"  — runs default (A) and variant (B), train + infer
set -e
V="$1"
d=$(mktemp -d)
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $d/ab_A_train.json 2>$d/ab.err
env $V python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $d/ab_B_train.json 2>$d/ab.err
python bench.py --full --mode infer --steps 20 --warmup 5 --no-cpu-baseline > $d/ab_A_infer.json 2>$d/ab.err
env $V python bench.py --full --mode infer --steps 20 --warmup 5 --no-cpu-baseline > $d/ab_B_infer.json 2>$d/ab.err
python - "$d" <<PY
import json, sys
for m in ("train","infer"):
    for n in ("A","B"):
        j=json.loads(open("%s/ab_%s_%s.json"%(sys.argv[1],n,m)).read().strip().splitlines()[-1])
        e=j["roofline"].get("encoder_stack_forward") or {}
        print(m, n, round(j["ms_per_step"],4), e.get("frac_vs_f32_mfma_peak"), [round(l["us"],1) for l in e.get("per_layer",[])])
PY
rm -rf "$d"
