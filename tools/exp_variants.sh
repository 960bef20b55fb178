#!/bin/bash
# Runs bench.py's main section (64 and 16 iterates per launch) against each experiment build named on the command line
# (lpopc_amd/csrc/librpm_exp_<name>.so) and the default library, interleaved twice, each checked against a single evaluation
# (--full --only-main); the lines go to OUTDIR.  Perf exploration only:  bash tools/exp_variants.sh OUTDIR <name>...
OUT=$(mkdir -p "${1:?usage: exp_variants.sh OUTDIR NAME...}" && cd "$1" && pwd)
shift
for rep in 1 2; do
for v in base "$@"; do
  L=$PWD/lpopc_amd/csrc/librpm_hip.so; [ "$v" != base ] && L=$PWD/lpopc_amd/csrc/librpm_exp_$v.so
  for b in 64 16; do
    RPM_HIP_LIB=$L python bench.py --full --steps 300 --warmup 30 --only-main --batch $b --iterates 256 > ${OUT}/exp_${v}_${b}_${rep}.json 2>${OUT}/exp_${v}_${b}_${rep}.err || exit 1
  done
done
done
python - "$OUT" "$@" <<'PY'
import json, os, sys
for v in ["base"] + sys.argv[2:]:
    for b in (64, 16):
        for rep in (1, 2):
            d = json.loads(open(os.path.join(sys.argv[1], "exp_%s_%d_%d.json" % (v, b, rep))).read().strip().splitlines()[-1])
            print(v, b, rep, "%.0f pairs/s  %.4f ms/step  frac %.3f" % (d["value"], d["ms_per_step"], d["roofline"]["frac"]))
PY
