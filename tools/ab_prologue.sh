# A/B of the decoder-fold placement (S2S_PROLOGUE, model_step.cpp model_step_impl) on one GPU:
#   tools/ab_prologue.sh [OUTDIR]  ->  OUTDIR/ab_<mode>.json (default: ab_out/)
set -e
out=${1:-ab_out}
mkdir -p "$out"
for m in 0 1 2; do
  S2S_PROLOGUE=$m timeout -k 10 200 python bench.py --full --no-cpu --no-pmc --steps 40 > "$out/ab_$m.json" 2>/dev/null
done
