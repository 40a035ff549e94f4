#!/bin/bash
# round 6, session a: the pruned build (ABI 8) -- per-stage error of raw ViT-G against the oracle as the number of split blocks grows (the non-monotone
# parity of VERDICT r5 weak 2), the self-calibration table, then the GPU suite and a short bench
cd "$GRAFT_REPO_ROOT" 2>/dev/null || true
export O=${SESSION_OUT:-session_out}/r6a
mkdir -p "$O"
export HSA_ENABLE_IPC_MODE_LEGACY=0
KS=0,8,12,16,40 F8=none timeout 900 python tools/stage_errors.py raw_vitg_224 > $O/stage_errors_vitg_fp16terms.txt 2>&1
tail -12 $O/stage_errors_vitg_fp16terms.txt
KS=0,8,12,16,40 timeout 900 python tools/stage_errors.py raw_vitg_224 raw_vitg_224_w1 > $O/stage_errors_vitg_policy.txt 2>&1
tail -8 $O/stage_errors_vitg_policy.txt
timeout 900 python tools/calibration_table.py > $O/calibration_table.txt 2>&1
cat $O/calibration_table.txt | tail -45
timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider -x --durations=15 > $O/gpu_suite.txt 2>&1
tail -40 $O/gpu_suite.txt
timeout 600 python bench.py --full --no-cpu-baseline --no-traffic > $O/bench.json 2> $O/bench.err
tail -c 1500 $O/bench.json
