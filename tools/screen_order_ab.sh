#!/bin/bash
# The screened ranking over item rows with lognormal norms, the descending-norm order of the fp16 pass on and off in the same
# build, twice each, alternated.  From the repo root on the GPU box: bash tools/screen_order_ab.sh [sigma]
# Every step has its own time limit and the chain stops at the first failure.
S=${1:-0.3}
cd "$(dirname "$0")/.." || exit 1
CRH_SCORE_SCREEN_ORDER=1 timeout -k 10 150 python3 tools/screen_order_ab.py --norm-sigma "$S" &&
CRH_SCORE_SCREEN_ORDER=0 timeout -k 10 150 python3 tools/screen_order_ab.py --norm-sigma "$S" &&
CRH_SCORE_SCREEN_ORDER=1 timeout -k 10 150 python3 tools/screen_order_ab.py --norm-sigma "$S" &&
CRH_SCORE_SCREEN_ORDER=0 timeout -k 10 150 python3 tools/screen_order_ab.py --norm-sigma "$S"
