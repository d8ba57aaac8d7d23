#!/bin/bash
# The screened ranking with 80 % of the items masked (the cold-item split), the compaction of the fp16 pass on and off in the same
# build, twice each, alternated.  From the repo root on the GPU box: bash tools/screen_cold_ab.sh [masked share]
# Every step has its own time limit and the chain stops at the first failure.
M=${1:-0.8}
cd "$(dirname "$0")/.." || exit 1
CRH_SCORE_SCREEN_COMPACT=1 timeout -k 10 150 python3 tools/screen_cold_ab.py --masked "$M" &&
CRH_SCORE_SCREEN_COMPACT=0 timeout -k 10 150 python3 tools/screen_cold_ab.py --masked "$M" &&
CRH_SCORE_SCREEN_COMPACT=1 timeout -k 10 150 python3 tools/screen_cold_ab.py --masked "$M" &&
CRH_SCORE_SCREEN_COMPACT=0 timeout -k 10 150 python3 tools/screen_cold_ab.py --masked "$M"
