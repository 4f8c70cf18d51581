#!/bin/bash
# The host half of the jb_*_pcm_batch entries (jbonsai_amd/csrc/jb_pcm_call.h) under AddressSanitizer + UBSan on the
# CPU: tests/plan/pcm_call_probe.cpp, a program of its own, compiled with g++ and run on the cases of
# tests/test_pcm_call_plan.py (the hand-out with every allocation failing in turn).  No GPU is touched and nothing is
# loaded into python.
set -euo pipefail
cd "$(dirname "$0")/.."
mkdir -p tools/_ab_pcm_call
exe=tools/_ab_pcm_call/pcm_call_sanitize
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -Wall -Wextra -Werror -pedantic -fsanitize=address,undefined \
  -fno-sanitize-recover=undefined -I jbonsai_amd/csrc tests/plan/pcm_call_probe.cpp -o $exe
export ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1
for words in "check 0 0 -1" "check 2147483648 1 -1 1 1 1 1 1 1 1 1" "check 3 1 1 4 1 4" "check 3 1 1 4 0 4" \
             "pack 4 0 1 1025 0" "pack 0" "hand 3 0 2 1 2 3 0 4 3" "hand 3 1 2 1 2 3 0 4 3" "hand 3 2 2 1 2 3 0 4 3" \
             "hand 3 3 2 1 2 3 0 4 3"; do
  echo "$words" | $exe
done
echo "pcm_call_sanitize: clean"
