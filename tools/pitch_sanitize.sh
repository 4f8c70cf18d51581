#!/bin/bash
# The host half of the pitch stage under AddressSanitizer + UBSan on the CPU: tools/pitch_sanitize_main.cpp and
# jbonsai_amd/csrc/jb_pitch.cpp compiled together, host pass sanitized, into a program of its own and run.  No GPU is
# touched and nothing is loaded into python.
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p tools/_ab_pitch
$HIPCC --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
  -x hip tools/pitch_sanitize_main.cpp jbonsai_amd/csrc/jb_pitch.cpp -Xarch_host -fsanitize=address,undefined -o tools/_ab_pitch/pitch_sanitize
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 tools/_ab_pitch/pitch_sanitize
