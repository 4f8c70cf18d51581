#!/bin/bash
# The host half of the stems of a mix under AddressSanitizer + UBSan on the CPU: tools/stems_sanitize_main.cpp,
# jbonsai_amd/csrc/jb_mix.cpp and jbonsai_amd/csrc/jb_output.cpp compiled together, host pass sanitized, into a program
# of its own and run.  No GPU is touched and nothing is loaded into python.
set -euo pipefail
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p tools/_ab_stems
$HIPCC --offload-arch=gfx950 -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off \
  -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-gpu-sanitize \
  -x hip tools/stems_sanitize_main.cpp jbonsai_amd/csrc/jb_mix.cpp jbonsai_amd/csrc/jb_output.cpp -fsanitize=address,undefined -o tools/_ab_stems/stems_sanitize
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 tools/_ab_stems/stems_sanitize
