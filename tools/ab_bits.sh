#!/bin/bash
# Bits of the tracks, the excitation and the PCM of fixed batches (tests/tools/ab_bits.py) under two prebuilt libraries:
#   tools/ab_bits.sh tools/_ab_base/libjbonsai_amd.so [other.so]      (second default: the product library)
#   BITS_ARGS=--host tools/ab_bits.sh ...   the host halves of the spectral stages alone (no device); --seams: the
#   entries on caller-held PCM alone
cd "$(dirname "$0")/.."
cp jbonsai_amd/libjbonsai_amd.so /tmp/_keep_bits.so
trap 'cp /tmp/_keep_bits.so jbonsai_amd/libjbonsai_amd.so' EXIT
A=$1; B=${2:-/tmp/_keep_bits.so}
# (each run under a time limit of its own; a run that fails ends the comparison: nothing more is started on the device)
run() { timeout -k 10 ${BITS_TIMEOUT:-900} python tests/tools/ab_bits.py $BITS_ARGS > "$2" 2>&1 || { echo "== $1: the run failed ($?)"; tail -20 "$2"; exit 1; }; }
cp "$A" jbonsai_amd/libjbonsai_amd.so; run "$A" /tmp/_bits_a.txt
cp "$B" jbonsai_amd/libjbonsai_amd.so; run "$B" /tmp/_bits_b.txt
echo "== $A"; cat /tmp/_bits_a.txt; echo "== $B"; cat /tmp/_bits_b.txt
if diff -q /tmp/_bits_a.txt /tmp/_bits_b.txt > /dev/null; then echo "BITS IDENTICAL"; else echo "BITS DIFFER"; diff /tmp/_bits_a.txt /tmp/_bits_b.txt; fi
