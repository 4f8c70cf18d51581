#!/bin/bash
# Builds libjbonsai_amd.so for gfx950 (cross-compiles without a GPU).
# -ffp-contract=off: MLPG/LF0 must keep the reference's rounding; the vocoder
# writes its fused multiply-adds explicitly.
# Stale objects are compiled side by side (a from-scratch build: 80 s one after the other, ~25 s this way).
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libjbonsai_amd.so
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result -Wno-unused-value"
mkdir -p build
objs=()
pids=()
names=()
for f in jb_mlpg.hip jb_gv_gang.hip jb_vocoder.hip jb_mglsa.hip jb_postfilter.hip jb_resample.hip jb_loudness.hip jb_loudness.cpp jb_flac.hip jb_flac.cpp jb_format.hip jb_format.cpp jb_adpcm.hip jb_adpcm.cpp jb_fbank.hip jb_fbank.cpp jb_mfcc.hip jb_mfcc.cpp jb_melspec.hip jb_melspec.cpp jb_join.hip jb_join.cpp jb_mix.hip jb_mix.cpp jb_activity.hip jb_activity.cpp jb_pitch.hip jb_pitch.cpp jb_filter.hip jb_filter.cpp jb_fir.hip jb_fir.cpp jb_noise.hip jb_noise.cpp jb_room.hip jb_room.cpp jb_limiter.hip jb_limiter.cpp jb_treesearch.hip jb_treesearch.cpp jb_plan.cpp jb_output.cpp jb_output_chain.cpp jb_batch.cpp jb_voice.cpp jb_engine.cpp jb_multi.cpp; do
  [ -f "$f" ] || continue
  o=build/${f%.*}.o
  # (a .cpp beside a .hip of the same name -- jb_treesearch, jb_loudness, jb_flac, jb_format, jb_adpcm, jb_fbank, jb_mfcc, jb_melspec, jb_join, jb_mix, jb_activity, jb_pitch, jb_filter, jb_fir, jb_noise, jb_room, jb_limiter -- is the host half: an object of its own)
  if [ "${f##*.}" = cpp ] && [ -f "${f%.*}.hip" ]; then o=build/${f%.*}_host.o; fi
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ jb_device.h -nt "$o" ] || [ jb_host.h -nt "$o" ] || [ jb_plan.h -nt "$o" ] || [ jb_output.h -nt "$o" ] || [ jb_pcm_call.h -nt "$o" ] || [ jb_treesearch.h -nt "$o" ] || [ jb_format.h -nt "$o" ] || [ jb_adpcm.h -nt "$o" ] || [ jb_rfft.h -nt "$o" ] || [ jb_rfft_dev.h -nt "$o" ] || [ jb_melbank.h -nt "$o" ] || [ jb_fbank.h -nt "$o" ] || [ jb_mfcc.h -nt "$o" ] || [ jb_melspec.h -nt "$o" ] || [ jb_join.h -nt "$o" ] || [ jb_mix.h -nt "$o" ] || [ jb_activity.h -nt "$o" ] || [ jb_pitch.h -nt "$o" ] || [ jb_filter.h -nt "$o" ] || [ jb_fir.h -nt "$o" ] || [ jb_noise.h -nt "$o" ] || [ jb_room.h -nt "$o" ] || [ jb_limiter.h -nt "$o" ] || [ jb_md5.h -nt "$o" ] || [ jb_loudness_rules.h -nt "$o" ] \
     || [ ../../include/jbonsai_amd.h -nt "$o" ] || { [ -f jb_voice.h ] && [ jb_voice.h -nt "$o" ]; }; then
    echo "hipcc $f"
    # (into a temporary name: an interrupted or failed compile must not leave a fresh-looking object behind)
    ( $HIPCC $FLAGS -x hip -c "$f" -o "$o.tmp" && mv "$o.tmp" "$o" ) &
    pids+=($!)
    names+=("$f")
  fi
  objs+=("$o")
done
fail=0
for i in "${!pids[@]}"; do
  if ! wait "${pids[$i]}"; then
    echo "hipcc failed: ${names[$i]}" >&2
    fail=1
  fi
done
[ $fail -eq 0 ] || exit 1
$HIPCC --offload-arch=gfx950 -shared -fPIC -pthread -o $OUT "${objs[@]}"
echo "built $(realpath $OUT)"
