#!/bin/bash
# Builds libfwamd.so for gfx950 (MI355X). hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
OUT=../libfwamd.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable"
mkdir -p build
pids=()
for f in logmel gemm rowops attn_enc engine decoder dec_kernels dec_vocab dec_trunc dec_boost dec_boost_trie dec_boost_graph dec_constrain dec_automaton dec_ngram vad resample hooks; do
  if [ ! -f build/$f.o ] || [ $f.hip -nt build/$f.o ] || [ common.h -nt build/$f.o ] || [ kernels.h -nt build/$f.o ] || [ engine.h -nt build/$f.o ] || [ dec_kernels.h -nt build/$f.o ] || [ ../../include/fwamd.h -nt build/$f.o ] || [ ../../include/fwamd_test.h -nt build/$f.o ] || [ vad_model.h -nt build/$f.o ] || [ build.sh -nt build/$f.o ] || { [ $f = dec_trunc ] && [ dec_vocab.hip -nt build/$f.o ]; }; then
    # attn_enc: MFMA accumulators in VGPRs (-amdgpu-mfma-vgpr-form): the softmax reads every score and rescales the output
    # accumulators, which with AGPR accumulators costs 191 v_accvgpr moves per 64-key tile of a vector-bound kernel (548 ->
    # 405 vector instructions per tile, 164 -> 138 registers)
    EXTRA=""
    if [ $f = attn_enc ]; then EXTRA="-mllvm -amdgpu-mfma-vgpr-form=1"; fi
    # dec_automaton is built with the packed-fp32 target feature off: the condition this one unit was tested and timed
    # under.  It is NOT a rule for other units and NOT the cure of anything seen — the unit does no fp32 arithmetic and
    # holds no v_pk_* instruction with or without the switch, and nothing was ever seen to go wrong.  The switch does move
    # the optimiser (16 VGPRs / 42 SGPRs with it, 28 / 62 without; the mask-init loop is not vectorised), so whoever
    # drops it re-runs tests/test_gpu_automaton*.py and profiles/automaton_*.py on the plain build (profiles/NOTES.md).
    if [ $f = dec_automaton ]; then EXTRA="-Xclang -target-feature -Xclang -packed-fp32-ops"; fi
    # dec_ngram likewise, and here the switch does something: the dense pass adds to four floats at a time, and with it
    # off those are four v_fma_f32 / v_add_f32 and no v_pk_* — the unit's tests and timings are of this build.
    if [ $f = dec_ngram ]; then EXTRA="-Xclang -target-feature -Xclang -packed-fp32-ops"; fi
    hipcc $FLAGS $EXTRA -c $f.hip -o build/$f.o &
    pids+=($!)
  fi
done
# host-only C++ (Silero VAD network): g++, with AVX2 / AVX-512 clones selected at run time (target_clones)
if [ ! -f build/vad_host.o ] || [ vad_host.cpp -nt build/vad_host.o ] || [ ../../include/fwamd.h -nt build/vad_host.o ] || [ vad_model.h -nt build/vad_host.o ]; then
  g++ -O3 -std=c++17 -fPIC -Wall -c vad_host.cpp -o build/vad_host.o &
  pids+=($!)
fi
# host-only C++: the native FLAC decoder of the audio front (row f-4)
if [ ! -f build/flac_host.o ] || [ flac_host.cpp -nt build/flac_host.o ] || [ ../../include/fwamd.h -nt build/flac_host.o ]; then
  g++ -O2 -std=c++17 -fPIC -Wall -c flac_host.cpp -o build/flac_host.o &
  pids+=($!)
fi
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -pthread build/*.o -o $OUT
echo "built $(realpath $OUT)"
