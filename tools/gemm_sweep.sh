#!/bin/bash
# GEMM sweep over the decoder shapes of the 7B step (M = 12792 token rows): correctness tests, then TF/s per layout/shape.
# The dispatcher chooses kernels by eligibility alone.  Timing ablations (NT: VLR_GEMM_ABLATE 1 no DMA, 4 no barriers, 8 no epilogue;
# VLR_GEMM_FLAGS for the 128x128 kernel) exist only in the diagnostics build: python vl-rlhf_amd/build_hip.py --ablation, then
# VLR_LIB=vl-rlhf_amd/libvlr_hip_ablation.so VLR_GEMM_ABLATE=1 bash tools/gemm_sweep.sh (the correctness tests fail there by design).
cd "$(dirname "$0")/.."
python -m pytest tests/test_hip_kernels.py -m gpu -x -q -k "gemm" 2>&1 | tail -2
for args in "0 8192 8192 8192" "0 12792 12288 4096" "0 12792 22016 4096" "0 12792 4096 11008" "1 12792 4096 12288" "1 12792 11008 4096" "1 12792 4096 22016" "2 12288 4096 12792" "2 4096 11008 12792" "2 22016 4096 12792"; do
  python tools/gemm_time.py $args 2>&1 | tail -1
done
