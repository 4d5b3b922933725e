#!/usr/bin/env bash
# Builds libmmeeg_hip.so for gfx950 in-tree (cross-compiles without a GPU).
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
out="$here/../libmmeeg_hip.so"
mkdir -p "$here/build"
objs=()
pids=()
# an object is rebuilt when its source, this script or ANY header is newer (coarse: who includes what is not tracked)
deps=("$0" "$here"/*.h "$here"/*.inc "$here/../../include/mmeeg_hip.h")
for src in "$here"/*.hip; do
  obj="$here/build/$(basename "${src%.hip}").o"
  objs+=("$obj")
  stale=0
  for dep in "$src" "${deps[@]}"; do [[ "$dep" -ot "$obj" ]] || stale=1; done
  if [[ ! -f "$obj" ]] || (( stale )); then
    extra=()
    # attention (attention.hip): MFMA results straight into VGPRs (the softmax is VALU work on every score: no v_accvgpr_read per
    # score).  Per file only: A/B in the training step, profiles/r03_attention_ab.txt (as a global flag it cost 25 %)
    [[ "$(basename "$src")" == attention*.hip ]] && extra=(-mllvm -amdgpu-mfma-vgpr-form=1)
    # xai.hip: its contract is torch's bits of `base + alpha * (x - base)`, every fp32 operation rounded on its own: no FMA contraction
    [[ "$(basename "$src")" == xai.hip ]] && extra=(-ffp-contract=off)
    # -fno-slp-vectorize: no compiler-formed v_pk_{fma,mul,add}_f32.  With them (op_sel-selected register halves, SGPR-pair
    # operands) the BatchNorm-reduce epilogue of the 1-D GEMM (igemm1d.h) gave run-to-run different sums in ~5 % of its workgroups
    # whenever it ran inside the two-stream training graph (never stand-alone); scalar fp32 code is bit-stable and the
    # step is not slower (profiles/r03_packed_fp32_ab.txt).  Hand-written v_pk_* in conv3d_wres's asm is unaffected.
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -fno-slp-vectorize -Wall -Wno-unused-function "${extra[@]}" \
        -I"$here" -I"$here/../../include" -c "$src" -o "$obj" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [[ -n "$p" ]] && wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out" "${objs[@]}"
echo "built $out"
