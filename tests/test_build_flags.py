"""VERDICT round 5, weak point 12: `build.sh` compiles attn_enc.hip with `-mllvm -amdgpu-mfma-vgpr-form=1` (MFMA accumulators in
VGPRs: the softmax reads every score and rescales the output accumulators — with AGPR accumulators that is 191 `v_accvgpr`
moves per 64-key tile of a vector-bound kernel, 548 vs 405 vector instructions, profiles/r04_attn_bench*.txt).  A compiler
bump that drops or renames the option would silently cost 4-5 % of the encoder attention.  This test compiles the file the way
build.sh does and checks what the flag buys: no AGPRs in `attn_enc_kernel` and a register count that still lets three waves per
SIMD in; and that every kernel of the decoder file stays out of scratch memory (a wave-uniform branch around array elements
once put the LayerNorm sums of dec_gemm_big_kernel there: profiles/NOTES.md, round 6); and that the kernels which hold a
vocabulary row in registers (dec_vocab.hip) still do."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faster_whisper_amd", "csrc")


def _resources(src, extra):
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *extra,
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_attention_accumulators_stay_in_vgprs():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    m = re.search(r'if \[ \$f = attn_enc \]; then EXTRA="([^"]+)"', sh)
    assert m, "build.sh no longer sets the extra flags of attn_enc.hip"
    extra = m.group(1).split()
    assert "-amdgpu-mfma-vgpr-form=1" in extra
    res = _resources("attn_enc.hip", extra)
    k = [v for n, v in res.items() if "attn_enc_kernel" in n]
    assert k, list(res)
    for v in k:
        assert int(v["AGPRs"]) == 0, v                      # the flag took effect: accumulators are VGPRs
        assert int(v["VGPRs"]) <= 168, v                    # three waves per SIMD (168 = the allocation step below 176)
        assert int(v["ScratchSize"]) == 0, v
    # without the flag the same file does use AGPRs: if this ever stops being true the flag (and this test) can go
    plain = [v for n, v in _resources("attn_enc.hip", []).items() if "attn_enc_kernel" in n]
    assert any(int(v["AGPRs"]) > 0 for v in plain), plain


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_decoder_kernels_use_no_scratch_memory():
    res = _resources("dec_kernels.hip", [])
    assert len(res) > 40
    # (the register-capped instantiations of the cross-attention kernel spill BY CONSTRUCTION: fw_test_knob 7, a measurement
    #  variant that the product never launches — include/fwamd_test.h)
    capped = ("dec_cross_attn_kernelILi8ELb1ELi5E", "dec_cross_attn_kernelILi8ELb1ELi6E")
    spilled = {n: v for n, v in res.items() if int(v.get("ScratchSize", 0)) != 0 and not any(c in n for c in capped)}
    assert not spilled, spilled


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_vocabulary_row_kernels_keep_the_row_in_registers():
    """dec_vocab.hip: the rules kernel and the scoring kernel hold 56 values of the row per thread, and a workgroup is 1 024
    threads: past 128 registers it cannot be launched, and a value in scratch memory is a round trip per use.  Both call
    the same device functions for the row, so one edit there moves all ten instantiations."""
    res = _resources("dec_vocab.hip", [])
    assert len(res) == 12 and not {n: v for n, v in res.items() if int(v.get("ScratchSize", 0)) != 0}, res
    k = {n: v for n, v in res.items() if "dec_logits_process_kernel" in n or "dec_score_kernel" in n}
    assert len(k) == 10, list(res)        # <SMP, TXI, ALT>: 2 x 2 x 2, and <RULES>: 2
    for n, v in k.items():
        assert int(v["ScratchSize"]) == 0, (n, v)
        assert int(v["VGPRs"]) <= 128, (n, v)
