"""The epilogues of the encoder GEMM and of the decoder linears issue their global loads (bias / LayerNorm-fold
constants / residual) TOGETHER and wait for them once, instead of one `load; s_waitcnt vmcnt(0)` round trip after the
other: with one workgroup per CU (encoder GEMM) nothing else runs on the CU while its waves sit in such a wait.  The
order of loads and waits is visible in the compiled code, so this guard needs no GPU: gemm.hip and dec_kernels.hip
are compiled to assembly with build.sh's flags, and for every instantiation the flagship path (large-v3, float16)
launches the text from the last `s_barrier` / `v_mfma` of the kernel to its end is scanned for LONELY vector loads: a
`global_load_dwordx2` / `global_load_dwordx4` that is followed by an `s_waitcnt vmcnt(..)` before any other
`global_load` and is not itself the last of a run of loads issued back to back (a group of loads ends in one wait: that
is the point).

  * encoder GEMM (row-major, transposed and both layered instantiations) and the LDS-staged decoder linear
    (dec_gemm_big_kernel, workgroup shapes 0 / 1 / 2, plain and LayerNorm-folded): 0;
  * the register-streaming decoder linear (1 x 1 and 2 x 2 tiles) and the vocabulary projection: at most one group wait
    per column-tile group (a wave finishes ONE group of column tiles, so at most 1).

Exempt: the scalar `global_load_ushort` tails of shapes whose strides are not multiples of 8 halves (`vec_ok == false`
in gemm.hip) — no shape of the model takes them, and a 2-byte load cannot be grouped into a vector.  Before the loads
were grouped this scan counted 40 in gemm_f16_kernel<false, false, false> (32 bias + 8 residual), 24 / 12 in the 4- / 2-
column-tile forms of dec_gemm_big_kernel and 8 per group in dec_gemm_wave_kernel."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "faster_whisper_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")

_VEC_LOAD = re.compile(r"^\s*global_load_dwordx[24]\b")
_ANY_LOAD = re.compile(r"^\s*global_load_(?!lds_)")
_VM_WAIT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(")
_TAIL_START = re.compile(r"^\s*(s_barrier|v_mfma_)")


def _build_flags():
    sh = open(os.path.join(CSRC, "build.sh")).read()
    m = re.search(r'^FLAGS="([^"]+)"', sh, re.M)
    assert m, "build.sh no longer defines FLAGS"
    return m.group(1).split()


_ASM = {}


def _kernels(src):
    """{mangled kernel name: its instruction lines} of one source file, compiled as build.sh compiles it"""
    if src not in _ASM:
        p = subprocess.run(["hipcc", *_build_flags(), "-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", "-"],
                           capture_output=True, text=True, cwd=CSRC)
        assert p.returncode == 0, p.stderr[-2000:]
        out, cur = {}, None
        for line in p.stdout.splitlines():
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            if cur is not None:
                cur.append(line)
        _ASM[src] = out
    return _ASM[src]


def lonely_vector_loads(lines):
    """vector loads after the kernel's last barrier / MFMA that are waited for before another load is issued"""
    start = max((k for k, ln in enumerate(lines) if _TAIL_START.match(ln)), default=-1)
    lonely, group, vec = 0, 0, False       # loads issued since the last wait; whether the last one was a vector load
    for ln in lines[start + 1:]:
        if _ANY_LOAD.match(ln):
            group += 1
            vec = bool(_VEC_LOAD.match(ln))
        elif _VM_WAIT.match(ln):
            lonely += group == 1 and vec
            group = 0
    return lonely


def _one(kernels, *parts):
    hit = [n for n in kernels if all(p in n for p in parts)]
    assert len(hit) == 1, (parts, hit)
    return hit[0], kernels[hit[0]]


def test_scanner_counts_what_it_should():
    text = """
        v_mfma_f32_32x32x16_f16 a[0:15], v[0:3], v[4:7], a[0:15]
        global_load_dwordx2 v[0:1], v2, s[0:1]
        s_waitcnt vmcnt(0)
        s_barrier
        global_load_dwordx4 v[0:3], v8, s[0:1]
        s_waitcnt lgkmcnt(0)
        s_waitcnt vmcnt(0) lgkmcnt(0)
        global_load_dwordx4 v[0:3], v8, s[0:1]
        global_load_dwordx4 v[4:7], v9, s[0:1]
        s_waitcnt vmcnt(1)
        s_waitcnt vmcnt(0)
        global_load_ushort v0, v1, s[0:1]
        s_waitcnt vmcnt(0)
        global_load_lds_dwordx4 v1, s[0:1]
        s_waitcnt vmcnt(0)
        global_load_dwordx2 v[0:1], v2, s[0:1]
        global_store_dwordx2 v2, v[0:1], s[0:1]
        s_waitcnt vmcnt(0)
        s_endpgm
    """.splitlines()
    assert lonely_vector_loads(text) == 2


@pytest.mark.parametrize("trans,layered", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_encoder_gemm_epilogue_loads_are_grouped(trans, layered):
    name, lines = _one(_kernels("gemm.hip"), f"gemm_f16_kernelILb{trans}ELb0ELb{layered}E")
    n = lonely_vector_loads(lines)
    print(f"{name}: {n} lonely vector loads")
    assert n == 0, name


# dec_gemm_big_kernel<LNF, S, WM, WN, FB, KC, NST>: its workgroup shapes (dec_kernels.hip: BIG_SHAPES)
@pytest.mark.parametrize("lnf", [0, 1])
@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_dec_linear_big_epilogue_loads_are_grouped(cfg, lnf):
    shape = {0: "Li4ELi2ELi4E", 1: "Li2ELi2ELi2E", 2: "Li2ELi2ELi4E"}[cfg]          # WM, WN, FB
    hits = [n for n in _kernels("dec_kernels.hip") if re.search(rf"dec_gemm_big_kernelILb{lnf}ELi\d+E{shape}", n)]
    assert hits, (cfg, lnf)
    for name in hits:
        n = lonely_vector_loads(_kernels("dec_kernels.hip")[name])
        print(f"{name}: {n} lonely vector loads")
        assert n == 0, name


@pytest.mark.parametrize("lnf", [0, 1])
@pytest.mark.parametrize("tiles", [1, 2])
def test_dec_linear_skinny_epilogue_loads_are_grouped(tiles, lnf):
    hits = [n for n in _kernels("dec_kernels.hip")
            if re.search(rf"dec_gemm_frag_kernelILi\d+ELb{lnf}ELi{tiles}ELi{tiles}ELi\d+E", n)]
    assert hits, (tiles, lnf)
    for name in hits:
        n = lonely_vector_loads(_kernels("dec_kernels.hip")[name])
        print(f"{name}: {n} lonely vector loads")
        assert n <= 1, name


def test_vocabulary_projection_epilogue_loads_are_grouped():
    hits = [n for n in _kernels("dec_kernels.hip") if re.search(r"dec_gemm_wave_kernelILb0E", n)]   # I8 = false
    assert hits
    for name in hits:
        n = lonely_vector_loads(_kernels("dec_kernels.hip")[name])
        print(f"{name}: {n} lonely vector loads")
        assert n <= 1, name
