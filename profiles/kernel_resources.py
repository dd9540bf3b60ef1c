"""Register / LDS / occupancy table of every kernel in a .hip file (hipcc -Rpass-analysis=kernel-resource-usage).
usage: python profiles/kernel_resources.py faster_whisper_amd/csrc/dec_kernels.hip [filter] [--asm]
       (the rules, scoring, no-speech and token-probability kernels: faster_whisper_amd/csrc/dec_vocab.hip)
--asm: from a `--cuda-device-only -S` build instead — the code object's metadata per kernel (registers, scalar and vector
       spill counts, LDS, scratch) and the number of instruction lines between the kernel's label and its end."""
import re, subprocess, sys, os, tempfile
args = [a for a in sys.argv[1:] if a != "--asm"]
asm = "--asm" in sys.argv[1:]
src = args[0]
flt = args[1] if len(args) > 1 else ""
extra = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"] if os.path.basename(src) == "attn_enc.hip" else []
base = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *extra]
cwd = os.path.dirname(os.path.abspath(src)) or "."
def dem(n):
    try:
        return subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", n], capture_output=True, text=True).stdout.strip().split("(")[0]
    except Exception:
        return n
if asm:
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([*base, "--cuda-device-only", "-S", os.path.abspath(src), "-o", out], check=True, cwd=cwd,
                       stderr=subprocess.DEVNULL)
        txt = open(out).read()
    lines, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1); lines[cur] = 0
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"^\t[a-z]", line):
            lines[cur] += 1
    for blk in re.split(r"\n  - \.agpr_count", txt)[1:]:
        d = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        n = dem(d["name"]) or d["name"]
        if flt and flt not in n: continue
        print(f"{n:70s} vgpr {d['vgpr_count']:>4} vgpr-spill {d['vgpr_spill_count']:>3} sgpr {d['sgpr_count']:>4} sgpr-spill "
              f"{d['sgpr_spill_count']:>3} lds {d['group_segment_fixed_size']:>6} scratch {d['private_segment_fixed_size']:>3} "
              f"lines {lines.get(d['name'], '?')}")
    sys.exit(0)
p = subprocess.run([*base, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.abspath(src), "-o", "/dev/null"],
                   capture_output=True, text=True, cwd=cwd)
cur = {}
rows = []
for line in p.stderr.splitlines():
    m = re.search(r"remark:\s+Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}; rows.append(cur); continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
    if m and rows:
        cur[m.group(1).strip()] = m.group(2)
for r in rows:
    n = dem(r["name"])
    if flt and flt not in n: continue
    print(f"{n:70s} vgpr {r.get('VGPRs','?'):>4} agpr {r.get('AGPRs','?'):>4} occ {r.get('Occupancy','?'):>2} lds {r.get('LDS Size','?'):>6} scratch {r.get('ScratchSize','?')}")
