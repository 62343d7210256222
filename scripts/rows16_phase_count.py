"""Static instruction counts of the 16-lane Vecchia row kernel's loop body, by phase.

    python scripts/rows16_phase_count.py [CSRC_DIR] [-DNAME=VALUE ...] [--kernel=MANGLED_PREFIX]

Copies vecchia_rows16.hip from CSRC_DIR (default: gpboost_amd/csrc) to a temporary directory with an
assembler comment inserted at each phase boundary (an empty volatile asm: it orders against the other
volatile asm statements and memory operations, plain arithmetic may still drift a few instructions
across it), compiles it for gfx950 with build.py's flags and counts, for
vecchia_rows16_kernel<matern05, DIM = 2>, the instructions of one trip of the problem-set loop
between the markers. --kernel names another instantiation by the head of its mangled name, e.g.
--kernel=vecchia_rows16d_kernelILi0E for the stored-distance form. Prints a markdown table.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
defs = [a for a in args if a.startswith("-D")]
kern = [a.split("=", 1)[1] for a in args if a.startswith("--kernel=")]
dirs = [a for a in args if not a.startswith("-")]
csrc = os.path.abspath(dirs[0]) if dirs else os.path.join(ROOT, "gpboost_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

# (phase name, the source line the marker goes in front of)
MARKS = [("gather", "// ---- gather (rows h and h + 16)"),
         ("covariances", "// ---- 1. circulant pairs"),
         ("row load", "// ---- 2. rows h and h + 16 into registers"),
         ("elimination", "// Gauss-Jordan, 30 pivots"),
         ("traces, sums, partials", "{   // the stashed c, y_nbr back")]

src = open(os.path.join(csrc, "vecchia_rows16.hip")).read().split("\n")
out, k = [], 0
for line in src:
    if k < len(MARKS) and line.strip().startswith(MARKS[k][1]):
        out.append(f'    asm volatile("; ROWS16_PHASE {k}" ::: "memory");')
        k += 1
    out.append(line)
assert k == len(MARKS), f"marker {MARKS[k][1]!r} not found"

with tempfile.TemporaryDirectory() as tmp:
    hip = os.path.join(tmp, "vecchia_rows16.hip")
    open(hip, "w").write("\n".join(out))
    asm = os.path.join(tmp, "k.s")
    cmd = [os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
           "--offload-arch=gfx950", "-fopenmp", f"-I{os.path.join(ROOT, 'include')}", f"-I{csrc}",
           f"-I{ROCM}/include", "-x", "hip", "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage"] + defs + [hip, "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    text = open(asm).read()
    remarks = r.stderr

name = kern[0] if kern else "vecchia_rows16_kernelILi0ELi2E"
body = text[text.index(f"{name}EEvNS_15VecchiaRowsArgsE:"):]
body = body[:body.index("s_endpgm")]
lines = body.split("\n")
first = next(i for i, l in enumerate(lines) if "ROWS16_PHASE 0" in l)
end = max(i for i, l in enumerate(lines) if re.match(r"\s*s_cbranch", l) or re.match(r"\s*s_branch", l))
# the loop body: from the first marker to the last backward branch, plus the loop head before the marker
head = max(i for i, l in enumerate(lines[:first]) if re.match(r"\.LBB\d+_\d+:", l))
phase = "gather"
counts = collections.OrderedDict((n, collections.Counter()) for n, _ in MARKS)
for l in lines[head:end + 1]:
    m = re.search(r"ROWS16_PHASE (\d)", l)
    if m:
        phase = MARKS[int(m.group(1))][0]
        continue
    t = l.split(";")[0].strip()
    if not t or t.endswith(":") or t.startswith("."):
        continue
    counts[phase][t.split()[0]] += 1


def cls(mn):
    if mn.startswith("v_") and not mn.startswith(("v_readlane", "v_readfirstlane")):
        return "VALU"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(("global_", "scratch_", "buffer_", "flat_")):
        return "VMEM"
    return "scalar"


def fp64(mn):
    return "_f64" in mn


m = re.search(rf"Function Name: \S*{name}.*?VGPRs: (\d+)", remarks, re.S)
print(f"VGPRs: {m.group(1) if m else '?'}")
m = re.search(rf"Function Name: \S*{name}.*?ScratchSize \[bytes/lane\]: (\d+)", remarks, re.S)
print(f"scratch bytes/lane: {m.group(1) if m else '?'}\n")
print("| phase | VALU | fp64 VALU | v_fmac_f64_dpp | v_mov_b64 | LDS | VMEM | scalar | notable |")
print("|---|---|---|---|---|---|---|---|---|")
tot = collections.Counter()
for n, c in counts.items():
    by = collections.Counter()
    for mn, q in c.items():
        by[cls(mn)] += q
        if cls(mn) == "VALU" and fp64(mn):
            by["f64"] += q
    top = ", ".join(f"{q} {mn}" for mn, q in c.most_common(6))
    row = [by["VALU"], by["f64"], c["v_fmac_f64_dpp"], c["v_mov_b64"] + c["v_mov_b64_e32"], by["LDS"], by["VMEM"],
           by["scalar"]]
    for i, x in enumerate(row):
        tot[i] += x
    print(f"| {n} | " + " | ".join(str(x) for x in row) + f" | {top} |")
print("| **loop body** | " + " | ".join(f"**{tot[i]}**" for i in range(7)) + " | |")
