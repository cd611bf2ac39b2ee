#!/usr/bin/env python3
"""Static instruction statistics of the kernels in one .hip file (no GPU needed).

    python tools/isa_stats.py runia_core_amd/csrc/mc_sampler.hip [name-filter]
    python tools/isa_stats.py runia_core_amd/csrc/mc_sampler.hip mc_entropy    # K1: the table forms and mc_entropy_lut_kernel
    python tools/isa_stats.py --digest runia_core_amd/csrc/proj_sq.hip         # one line per kernel, for diff

Compiles the file to gfx950 assembly with the Makefile's flags and prints, per kernel: vector / scalar instruction
counts, v_readlane + v_writelane (scalar registers spilled to vector lanes), MFMA count, VGPRs, SGPRs, scratch bytes,
v_mov count and branch count (s_cbranch_* + s_branch).
--digest prints instead, per kernel and sorted by mangled name: a hash of the instruction stream, a hash of the kernel
descriptor (.amdhsa_* lines: registers, LDS, scratch) and the mangled name.  Comments and directives that carry file
positions are dropped and local labels renumbered in order of appearance (a label carries the function's index within the
file), so a refactor that must not change a kernel is checked by diffing the output before and after - also across a file
split or a moved function: `sort` the outputs of the files of each side together.
The hot kernels are sensitive to small source changes (K1 went from 722 to 937 vector instructions when one more
scalar load entered its loop), so this is run before a GPU measurement."""
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FLAGS = (__import__("os").environ.get("ISA_EXTRA", "") + " --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -mllvm -amdgpu-mfma-vgpr-form").split()


def _sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def digest(text):
    """[(mangled name, hash of the normalised instruction stream, hash of the .amdhsa_* block)] of every kernel in `text`."""
    rows = []
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.S | re.M):
        name = m.group(1)
        start = re.search(rf"^{re.escape(name)}:", text, re.M)
        if not start:
            raise SystemExit(f"{name}: kernel descriptor without a code label")
        labels, body = {}, []
        for line in text[start.end():m.start()].split("\n"):
            line = line.split(";")[0].rstrip()
            if not line.strip() or re.match(r"\s*\.(loc|file|cfi_\w+|section|p2align|text)\b", line):
                continue
            body.append(re.sub(r"\.L[\w$.]+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line))
        hsa = [l.split(";")[0].strip() for l in m.group(2).split("\n") if l.strip()]
        rows.append((name, _sha(body), _sha(hsa)))
    return sorted(rows)


def main():
    args = [a for a in sys.argv[1:] if a != "--digest"]
    src = Path(args[0]).resolve()
    flt = args[1] if len(args) > 1 else ""
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "k.s"
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-S", "--cuda-device-only", f"-I{ROOT}/include", str(src), "-o", str(out)],
                       check=True, stderr=subprocess.DEVNULL)
        text = out.read_text()
    if "--digest" in sys.argv:
        for name, body, hsa in digest(text):
            if flt in name:
                print(body, hsa, name)
        return
    meta = {}
    kernels = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    for block in re.split(r"\n  - \.", kernels)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", block)
        if not nm:
            continue
        def g(k, block=block):
            r = re.search(rf"{k}:\s+(\d+)", block)
            return int(r.group(1)) if r else 0
        meta[nm.group(1)] = (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"))
    rows = []
    for name, (vg, sg, scratch, lds) in meta.items():
        m = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)
        if not m:
            continue
        body = m.group(1)
        ins = re.findall(r"^\s+([vs]_[a-z0-9_]+)", body, re.M)
        valu = sum(1 for i in ins if i.startswith("v_") and "mfma" not in i)
        mfma = sum(1 for i in ins if "mfma" in i)
        salu = sum(1 for i in ins if i.startswith("s_"))
        lanes = sum(1 for i in ins if i.startswith(("v_readlane", "v_writelane")))
        vmov = sum(1 for i in ins if i.startswith("v_mov"))
        br = sum(1 for i in ins if i.startswith(("s_cbranch", "s_branch")))
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        short = short.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if flt and flt not in short:
            continue
        rows.append((short, valu, salu, lanes, mfma, vg, sg, scratch, lds, vmov, br))
    print(f"{'kernel':64s} {'valu':>5s} {'salu':>5s} {'lane':>5s} {'mfma':>5s} {'vgpr':>5s} {'sgpr':>5s} {'scr':>5s} {'lds':>6s} {'vmov':>5s} {'br':>4s}")
    for r in rows:
        print(f"{r[0][:64]:64s} " + " ".join(f"{v:5d}" for v in r[1:8]) + f" {r[8]:6d} {r[9]:5d} {r[10]:4d}")


if __name__ == "__main__":
    main()
