"""Per-kernel table of the awry_hip device code: registers, LDS, scratch, code size and a hash of the disassembly.

    python tools/device_code_table.py [--src awry_amd/csrc/awry_hip.hip] [--keep DIR] [--fold-library] > table.txt

Compiles the source with the compile line of awry_amd/build.py plus --offload-device-only (gfx950, no GPU needed),
reads the kernels' metadata with llvm-readobj --notes and disassembles with llvm-objdump -d.  The hash is over a
kernel's instructions with addresses, encodings, branch-target offsets, pc-relative distances and the padding behind the
kernel stripped, so that two builds can be compared
with diff: a refactor of the host side must leave every row as it was.  --keep DIR also writes the stripped
disassembly of every kernel to DIR/<symbol>.s.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
FLAGS = ["--offload-arch=gfx950", "-march=x86-64-v3", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "--offload-device-only"]
FIELDS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".group_segment_fixed_size": "lds",
          ".private_segment_fixed_size": "scratch"}


def kernel_metadata(co):
    """-> {symbol: {field: int}} from the AMDGPU metadata note: one map per kernel under amdhsa.kernels, keys at one indentation"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readobj"), "--notes", co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^  ([- ]) (\.[a-z_]+):\s*(\S*)\s*$", line)
        if not m:
            continue
        first, key, val = m.groups()
        if first == "-":
            cur = {}
        if cur is None:
            continue
        if key in FIELDS:
            cur[FIELDS[key]] = int(val)
        elif key == ".symbol":
            sym = val.strip("'\"")
            out[sym[:-3] if sym.endswith(".kd") else sym] = cur
    return out


def kernel_disassembly(co):
    """-> {symbol: [instruction text, ...]} with addresses, encodings and label offsets stripped"""
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    out, cur, pcrel = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:\s*$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        ins = re.sub(r"//.*$", "", line)               # the address comment
        ins = re.sub(r"^\s*[0-9a-f]+:\s*", "", ins)     # a leading address, where objdump prints one
        ins = re.sub(r"<([^>+]+)\+0x[0-9a-f]+>", r"<\1>", ins)
        ins = ins.strip()
        # s_getpc_b64, then s_add_u32 / s_addc_u32 with the distance to a constant table: an address like any other
        if pcrel and re.match(r"s_addc?_u32 .*, 0x[0-9a-f]+$", ins):
            ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)
        pcrel = 2 if ins.startswith("s_getpc_b64") else max(0, pcrel - 1)
        cur.append(ins)
    # what follows a kernel's last instruction up to the next symbol is alignment padding: it depends on the section the
    # kernel is emitted into (a template instantiation has one of its own), not on the kernel
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."):
            body.pop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "awry_amd", "csrc", "awry_hip.hip"))
    ap.add_argument("--keep", default=None)
    ap.add_argument("--fold-library", action="store_true", help="one row for all kernels outside namespace awry (rocprim's): their number "
                    "and a hash over their rows, so that a committed table stays small and still shows whether any of them changed")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "awry_hip.co")
        subprocess.check_call([os.path.join(ROCM, "bin", "hipcc")] + FLAGS + ["-c", args.src, "-o", co + ".bundle"])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + co + ".bundle",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        meta, dis = kernel_metadata(co), kernel_disassembly(co)
    if args.keep:
        os.makedirs(args.keep, exist_ok=True)
    print("%-5s %-5s %-5s %-7s %-7s %-8s %-16s %s" % ("vgpr", "agpr", "sgpr", "lds", "scratch", "insns", "sha256[:16]", "kernel"))
    rows, folded = [], []
    for sym in sorted(meta):
        body = dis.get(sym, [])
        if args.keep:
            with open(os.path.join(args.keep, (sym if len(sym) < 200 else hashlib.sha256(sym.encode()).hexdigest()) + ".s"), "w") as f:
                f.write("\n".join(body) + "\n")
        m = meta[sym]
        row = "%-5d %-5d %-5d %-7d %-7d %-8d %-16s %s" % (m.get("vgpr", -1), m.get("agpr", -1), m.get("sgpr", -1), m.get("lds", -1),
                                                          m.get("scratch", -1), len(body), hashlib.sha256("\n".join(body).encode()).hexdigest()[:16],
                                                          sym if len(sym) < 200 else sym[:150] + "...#" + hashlib.sha256(sym.encode()).hexdigest()[:12])
        (folded if args.fold_library and not sym.startswith("_ZN4awry") else rows).append(row)
    print("\n".join(rows))
    if folded:
        print("%d kernels outside namespace awry, sha256 over their rows of the unfolded table: %s" % (len(folded), hashlib.sha256("\n".join(folded).encode()).hexdigest()))
    missing = sorted(set(meta) - set(dis))
    if missing:
        sys.exit("no disassembly for: " + ", ".join(missing))


if __name__ == "__main__":
    main()
