"""Per-kernel comparison of the gfx950 code objects of two builds of libprio3gpu.so (no GPU):
every kernel's bytes in .text, its kernel descriptor and its metadata entry in .note, whichever
of a library's code objects (one per HIP translation unit) defines it.
usage: tools/code_object_compare.py PARENT.so BRANCH.so WORKDIR > report"""
import difflib
import hashlib
import os
import re
import subprocess
import sys
from pathlib import Path

LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def sh(*a):
    return subprocess.run([str(x) for x in a], check=True, capture_output=True, text=True).stdout


def code_objects(lib, work, tag):
    work.mkdir(parents=True, exist_ok=True)
    fat = work / f"{tag}.fatbin"
    sh(LLVM / "llvm-objcopy", "--only-section=.hip_fatbin", "-O", "binary", lib, fat)
    # objcopy -O binary of one section = the section's bytes
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(data)
        b = work / f"{tag}.bundle{k}"
        b.write_bytes(data[s:e])
        co = work / f"{tag}.{k}.co"
        sh(LLVM / "clang-offload-bundler", "--unbundle", "--type=o",
           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={b}", f"--output={co}")
        out.append(co)
    return out


def sections(co):
    secs = {}
    for l in sh(LLVM / "llvm-readelf", "-S", "-W", co).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", l)
        if m:
            secs[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16),
                                     int(m.group(5), 16))
    return secs


def kernels(co):
    """name -> dict(text=bytes, kd=bytes, meta=str) for every kernel of the code object."""
    raw = co.read_bytes()
    secs = sections(co)
    syms = {}
    for l in sh(LLVM / "llvm-readelf", "-s", "-W", co).splitlines():
        p = l.split()
        if len(p) == 8 and p[3] in ("FUNC", "OBJECT") and p[6].isdigit():
            syms[p[7]] = (int(p[1], 16), int(p[2]), int(p[6]))
    notes = sh(LLVM / "llvm-readelf", "--notes", co)
    metas = {}
    body = notes.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0]
    for ent in re.split(r"\n  - ", "\n" + body.strip("\n")):
        m = re.search(r"\.name:\s+(\S+)", ent)
        if m:
            metas[m.group(1)] = ent.strip()

    def bytes_of(name):
        addr, size, shndx = syms[name]
        _, saddr, soff, _ = secs[shndx]
        return raw[soff + addr - saddr: soff + addr - saddr + size]

    out = {}
    for name, meta in metas.items():
        out[name] = dict(text=bytes_of(name), kd=bytes_of(name + ".kd"), meta=meta, co=co.name)
    return out


def disasm(co, name):
    txt = sh(LLVM / "llvm-objdump", "-d", "--no-show-raw-insn", f"--disassemble-symbols={name}", co)
    lines = [re.sub(r"^\s*", "", re.sub(r"\s*//.*$", "", l)) for l in txt.splitlines()
             if l.startswith("\t") or l.startswith("  ")]
    # objdump prints "..." for the zero padding after an object's last kernel: no instruction
    return [l for l in lines if l != "..."]


def main():
    parent, branch, work = Path(sys.argv[1]), Path(sys.argv[2]), Path(sys.argv[3])
    pco = code_objects(parent, work, "parent")
    bco = code_objects(branch, work, "branch")
    print(f"parent: {len(pco)} gfx950 code object(s); branch: {len(bco)}")
    P = {}
    for co in pco:
        P.update(kernels(co))
    B, dup = {}, []
    for co in bco:
        for k, v in kernels(co).items():
            if k in B:
                dup.append(k)
            B[k] = v
    for co in pco + bco:
        secs = {n: sz for n, _, _, sz in sections(co).values()}
        print(f"  {co.name}: .text {secs['.text']:,} bytes, {len(kernels(co))} kernels")
    print(f"kernels: parent {len(P)}, branch {len(B)}; only in parent {sorted(set(P) - set(B))}; "
          f"only in branch {sorted(set(B) - set(P))}; defined in both branch objects {dup}")
    same = diff_text = diff_meta = diff_kd = 0
    differing = []
    per_co = {}
    for k in sorted(P):
        if k not in B:
            continue
        p, b = P[k], B[k]
        per_co[b["co"]] = per_co.get(b["co"], 0) + 1
        if p["meta"] != b["meta"]:
            diff_meta += 1
            d = [l for l in difflib.unified_diff(p["meta"].splitlines(), b["meta"].splitlines(),
                                                 "parent", "branch", lineterm="", n=0)]
            print(f"METADATA DIFFERS: {k}\n   " + "\n   ".join(d))
        # bytes 16..23 of a descriptor: the code's offset from the descriptor (layout, not content)
        if p["kd"][:16] + p["kd"][24:] != b["kd"][:16] + b["kd"][24:]:
            diff_kd += 1
        if p["text"] == b["text"]:
            same += 1
        else:
            diff_text += 1
            differing.append(k)
    print(f"branch kernels per object: {per_co}")
    print(f".text bytes identical: {same}; differing: {diff_text}; .note metadata entries "
          f"differing: {diff_meta}; kernel descriptors (.kd, 64 bytes, without the code-entry "
          f"offset) differing: {diff_kd}")
    sha = hashlib.sha256()
    for k in sorted(P):
        if k in B and P[k]["text"] == B[k]["text"]:
            sha.update(k.encode() + P[k]["text"])
    print(f"sha256 over (name, bytes) of the identical kernels: {sha.hexdigest()}")
    total_other = 0
    for k in differing:
        p, b = P[k], B[k]
        print(f"\n== {k}: parent {len(p['text'])} bytes, branch {len(b['text'])} bytes")
        dp = disasm(work / p["co"], k)
        db = disasm(work / b["co"], k)
        if len(dp) != len(db):
            print(f"   instruction count differs: {len(dp)} vs {len(db)}")
            total_other += 1
            continue
        n = other = 0
        lit = re.compile(r"^(s_add_u32 \S+, \S+, )0x[0-9a-f]+$")
        for i, (x, y) in enumerate(zip(dp, db)):
            if x != y:
                n += 1
                mx, my = lit.match(x), lit.match(y)
                getpc = any(l.startswith("s_getpc_b64") for l in dp[max(0, i - 3):i])
                if not (mx and my and mx.group(1) == my.group(1) and getpc):
                    other += 1
                    print(f"   OTHER insn {i}: parent `{x}`  branch `{y}`")
                elif n <= 3:
                    print(f"   insn {i}: parent `{x}`  branch `{y}`")
        print(f"   {n} of {len(dp)} instructions differ; {n - other} of them are the literal of an "
              f"`s_add_u32 REG, REG, <literal>` after an s_getpc_b64 (the pc-relative address of a "
              f"constant table); other: {other}")
        total_other += other
    print(f"\ninstructions that differ in anything but such a literal, all kernels: {total_other}")


main()
