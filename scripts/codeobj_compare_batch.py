#!/usr/bin/env python3
"""Compare the many-query kernels of two builds of libcerebro_hip.so (no GPU): for every kernel whose name contains one of the given
substrings, the register figures of the code object's notes (.vgpr_count, .agpr_count, .sgpr_count, spill counts, scratch, LDS) and the
instruction listing.  Used to show that a change to batch.hip left the existing db_gemm_topk instantiations as they were
(profiles/query_prefix.md).

    python scripts/codeobj_compare_batch.py NEW.so [OLD.so] [--match db_gemm_topk --match db_gemm_prefixed ...]

Prints one markdown table row per kernel; with OLD.so also whether the listing (mnemonics and operands, addresses dropped) is equal."""
import argparse
import os
import re
import struct
import subprocess
import tempfile
from pathlib import Path

LLVM = Path(os.environ.get("ROCM", "/opt/rocm")) / "lib" / "llvm" / "bin"
KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size"]


def code_objects(so, tmp):
    out = subprocess.run([str(LLVM / "llvm-readelf"), "-S", "-W", str(so)], capture_output=True, text=True, check=True).stdout
    off = size = None
    for line in out.splitlines():
        if ".hip_fatbin" in line:
            f = line.split()
            i = f.index(".hip_fatbin")
            off, size = int(f[i + 3], 16), int(f[i + 4], 16)
    data = Path(so).read_bytes()[off:off + size]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos, paths = 0, []
    while True:
        p = data.find(magic, pos)
        if p < 0:
            break
        (n_entries,) = struct.unpack_from("<Q", data, p + 24)
        q = p + 32
        for _ in range(n_entries):
            o, s, ts = struct.unpack_from("<QQQ", data, q)
            q += 24
            triple = data[q:q + ts].decode()
            q += ts
            if "amdgcn" in triple and s > 0:
                path = Path(tmp) / f"{Path(so).stem}_{len(paths)}.elf"
                path.write_bytes(data[p + o:p + o + s])
                paths.append(path)
        pos = p + 24
    return paths


def kernels_of(so, tmp, wanted):
    """name -> (notes dict, [instruction text])"""
    out = {}
    for co in code_objects(so, tmp):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        meta = {}
        for block in notes.split("- .agpr_count:")[1:]:
            block = ".agpr_count:" + block
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            if any(w in name for w in wanted):
                meta[name] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
        if not meta:
            continue
        dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--mcpu=gfx950", "--no-show-raw-insn", str(co)],
                             capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1) if m.group(1) in meta else None
                if cur:
                    out[cur] = (meta[cur], [])
                continue
            if cur and line.strip() and line.strip() != "..." and not line.startswith("Disassembly"):   # ("...": padding behind a kernel)
                out[cur][1].append(line.split("//")[0].strip())
    return out


def short(name):
    m = re.search(r"(db_gemm_topk|db_gemm_prefixed)ILi32ELi(\d+)ELi(\d+)E([fd])EE", name)
    if m:
        return f"{m.group(1)}<32, {m.group(2)}, {m.group(3)}, {'float' if m.group(4) == 'f' else 'double'}>"
    m = re.search(r"gather_query_tilesI([fd])Li(\d+)EE", name)
    if m:
        return f"gather_query_tiles<{'float' if m.group(1) == 'f' else 'double'}, {m.group(2)}>"
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("new")
    ap.add_argument("old", nargs="?")
    ap.add_argument("--match", action="append")
    a = ap.parse_args()
    wanted = a.match or ["db_gemm_topk", "db_gemm_prefixed", "gather_query_tiles", "transpose_queries"]
    with tempfile.TemporaryDirectory() as tmp:
        new = kernels_of(a.new, tmp, wanted)
        old = kernels_of(a.old, tmp, wanted) if a.old else {}
    print("| kernel | vgpr | agpr | sgpr | vgpr spills | sgpr spills | scratch B | LDS B | instructions | mfma 32x32x2 |" + (" parent: figures | parent: listing |" if a.old else ""))
    print("|---|---|---|---|---|---|---|---|---|---|" + ("---|---|" if a.old else ""))
    bad = 0
    for name in sorted(new, key=short):
        meta, ins = new[name]
        row = [short(name)] + [str(meta[k]) for k in KEYS] + [str(len(ins)), str(sum(t.startswith("v_mfma_f32_32x32x2") for t in ins))]
        if a.old:
            if name in old:
                same_meta, same_ins = old[name][0] == meta, old[name][1] == ins
                bad += not (same_meta and same_ins)
                row += ["equal" if same_meta else "DIFFER", "equal" if same_ins else f"DIFFER ({len(old[name][1])} instructions)"]
            else:
                row += ["-", "-"]
        print("| " + " | ".join(row) + " |")
    for name in sorted(set(old) - set(new)):
        print(f"| {short(name)} | only in the parent build |")
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
