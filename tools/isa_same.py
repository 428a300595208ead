#!/usr/bin/env python3
"""Are two builds' kernels the same machine code?

    python tools/isa_same.py A B [--only REGEX] [--common]

A and B are each a device assembly (hipcc --cuda-device-only -S), a
disassembly (llvm-objdump -d of a gfx950 code object), or a built library /
code object, which is unbundled and disassembled here (tools/kernel_meta.py).
Per kernel the instruction text is compared with what moves without a change
of the code masked out: comments, addresses and encodings, the __hip_cuid_*
symbol, local label numbers (renumbered in order of appearance), and of a
library or code object the assembler's padding past the end of a kernel's
symbol.  Kernels
that are not identical get their opcode-count differences listed, first as
printed and then with the encoding suffix (_e32, _e64, _dpp, _sdwa) folded,
and a line-by-line pass says whether they differ in literal operands alone
(a pc-relative literal of a disassembly moves with the layout).  Every
kernel's metadata (VGPR, AGPR, SGPR, both spill counts, private and LDS
bytes) is compared where the input carries it.  Exit status 0 when every
kernel common to both is identical in text and metadata and none is missing
(--common: kernels in one build only are listed but do not fail it).
The comparison is generic: no instruction is looked for by name."""
from __future__ import annotations

import collections
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import kernel_meta  # noqa: E402

META = {".vgpr_count": "VGPR", ".agpr_count": "AGPR", ".sgpr_count": "SGPR", ".vgpr_spill_count": "VGPR spill",
        ".sgpr_spill_count": "SGPR spill", ".private_segment_fixed_size": "private B",
        ".group_segment_fixed_size": "LDS B"}


def parse_meta(text: str) -> dict[str, dict]:
    """name -> metadata of the amdhsa.kernels list (YAML as the assembler and
    llvm-readelf --notes print it): an item starts at the list's indent."""
    out, cur, indent = {}, None, None
    for line in text.splitlines():
        m = re.match(r"(\s*)amdhsa\.kernels:", line)
        if m:
            indent = len(m.group(1)) + 2
            continue
        if indent is None:
            continue
        m = re.match(r"(\s*)(- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            if line.strip() and len(line) - len(line.lstrip()) < indent:
                indent = None
            continue
        if m.group(2) and len(m.group(1)) == indent:
            cur = {}
        if cur is None or len(m.group(1)) + (2 if m.group(2) else 0) != indent + 2:
            continue
        k, v = m.group(3), m.group(4).strip()
        if k == ".name":
            out[v.strip("'\"")] = cur
        elif k in META:
            cur[META[k]] = int(v)
    return out


def norm_labels(lines: list[str]) -> list[str]:
    """Local labels (.LBB12_34, .Ltmp5, ...) renumbered by first appearance."""
    seen: dict[str, str] = {}

    def sub(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    return [re.sub(r"\.L[A-Za-z_]*[0-9_]+", sub, ln) for ln in lines]


def kernels_of_asm(text: str) -> dict[str, list[str]]:
    funcs = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = out.setdefault(m.group(1), []) if m.group(1) in funcs else None
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
            continue
        if cur is None:
            continue
        ln = line.split(";", 1)[0].strip()
        if not ln or (ln.startswith(".") and not ln.startswith(".L")):
            continue
        cur.append(re.sub(r"\s+", " ", ln))
    return {k: norm_labels(v) for k, v in out.items() if v}


def kernels_of_dis(text: str, sizes: dict[str, int] | None = None) -> dict[str, list[str]]:
    """sizes: bytes of each kernel's symbol (kernel_meta.code_sizes).  Where given, a kernel ends
    where its symbol does: what the assembler pads with after it (alignment of the next kernel, and
    after the last function of a unit's .text the longer fill that guards instruction prefetch) is
    no code of the kernel's, and which kernel a unit ends with changes when kernels change units."""
    out, cur, end = {}, None, None
    for line in text.splitlines():
        m = re.match(r"([0-9a-f]+) <([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(2), [])
            end = int(m.group(1), 16) + sizes[m.group(2)] if sizes and m.group(2) in sizes else None
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ln, _, enc = line.partition("//")
        a = re.match(r"\s*([0-9A-Fa-f]+):", enc)
        if end is not None and a and int(a.group(1), 16) >= end:
            continue
        ln = ln.strip()
        if ln and ln != "...":      # ("...": zero padding the disassembler elides, after a unit's last kernel)
            cur.append(re.sub(r"\s+", " ", ln))
    return {k: v for k, v in out.items() if v}


def load(path: Path):
    """(kernel -> instruction lines, kernel -> metadata or {})"""
    head = path.read_bytes()[:4]
    if head == b"\x7fELF":
        ks, meta = {}, {}
        with tempfile.TemporaryDirectory() as t:
            cos = [path]
            secs = subprocess.run([str(kernel_meta.LLVM / "llvm-readelf"), "-S", "-W", str(path)],
                                  capture_output=True, text=True, check=True).stdout
            if ".hip_fatbin" in secs:       # a library: every device unit's code object
                cos = kernel_meta.code_objects(path, Path(t))
            for co in cos:
                dis = subprocess.run([str(kernel_meta.LLVM / "llvm-objdump"), "-d", str(co)], capture_output=True,
                                     text=True, check=True).stdout
                notes = subprocess.run([str(kernel_meta.LLVM / "llvm-readelf"), "--notes", str(co)],
                                       capture_output=True, text=True, check=True).stdout
                ks.update(kernels_of_dis(dis, kernel_meta.code_sizes(co)))
                meta.update(parse_meta(notes))
        return ks, meta
    text = path.read_text(errors="replace")
    if re.search(r"^[0-9a-f]+ <[^>]+>:", text, re.M):
        return kernels_of_dis(text), parse_meta(text)
    ks = kernels_of_asm(re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text))
    return ks, parse_meta(text)


def opcodes(lines: list[str], fold: bool) -> collections.Counter:
    c = collections.Counter()
    for ln in lines:
        if ln.endswith(":"):
            continue
        op = ln.split(" ", 1)[0]
        c[re.sub(r"_(e32|e64|dpp|sdwa)\b", "", op) if fold else op] += 1
    return c


# (a symbol's pc-relative reference in an assembly is the address literal of a disassembly)
LIT = re.compile(r"(?<![\w.])(0x[0-9a-fA-F]+|-?\d+|[\w$.]+@rel32@(?:lo|hi))(?![\w.])")


def literal_only(a: list[str], b: list[str]) -> list[tuple[int, str, str]] | None:
    """The differing lines when a and b differ in literal operands alone."""
    if len(a) != len(b):
        return None
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        if x == y:
            continue
        if x.split(" ", 1)[0] != y.split(" ", 1)[0] or LIT.sub("#", x.split(" ", 1)[-1]) != LIT.sub("#", y.split(" ", 1)[-1]):
            return None
        out.append((i, x, y))
    return out


def demangle(names: list[str]) -> dict[str, str]:
    return dict(zip(names, kernel_meta.demangle(names)))


def main() -> int:
    args = sys.argv[1:]
    only = None
    if "--only" in args:
        i = args.index("--only")
        only = re.compile(args[i + 1])
        del args[i:i + 2]
    pos = [a for a in args if not a.startswith("--")]
    if len(pos) != 2:
        print(__doc__)
        return 2
    (ka, ma), (kb, mb) = load(Path(pos[0])), load(Path(pos[1]))
    names = sorted(set(ka) | set(kb))
    dm = demangle(names)
    if only is not None:
        names = [n for n in names if only.search(dm[n]) or only.search(n)]
    print(f"A = {pos[0]}\nB = {pos[1]}\n{len(names)} kernels")
    same = diff = 0
    for n in names:
        short = dm[n].replace("h9k::", "").replace("(KArgs, ", "(")
        if n not in ka or n not in kb:
            print(f"ONLY IN {'A' if n in ka else 'B'}  {short}")
            diff += 1
            continue
        a, b = ka[n], kb[n]
        meta = [(k, ma[n].get(k), mb[n].get(k)) for k in META.values()] if n in ma and n in mb else None
        meta_diff = [f"{k} {x} -> {y}" for k, x, y in (meta or []) if x != y]
        mtxt = "metadata " + ("n/a" if meta is None else "equal" if not meta_diff else "; ".join(meta_diff))
        if a == b:
            print(f"identical  {len(a):6d} lines  {mtxt}  {short}")
            same += not meta_diff
            diff += bool(meta_diff)
            continue
        diff += 1
        lo = literal_only(a, b)
        print(f"DIFFERENT  {len(a):6d} -> {len(b):6d} lines  {mtxt}  {short}")
        if lo is not None:
            print(f"    the same but for literal operands in {len(lo)} lines:")
            for i, x, y in lo[:20]:
                print(f"      {i}: {x}  |  {y}")
        for fold in (False, True):
            ca, cb = opcodes(a, fold), opcodes(b, fold)
            d = {k: cb[k] - ca[k] for k in set(ca) | set(cb) if ca[k] != cb[k]}
            print(f"    opcode counts{' (encodings folded)' if fold else ''}: " +
                  (", ".join(f"{k} {ca[k]} -> {cb[k]}" for k in sorted(d)) or "equal"))
    print(f"{same} identical, {diff} not")
    if "--common" in sys.argv:      # a build that adds kernels: those of both must be the same
        missing = sum(1 for n in names if n not in ka or n not in kb)
        return 0 if diff == missing else 1
    return 0 if diff == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
