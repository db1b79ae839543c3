#!/usr/bin/env python3
"""Are the gfx950 kernels of two sets of sources the same?  For a refactor that moves kernels between files.

    python tools/isa_diff.py --old OLD.s [...] --new avlmaps_amd/csrc/a.hip avlmaps_amd/csrc/b.hip [...]

A .hip argument is compiled to device assembly with build.py's flags for that file name (what tools/kernel_regs.py does), a .s
argument is read as it is (the old side: `hipcc <flags> -S --cuda-device-only` on the parent commit's file).  Per kernel, over
the union of each side: the code-object metadata (registers, LDS, scratch, spills, workgroup size, arguments) and the
instruction stream, comments / debug directives dropped and local labels renumbered, must be equal.  Prints one line per kernel
and a verdict; exit status 1 if anything differs, is missing, is new or is defined in more files than before."""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def assembly(arg: str) -> str:
    if arg.endswith(".s"):
        return Path(arg).read_text()
    from avlmaps_amd import build as b
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "k.s"
        cmd = [b._hipcc(), *b.COMMON, *b.SOURCES[Path(arg).name], "-S", "--cuda-device-only", "-o", str(out), arg]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        return out.read_text()


def kernels(text: str) -> dict:
    """mangled name -> (metadata block, normalised code from the kernel's label to the end of its function)"""
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        meta[re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)] = m.group(0)
    out = {}
    for name, md in meta.items():
        body = re.search(r"^" + re.escape(name) + r":.*?^\.Lfunc_end\d+:", text, re.S | re.M).group(0)
        lines = []
        for ln in body.splitlines()[:-1]:
            ln = ln.split(";")[0].rstrip()
            if not ln or re.match(r"\s*\.(loc|file|cfi_\w+)\b", ln):
                continue
            lines.append(re.sub(r"\.L([A-Za-z]+)\d+_(\d+)", r".L\1_\2", ln))     # .LBB<function number>_<block>
        out[name] = (md, "\n".join(lines))
    return out


def side(args) -> dict:
    """mangled name -> [(metadata, code, file), ...]: one entry per file that defines the kernel"""
    merged = {}
    for a in args:
        for name, k in kernels(assembly(a)).items():
            merged.setdefault(name, []).append(k + (Path(a).name,))
    return merged


def main() -> int:
    argv = sys.argv[1:]
    i, j = argv.index("--old"), argv.index("--new")
    old = side(argv[i + 1:j] if i < j else argv[i + 1:])
    new = side(argv[j + 1:] if i < j else argv[j + 1:i])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in new or name not in old:
            verdict = "LOST" if name not in new else "NEW"
        elif any(o[0] != n[0] for o in old[name] for n in new[name]):
            verdict = "metadata differs"
        elif any(o[1] != n[1] for o in old[name] for n in new[name]):
            verdict = "code differs"
        else:
            verdict = "equal"
        if name in old and name in new and len(new[name]) != len(old[name]):
            verdict += f", in {len(new[name])} files"
        bad += verdict != "equal"
        k = (new.get(name) or old[name])
        print(f"{verdict:24s} {'+'.join(x[2] for x in k):32s} {k[0][1].count(chr(10)) + 1:6d}  {name}")
    print(f"\n{len(old)} kernels before, {len(new)} after: " + ("all equal" if not bad else f"{bad} NOT equal"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
