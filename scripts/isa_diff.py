#!/usr/bin/env python3
"""Same machine code, kernel by kernel (docs/KERNELS.md, "Refactoring a kernel
file"): compare the gfx950 assembly of a kernel file before and after a change.

    isa_diff.py OLD.s NEW.s                      two assembly listings
    isa_diff.py --trees OLD_ROOT NEW_ROOT UNIT.. csrc/kernels/UNIT.hip of two source
                                                 trees, compiled with the flags of
                                                 _build.py plus --cuda-device-only -S

Per `.amdhsa_kernel` symbol the text from the symbol's label to its
`.Lfunc_end` (the `.amdhsa_kernel` block lies inside), without comments and
with `.LBB<n>_<k>` rewritten to `.LBB_<k>`, and the kernel's record in the
`amdhsa.kernels` metadata. Prints same / different / only-in-one per mangled
name; exit status 1 on any difference. Text is compared, never interpreted.
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from pathlib import Path


def kernels(asm: str) -> dict:
    """mangled name -> (normalised code text, metadata record) of every kernel."""
    lines = asm.split("\n")
    records = {}
    if "amdhsa.kernels:" in lines:
        rec = None
        for line in lines[lines.index("amdhsa.kernels:") + 1:]:
            if line.startswith("  - "):
                rec = []
            elif rec is None or not line.startswith("    "):
                break
            rec.append(line)
            m = re.match(r"\s+\.name:\s+(\S+)", line)
            if m:
                records[m.group(1)] = rec
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        start = next((i for i, l in enumerate(lines) if l.startswith(name + ":")), None)
        if start is None:
            continue
        body = []
        for line in lines[start:]:
            if line.startswith(".Lfunc_end"):
                break
            line = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*", "", line)).rstrip()
            if line:
                body.append(line)
        out[name] = ("\n".join(body), "\n".join(records.get(name, [])))
    return out


def compare(old: str, new: str, label: str = "", out=sys.stdout) -> int:
    """Print one line per kernel of either listing; the number that differ."""
    a, b = kernels(old), kernels(new)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "only in new" if name in b else "only in old"
        elif a[name] == b[name]:
            verdict = "same"
        else:
            what = [w for w, x, y in zip(("code", "metadata"), a[name], b[name]) if x != y]
            verdict = "different (" + ", ".join(what) + ")"
        bad += verdict != "same"
        print(f"{label}{verdict:<28} {name}", file=out)
    print(f"{label}{len(a)} kernels old, {len(b)} new, {bad} not the same", file=out)
    return bad


def assemble(root: Path, unit: str, out: Path) -> str:
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from tensorflow_distributed_on_gke_amd import _build  # this tree's flags, for both sides

    csrc = root / "csrc"
    cmd = [f"{_build.rocm_path()}/bin/hipcc", *_build.hip_flags(csrc).split(), "--cuda-device-only", "-S",
           str(csrc / "kernels" / f"{unit}.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True)
    return out.read_text()


def main(argv) -> int:
    if len(argv) == 2:
        return 1 if compare(Path(argv[0]).read_text(), Path(argv[1]).read_text()) else 0
    if len(argv) < 4 or argv[0] != "--trees":
        print(__doc__, file=sys.stderr)
        return 2
    old, new, units = Path(argv[1]).resolve(), Path(argv[2]).resolve(), argv[3:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units:
            texts = [assemble(root, unit, Path(tmp) / f"{unit}_{side}.s")
                     for side, root in (("old", old), ("new", new))]
            bad += compare(*texts, label=f"{unit}.hip  ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
