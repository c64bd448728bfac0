#!/usr/bin/env python3
"""Compare the gfx950 device code of two libqba.so builds, object by object.

    tools/codeobj_diff.py OLD/libqba.so NEW/libqba.so

For every gfx950 code object (in link order) the sections .text (the code),
.rodata (the kernel descriptors) and .note (the kernel metadata) must be
byte-identical and the sets of kernel symbols (*.kd) equal.  Symbol-name
tables are not compared: each object's __hip_cuid_* name hashes its source.
Prints one line per object; exit status 1 on any difference.  No GPU needed.
"""
import hashlib
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from kd_util import _descriptors, _sections, code_objects  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")


def summary(elf: bytes):
    secs = {s["name"]: elf[s["off"]:s["off"] + s["size"]] for s in _sections(elf) if s["name"] in SECTIONS}
    return secs, frozenset(_descriptors(elf))


def main(old: str, new: str) -> int:
    a, b = list(code_objects(old)), list(code_objects(new))
    bad = len(a) != len(b)
    if bad:
        print(f"DIFFERENT: {len(a)} code objects against {len(b)}")
    for i, (x, y) in enumerate(zip(a, b)):
        (sx, kx), (sy, ky) = summary(x), summary(y)
        diff = [n for n in SECTIONS if sx.get(n) != sy.get(n)]
        if kx != ky:
            diff.append(f"kernels -{len(kx - ky)} +{len(ky - kx)}")
        bad |= bool(diff)
        first = min(ky, default="(no kernels)")
        print(f"object {i:2d}: {len(ky):3d} kernels, .text {len(sy.get('.text', b'')):8d} B "
              f"sha256 {hashlib.sha256(sy.get('.text', b'')).hexdigest()[:12]}  "
              f"{'DIFFERENT: ' + ', '.join(diff) if diff else 'equal'}  [{first[:40]}]")
    print("DIFFERENT" if bad else f"all {len(b)} code objects equal (.text, .rodata, .note, kernel names)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
