#!/usr/bin/env python3
"""Compare the gfx950 device code of two libqba.so builds, object by object.

    tools/codeobj_diff.py OLD/libqba.so NEW/libqba.so

Code objects are paired by position (link order) when both builds have the
same number, else by their first kernel symbol, so that a source file added
to or taken out of the build shows as one `added` / `removed` object and the
others are still compared.  For every pair the sections .text (the code),
.rodata (the kernel descriptors) and .note (the kernel metadata) must be
byte-identical and the sets of kernel symbols (*.kd) equal.  Symbol-name
tables are not compared: each object's __hip_cuid_* name hashes its source.
Prints one line per object; exit status 1 on any difference between paired
objects or on a removed one (an added object alone is not a difference in
the kernels the old build had).  Under an object that differs or was added,
one line per kernel gives the descriptor's VGPRs, SGPRs, static LDS and
scratch of both builds.  No GPU needed.
"""
import hashlib
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
from kd_util import _descriptors, _sections, code_objects  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")


def summary(elf: bytes):
    secs = {s["name"]: elf[s["off"]:s["off"] + s["size"]] for s in _sections(elf) if s["name"] in SECTIONS}
    return secs, _descriptors(elf)


def _line(i, secs, kernels, verdict):
    first = min(kernels, default="(no kernels)")
    text = secs.get(".text", b"")
    return (f"object {i:2d}: {len(kernels):3d} kernels, .text {len(text):8d} B "
            f"sha256 {hashlib.sha256(text).hexdigest()[:12]}  {verdict}  [{first[:40]}]")


def _kernels(old: dict, new: dict):
    """Per kernel of a changed object: the descriptor fields in the old and the new build."""
    fmt = lambda d: "-" if d is None else "vgpr {vgprs:3d} sgpr {sgprs:3d} lds {lds:6d} scratch {scratch}".format(**d)  # noqa: E731
    for k in sorted(set(old) | set(new)):
        print(f"    {k}\n      old: {fmt(old.get(k))}\n      new: {fmt(new.get(k))}")


def main(old: str, new: str) -> int:
    a, b = [summary(x) for x in code_objects(old)], [summary(y) for y in code_objects(new)]
    if len(a) == len(b):
        pairs = list(zip(a, b))
    else:
        by_first = {min(k, default=""): (s, k) for s, k in a}
        pairs = [(by_first.pop(min(k, default=""), None), (s, k)) for s, k in b]
        pairs += [(x, None) for x in by_first.values()]
    bad = False
    for i, (x, y) in enumerate(pairs):
        if x is None:
            print(_line(i, *y, "added"))
            _kernels({}, y[1])
            continue
        if y is None:
            print(_line(i, *x, "REMOVED"))
            bad = True
            continue
        (sx, kx), (sy, ky) = x, y
        diff = [n for n in SECTIONS if sx.get(n) != sy.get(n)]
        if set(kx) != set(ky):
            diff.append(f"kernels -{len(set(kx) - set(ky))} +{len(set(ky) - set(kx))}")
        bad |= bool(diff)
        print(_line(i, sy, ky, "DIFFERENT: " + ", ".join(diff) if diff else "equal"))
        if diff:
            _kernels(kx, ky)
    added = sum(1 for x, _ in pairs if x is None)
    print("DIFFERENT" if bad else
          f"all {len(a)} code objects of the old build equal (.text, .rodata, .note, kernel names)"
          + (f"; {added} added" if added else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
