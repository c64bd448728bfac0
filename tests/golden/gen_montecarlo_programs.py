#!/usr/bin/env python3
"""Fixture for tests/montecarlo_programs.py: the compiled programs of its
circuit pairs, as Engine.compile exports them (descriptors and the pat / apat /
thr tables of the not-Q and the Q program), so that the C twin can sample from
them without a device.  Needs a GPU; the GPU tests compare every fresh compile
with the file.

    python tests/golden/gen_montecarlo_programs.py
"""
import importlib
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import conftest  # noqa: E402,F401  (the import paths of the suite)
from montecarlo_programs import GOLDEN_PROGRAMS, PROGRAMS  # noqa: E402


def main():
    eng = importlib.import_module(f"{conftest.PKG_NAME}.engine").Engine(0)
    out = {}
    for name, (n, pair, _, _) in PROGRAMS.items():
        info = eng.compile(n, *pair())
        for kind in ("notq", "q"):
            assert info[kind]["nfac"] == len(info[kind]["desc"])
            for k in ("desc", "pat", "apat", "thr"):
                out[f"{name}.{kind}.{k}"] = info[kind][k]
        print(name, n, len(info["notq"]["pat"]), "+", len(info["q"]["pat"]), "entries")
    eng.close()
    np.savez_compressed(GOLDEN_PROGRAMS, **out)
    print("wrote", GOLDEN_PROGRAMS, GOLDEN_PROGRAMS.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
