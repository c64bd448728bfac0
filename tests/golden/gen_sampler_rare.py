#!/usr/bin/env python3
"""Fixture of the samplers' rare rejection branches (tests/test_sampler_rare.py,
tests/test_gpu_sampler_rare.py, tests/test_closed_form.py): positions (key,
entry) at which a Q-correlated entry leaves the common path of its rank draw,
found by the C twin's scanner (oracle_lib.scan_rare, which tests Philox words
against the thresholds and calls no sampler) and described by the Python
restatement (tests/sampler_restate.py).  CPU only.

Kinds (csrc/qba_lists_sample.h): closed form, n <= 11 -- `w0` (w1 rejected, the
27-bit second candidate accepted), `retry1` (both rejected, word 0 of retry
block 1 accepted), `retry_late` (a later retry word accepted); 64-bit
permutation of the table samplers -- `retry64` (first F rejected).

Two families of records (n, sampler, kind, key, entry, h = entry & 1, word = the
accepted rank word, where, values of the n + 1 groups):

  anywhere  under the one key ANY_KEY, entries from 16 on (half h = 0) and from
            2^35 + 16 on (half h = 1, so the retry counter's high word is
            nonzero there), for the list calls that take `first`:
            w0 at n = 3..11 and retry1 at n = 9, 10, 11, one per half;
            retry_late at n = 11 and retry64 at n = 14, 15, one from each start.
  small     entries below 64 under keys from SMALL_KEY0 on, for the batched
            and Monte-Carlo calls (entries [0, count) under key seed_base + i):
            w0 at n = 7, 9, 10, 11, retry1 at n = 10, 11, retry64 at n = 15.
            These also hold `naive`, the values had the first candidate been
            taken without its test (asserted different), and `n_dishonest`:
            a number of traitors at which the host model (montecarlo.run_host
            on injected lists, count = entry + 1, noiseless and at flip_q16 =
            1) gives another row for the true lists than for the lists with
            that entry replaced by `naive` -- or null when none of the cell's
            candidates has one, which the generator refuses for the cells the
            Monte-Carlo tests need (MC_CELLS).  Each cell keeps its first
            candidate and its first sensitive one.

Out of scope: retry64 at n = 12 and 13.  Its probability per Q entry is
(2^64 mod n!) / 2^64 = 1.1e-11 and 8.9e-11, about 1e11 and 1e10 Q entries per
hit against 1.8e-9 and 1.6e-8 at n = 14 and 15; those two loops are the same
template code as n = 14 and 15 and stay unreached.

The model's lists at n = 15: the Q entries are the C twin's under the shipped Q
program (the GHZ table: big15's Q program in tests/golden/montecarlo_programs.npz,
which the GPU tests hold to Engine.prepare(15)); the shipped not-Q program is
not in a CPU fixture, but its entries have L0 == L1, which neither the count
tables nor the rounds read, so all-zero entries stand in for them here.  The
GPU test repeats the comparison on the true lists.

The header of the JSON file records, per cell, the first-candidate Philox
blocks the scan read up to the last record kept.

    python tests/golden/gen_sampler_rare.py
"""
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import conftest  # noqa: E402,F401  (the import paths of the suite)
import oracle_lib  # noqa: E402
from montecarlo_programs import host_info  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402
from sampler_restate import NO_PROGRAM, closed_classify, perm64_classify  # noqa: E402

OUT = HERE / "sampler_rare.json"
ANY_KEY = 0x5EED5A3
STARTS = {0: 16, 1: (1 << 35) + 16}   # half h -> first entry scanned
SPAN = 1 << 40                        # entries scanned from a start at most
SMALL_KEY0, SMALL_KEYS, SMALL_ENTRIES, CANDIDATES = 1 << 20, 1 << 36, 64, 12
Q_PROGRAMS = {14: "narrow14", 15: "big15"}  # programs whose Q program is the shipped one of that n

ANYWHERE = [("w0", n, True) for n in range(3, 12)] + [("retry1", n, True) for n in (9, 10, 11)] + \
    [("retry_late", 11, False), ("retry64", 14, False), ("retry64", 15, False)]   # (kind, n, one per half)
SMALL = [("w0", 7), ("w0", 9), ("w0", 10), ("w0", 11), ("retry1", 10), ("retry1", 11), ("retry64", 15)]
MC_CELLS = {("w0", 7), ("w0", 11), ("retry64", 15), ("retry1", 11)}  # must have a sensitive record


def sampler_of(kind):
    return "perm64" if kind == "retry64" else "closed"


def q_program(n):
    return host_info(Q_PROGRAMS[n])["q"]


def classify(n, kind, key, entry):
    if sampler_of(kind) == "closed":
        return closed_classify(n, key, entry)
    return perm64_classify(n, key, entry, q_program(n))


def record(n, kind, hit, small):
    got, word, where, values, naive = classify(n, kind, hit["key"], hit["entry"])
    assert (got, word, where) == (kind, hit["word"], hit["where"]), (n, kind, hit, got, word, where)
    rec = {"n": n, "sampler": sampler_of(kind), "kind": kind, "key": hit["key"], "entry": hit["entry"],
           "h": hit["entry"] & 1, "word": word, "where": where, "values": values}
    if small:
        assert naive != values, (n, kind, hit)
        rec["naive"] = naive
        rec["n_dishonest"] = None
    return rec


def model_lists(n, key, count):
    """[1, n+1, count] uint8: the lists the host model decides (module docstring for n = 15)."""
    if n <= 11:
        li = oracle_lib.sample(n, key, 0, count, NO_PROGRAM, NO_PROGRAM, closed=True)
    else:
        li = oracle_lib.sample(n, key, 0, count, NO_PROGRAM, q_program(n), closed=False)
    return np.array(li)[None]


def sensitive_nd(mc, rec):
    """The smallest n_dishonest at which the host model tells the true entry
    from the naive one, without noise and at flip_q16 = 1; None if there is none."""
    n, key, count = rec["n"], rec["key"], rec["entry"] + 1
    true = model_lists(n, key, count)
    assert true[0, :, -1].tolist() == rec["values"]
    naive = true.copy()
    naive[0, :, -1] = rec["naive"]
    for nd in range(n + 1):
        if all(not np.array_equal(mc.run_host(n, count, nd, 1, key, OracleEngine(), lists=true, flip_q16=k),
                                  mc.run_host(n, count, nd, 1, key, OracleEngine(), lists=naive, flip_q16=k))
               for k in (0, 1)):
            return nd
    return None


def main():
    mc = importlib.import_module(f"{conftest.PKG_NAME}.montecarlo")
    cells, anywhere, small = [], [], []
    for kind, n, per_half in ANYWHERE:
        for h, e0 in STARTS.items():
            t0 = time.time()
            hits = oracle_lib.scan_rare(n, sampler_of(kind), kind, ANY_KEY, 1, e0, SPAN, 1,
                                        h if per_half else -1)
            if not hits:
                raise SystemExit(f"anywhere {kind} n={n} from {e0}: nothing in {SPAN} entries")
            anywhere.append(record(n, kind, hits[0], False))
            cells.append({"family": "anywhere", "kind": kind, "n": n, "from": e0, "half": h if per_half else None,
                          "blocks": hits[0]["blocks"]})
            print(f"anywhere {kind:10s} n={n:2d} from {e0:#x}: entry {hits[0]['entry']:#x}, "
                  f"{hits[0]['blocks']:.3e} blocks, {time.time() - t0:.1f} s", flush=True)
    for kind, n in SMALL:
        t0 = time.time()
        hits = oracle_lib.scan_rare(n, sampler_of(kind), kind, SMALL_KEY0, SMALL_KEYS, 0, SMALL_ENTRIES, CANDIDATES)
        if not hits:
            raise SystemExit(f"small {kind} n={n}: nothing under {SMALL_KEYS} keys")
        recs = [record(n, kind, hit, True) for hit in hits]
        keep, tried = [0], 0
        for i, rec in enumerate(recs):
            tried += 1
            rec["n_dishonest"] = sensitive_nd(mc, rec)
            if rec["n_dishonest"] is not None:
                keep = sorted({0, i})
                break
        if recs[keep[-1]]["n_dishonest"] is None and (kind, n) in MC_CELLS:
            raise SystemExit(f"small {kind} n={n}: none of {len(recs)} candidates moves the host model's row")
        small += [recs[i] for i in keep]
        cells.append({"family": "small", "kind": kind, "n": n, "candidates_tried": tried,
                      "blocks": hits[keep[-1]]["blocks"]})
        print(f"small    {kind:10s} n={n:2d}: " + ", ".join(
            f"key {recs[i]['key']:#x} entry {recs[i]['entry']} nd {recs[i]['n_dishonest']}" for i in keep) +
            f", {hits[keep[-1]]['blocks']:.3e} blocks, {time.time() - t0:.1f} s", flush=True)
    doc = {"header": {"generator": "tests/golden/gen_sampler_rare.py", "any_key": ANY_KEY, "small_key0": SMALL_KEY0,
                      "small_entries": SMALL_ENTRIES, "cells": cells},
           "anywhere": anywhere, "small": small}
    OUT.write_text(json.dumps(doc, indent=1) + "\n")
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
