"""The rare rejection branches of the samplers' rank draws, on the CPU: the
fixture tests/golden/sampler_rare.json (written by gen_sampler_rare.py, which
describes kinds and families) against the Python restatement
(tests/sampler_restate.py), the C twin against the restatement at every record,
and the twin's scanner against the restatement on a range small enough to
classify entry by entry.  No device calls.

Per Q entry the branches are taken with probability (2^32 mod n!) / 2^32 for
the w0 fallback, times (2^27 mod n!) / 2^27 for the closed-form retry, and
(2^64 mod n!) / 2^64 for the 64-bit retry:

    n      w0 fallback   closed-form retry   64-bit retry
    3      9.3e-10       1.4e-17
    4, 5   3.7e-9        2.2e-16
    6      6.0e-8        1.6e-13
    7      6.0e-8        1.1e-12
    8      6.0e-8        1.5e-11
    9      6.6e-5        1.5e-7
    10     4.9e-4        1.3e-5
    11     5.6e-3        6.0e-4
    12 .. 15                                 1.1e-11, 8.9e-11, 1.8e-9, 1.6e-8

First-candidate Philox blocks the generator's scans read per cell (the
fixture's header; a closed-form block holds two entries, about one of them Q,
a 64-bit block one entry, Q half of the time), half 0 from entry 16 / half 1
from entry 2^35 + 16:

    anywhere w0      n = 3: 2.1e8 / 4.0e8    4: 2.1e8 / 4.0e8    5: 9.2e8 / 4.6e8
                     6: 6.3e6 / 4.9e7        7: 2.3e7 / 5.9e6    8: 7.5e7 / 2.6e7
                     9: 7.2e4 / 1.2e5        10: 734 / 750       11: 20 / 223
    anywhere retry1  n = 9: 2.8e7 / 2.0e7    10: 1.5e4 / 1.9e5   11: 1.3e4 / 7.8e3
    anywhere retry_late n = 11: 5.6e4 / 7.5e4
    anywhere retry64 n = 14: 8.6e8 / 1.1e9   15: 1.5e6 / 4.9e7
    small (keys from 2^20, entries below 64, to the last record kept)
             w0      n = 7: 1.3e8   9: 8.1e3   10: 1.9e3   11: 33
             retry1  n = 10: 7.5e4  11: 578
             retry64 n = 15: 1.7e8

The whole file regenerates in under a minute on 8 cores.  retry64 at n = 12 and
13 (about 1e11 and 1e10 Q entries per hit) is out of the fixture's reach.
"""
import importlib
import json

import numpy as np
import pytest

import oracle_lib
from conftest import GOLDEN, PKG_NAME
from montecarlo_programs import host_info
from oracle_engine import OracleEngine
from sampler_restate import NO_PROGRAM, closed_classify, closed_entry_py, perm64_classify

FIXTURE = json.loads((GOLDEN / "sampler_rare.json").read_text())
ANYWHERE, SMALL = FIXTURE["anywhere"], FIXTURE["small"]
RECORDS = [("anywhere", r) for r in ANYWHERE] + [("small", r) for r in SMALL]
Q_PROGRAMS = {14: "narrow14", 15: "big15"}  # their Q program is the shipped one of that n (held to it on the GPU)


def rec_id(r):
    return f"{r['kind']}-n{r['n']}-k{r['key']:x}-e{r['entry']:x}"


IDS = [f"{fam}-{rec_id(r)}" for fam, r in RECORDS]


def restated(r):
    if r["sampler"] == "closed":
        return closed_classify(r["n"], r["key"], r["entry"])
    return perm64_classify(r["n"], r["key"], r["entry"], host_info(Q_PROGRAMS[r["n"]])["q"])


def test_required_cells_are_present():
    cells = {}
    for r in ANYWHERE:
        cells.setdefault((r["kind"], r["n"]), []).append(r)
    for n in range(3, 12):
        assert {r["h"] for r in cells["w0", n]} == {0, 1}, n
    for n in (9, 10, 11):
        assert {r["h"] for r in cells["retry1", n]} == {0, 1}, n
    assert len(cells["retry_late", 11]) >= 1
    for n in (14, 15):
        assert len({r["entry"] for r in cells["retry64", n]}) >= 2, n
    assert all(r["key"] == FIXTURE["header"]["any_key"] and r["entry"] >= 16 for r in ANYWHERE)
    assert any(r["entry"] >= 1 << 33 for r in ANYWHERE if r["kind"] in ("retry1", "retry_late"))  # p_hi != 0
    small = {(r["kind"], r["n"]) for r in SMALL}
    assert {("w0", 7), ("w0", 9), ("w0", 10), ("w0", 11), ("retry1", 10), ("retry1", 11), ("retry64", 15)} <= small
    assert all(r["entry"] < 64 and r["key"] >= 4 for r in SMALL)
    # the Monte-Carlo cells: a record the host model is sensitive to
    sensitive = {(r["kind"], r["n"]) for r in SMALL if r["n_dishonest"] is not None}
    assert {("w0", 7), ("w0", 11), ("retry64", 15)} <= sensitive
    assert ("retry1", 10) in sensitive or ("retry1", 11) in sensitive


@pytest.mark.parametrize("fam,r", RECORDS, ids=IDS)
def test_record_is_of_its_kind_and_holds_the_restatements_values(fam, r):
    kind, word, where, values, naive = restated(r)
    assert (kind, word, where, values) == (r["kind"], r["word"], r["where"], r["values"])
    assert r["h"] == r["entry"] & 1 and r["sampler"] == ("perm64" if kind == "retry64" else "closed")
    assert (where == 0) == (kind in ("w0", "retry1")) and len(values) == r["n"] + 1
    assert sorted(v ^ values[0] for v in values) == list(range(r["n"] + 1))  # r ^ pi, pi(0) = 0
    if fam == "small":
        assert naive == r["naive"] != values and sorted(v ^ naive[0] for v in naive) == list(range(r["n"] + 1))


@pytest.mark.parametrize("fam,r", RECORDS, ids=IDS)
def test_twin_equals_the_restatement(fam, r):
    """oracle_lib.sample at the record and at the Q entries around it.  The
    64-bit records run sample_outcome's retry loop: under the program whose Q
    program is the shipped one (and, at n = 15, whose not-Q program is a
    general one, big15), and under that Q program with an empty not-Q program."""
    n, key, e = r["n"], r["key"], r["entry"]
    first = max(e - 5, 0)
    if r["sampler"] == "closed":
        got = oracle_lib.sample(n, key, first, 11, NO_PROGRAM, NO_PROGRAM, closed=True)
        assert got[:, e - first].tolist() == r["values"]
        for k in range(11):
            assert got[:, k].tolist() == closed_entry_py(n, key, first + k), k
        return
    info = host_info(Q_PROGRAMS[n])
    for notq in (info["notq"], NO_PROGRAM):
        got = oracle_lib.sample(n, key, first, 11, notq, info["q"], closed=False)
        assert got[:, e - first].tolist() == r["values"]
        for k in range(11):
            kind, _, _, values, _ = perm64_classify(n, key, first + k, info["q"])
            assert kind == "notq" or got[:, k].tolist() == values, k


@pytest.mark.parametrize("r", [r for r in SMALL if r["n_dishonest"] is not None], ids=rec_id)
def test_host_model_tells_the_true_entry_from_the_naive_one(r):
    """What the Monte-Carlo GPU tests rely on, a property of the reference
    alone: at count = entry + 1 and the recorded n_dishonest the row of
    montecarlo.run_host changes when the entry's values are replaced by
    `naive`, without noise and under the masks of flip_q16 = 1, and at count =
    entry it cannot.  n = 15: all-zero not-Q entries stand in for the shipped
    program's (L0 == L1 there, which the tables skip; gen_sampler_rare.py)."""
    mc = importlib.import_module(f"{PKG_NAME}.montecarlo")
    n, key, e, nd = r["n"], r["key"], r["entry"], r["n_dishonest"]
    if n <= 11:
        true = oracle_lib.sample(n, key, 0, e + 1, NO_PROGRAM, NO_PROGRAM, closed=True)
    else:
        true = oracle_lib.sample(n, key, 0, e + 1, NO_PROGRAM, host_info(Q_PROGRAMS[n])["q"], closed=False)
    true = np.array(true)[None]
    naive = true.copy()
    naive[0, :, e] = r["naive"]
    assert true[0, :, e].tolist() == r["values"] and 0 <= nd <= n
    for k in (0, 1):
        rows = [mc.run_host(n, e + 1, nd, 1, key, OracleEngine(), lists=li, flip_q16=k) for li in (true, naive)]
        assert not rows[0][0, 3] and not rows[1][0, 3] and not np.array_equal(rows[0], rows[1]), k


def test_header_holds_the_blocks_scanned_per_cell():
    head = FIXTURE["header"]
    cells = {(c["family"], c["kind"], c["n"], c.get("from")): c for c in head["cells"]}
    assert len(cells) == len(head["cells"]) and all(c["blocks"] >= 1 for c in cells.values())
    for r in ANYWHERE:
        e0 = 16 if r["entry"] < 1 << 35 else (1 << 35) + 16
        shift = 1 if r["sampler"] == "closed" else 0
        assert cells["anywhere", r["kind"], r["n"], e0]["blocks"] == ((r["entry"] - e0) >> shift) + 1
    for kind, n in {(r["kind"], r["n"]) for r in SMALL}:
        last = [r for r in SMALL if (r["kind"], r["n"]) == (kind, n)][-1]
        per_key = head["small_entries"] // (2 if last["sampler"] == "closed" else 1)
        unit = last["entry"] >> (1 if last["sampler"] == "closed" else 0)
        assert cells["small", kind, n, None]["blocks"] == (last["key"] - head["small_key0"]) * per_key + unit + 1


@pytest.mark.parametrize("n", [10, 11])
def test_scanner_finds_exactly_the_restatements_positions_in_order(n):
    """Entries [0, 2^15) of 3 keys, every entry classified by the restatement:
    the scanner returns those positions and no others, in scan order, for
    either half alone too, whatever the thread count, and the first `cap` of
    them when capped.  (The 64-bit kind has no hit in a range this small; its
    fixture records are classified by the restatement above.)"""
    key0, keys, ne = 0xABCDE, 3, 1 << 15
    want = {k: [] for k in ("w0", "retry1", "retry_late")}
    for key in range(key0, key0 + keys):
        ctr = np.zeros((ne // 2, 4), np.uint32)
        ctr[:, 0] = np.arange(ne // 2)
        x = oracle_lib.philox(ctr, key)
        nf = int(np.prod(np.arange(1, n + 1)))
        # prefilter on w1's test alone (vectorised); the restatement decides
        for h in (0, 1):
            x[:, 2 * h + 1] = np.where((x[:, 2 * h + 1].astype(np.uint64) * nf) & 0xFFFFFFFF >= (1 << 32) % nf, 0, 1)
        for p in np.nonzero(x[:, 1] | x[:, 3])[0].tolist():
            for e in (2 * p, 2 * p + 1):
                kind, word, where, _, _ = closed_classify(n, key, e)
                if kind in want:
                    want[kind].append((key, e, word, where))
    assert len(want["w0"]) > 20 and (n < 11 or len(want["retry1"]) > 2)
    for kind, hits in want.items():
        for team in ("all", "one"):
            for h in (-1, 0, 1):
                sel = [t for t in hits if h < 0 or t[1] & 1 == h]
                if team == "one":
                    with oracle_lib.single_thread():
                        got = oracle_lib.scan_rare(n, "closed", kind, key0, keys, 0, ne, len(hits) + 5, h)
                else:
                    got = oracle_lib.scan_rare(n, "closed", kind, key0, keys, 0, ne, len(hits) + 5, h)
                assert [(g["key"], g["entry"], g["word"], g["where"]) for g in got] == sel, (kind, team, h)
        if len(hits) >= 3:
            got = oracle_lib.scan_rare(n, "closed", kind, key0, keys, 0, ne, 3)
            assert [(g["key"], g["entry"]) for g in got] == [t[:2] for t in hits[:3]]
            assert got[-1]["blocks"] == (hits[2][0] - key0) * (ne // 2) + (hits[2][1] >> 1) + 1


def test_scanner_refuses_what_it_cannot_scan():
    for args in ((12, "closed", "w0", 0, 1, 0, 64), (11, "closed", "w0", 0, 1, 1, 64), (11, "closed", "w0", 0, 1, 0, 63),
                 (16, "perm64", "retry64", 0, 1, 0, 64), (11, "closed", "retry64", 0, 1, 0, 64),
                 (15, "perm64", "w0", 0, 1, 0, 64)):
        with pytest.raises(ValueError):
            oracle_lib.scan_rare(*args)
    assert oracle_lib.scan_rare(11, "closed", "w0", 0, 0, 0, 64) == []
