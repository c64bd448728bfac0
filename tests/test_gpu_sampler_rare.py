"""The samplers' rare rejection branches in every kernel that samples, at the
positions of tests/golden/sampler_rare.json (tests/golden/gen_sampler_rare.py
describes kinds and families; tests/test_sampler_rare.py holds every record to
the Python restatement and the C twin to it, on the CPU).

  list kernels      the `anywhere` records: sample, sample_check, sample_packed,
                    sample_check_packed and the two deferred forms, 24 entries
                    from first = entry - d for every d in 0..15, so the rare
                    entry sits in every slot of a thread's entries, on both
                    halves of a Philox block, behind aligned and unaligned
                    heads; with launches cut (chunk knob) so that it is the
                    first and the last entry of a launch; at n = 11 with pair
                    bins forced; at n = 14 and 15 under a general program too
                    (qba_sample_entry's loop beside qba_sample_entry_fast's).
  batched kernels   the `small` records: sample_check_batched, packed, and the
                    noisy forms, the rare instance at index 0, 2 and 4 of 5.
  Monte-Carlo       the `small` records with n_dishonest: montecarlo_sampled
                    and montecarlo_curve_sampled, noiseless and at flip_q16 = 1,
                    against the host model on the twin's lists -- whose row is
                    asserted to change when the rare entry's values are
                    replaced by the ones a missing rejection test would give.

Every comparison is exact; the reference is the C twin (lists, counts) and
montecarlo.run_host / noise_masks, never a kernel."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_lib
from conftest import GOLDEN, sub
from montecarlo_programs import PROGRAMS, host_info, same_program, twin_lists
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

FIXTURE = json.loads((GOLDEN / "sampler_rare.json").read_text())
ANYWHERE, SMALL = FIXTURE["anywhere"], FIXTURE["small"]
SENSITIVE = [r for r in SMALL if r["n_dishonest"] is not None]
GENERAL = {14: "narrow14", 15: "big15"}   # general programs whose Q program is the shipped one of their n
COUNT, LEAD = 24, 15                      # entries per list call; the rare entry sits at index d = 0..LEAD
CHUNKS = {8: (0, 7, 8, 15), 5: (0, 4, 5, 9, 10, 14, 15)}   # chunk -> the d that put it first or last in a launch
INST, BIG = 5, 130
MASK64 = (1 << 64) - 1


def rec_id(r):
    return f"{r['kind']}-n{r['n']}-k{r['key']:x}-e{r['entry']:x}"


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)[0].tolist()
        raise AssertionError(f"{what} first difference at {at}: {got[tuple(at)]} != {want[tuple(at)]}")


def _eq_counts(c, want, what):
    for name, got, w in zip("HCP", c.numpy(), want):
        _eq(got, w, f"{what} {name}:")


@pytest.fixture(scope="module")
def engines(engine):
    """shipped: the session's engine; knobs: a fresh one for the launch-shape
    knobs (shipped programs); general: one with GENERAL compiled.  The CPU
    tests take the Q program of GENERAL's golden files for the shipped one:
    held here."""
    em = sub("engine")
    knobs, general = em.Engine(0), em.Engine(0)
    for n, name in GENERAL.items():
        info = general.compile(n, *PROGRAMS[name][1]())
        assert not info["closed"] and not info["canonical"]
        for kind in ("notq", "q"):
            assert same_program(info[kind], host_info(name)[kind]), (name, kind)
        shipped = engine.prepare(n)
        assert shipped["canonical"] and not shipped["closed"] and same_program(shipped["q"], info["q"]), n
    yield SimpleNamespace(shipped=engine, knobs=knobs, general=general)
    knobs.close()
    general.close()


def _list_calls(eng, r, ds, what):
    """Every list call at first = entry - d, d in ds, against the twin."""
    import torch
    unpack = sub("engine").unpack_nibbles
    n, key, entry = r["n"], r["key"], r["entry"]
    info = eng.prepare(n)
    ref = oracle_lib.sample(n, key, entry - LEAD, LEAD + COUNT, info["notq"], info["q"], info["closed"])
    assert ref[:, LEAD].tolist() == r["values"], what
    wants, pending = {}, []
    with oracle_lib.single_thread():
        for d in ds:
            want = np.ascontiguousarray(ref[:, LEAD - d:LEAD - d + COUNT])
            H, C, P, bad = oracle_lib.counts(want, n)
            assert bad == 0 and want[:, d].tolist() == r["values"]
            wants[d] = (want, (H, C, P))
    for d in ds:
        first, (want, tables) = entry - d, wants[d]
        w = f"{what} d={d}"
        _eq(eng.sample(n, key, first, COUNT)[:, :COUNT].cpu().numpy(), want, w + " sample:")
        lists, c = eng.sample_check(n, key, first, COUNT)
        _eq(lists[:, :COUNT].cpu().numpy(), want, w + " sample_check:")
        _eq_counts(c, tables, w + " sample_check")
        _eq(unpack(eng.sample_packed(n, key, first, COUNT).cpu().numpy(), COUNT), want, w + " sample_packed:")
        packed, c = eng.sample_check_packed(n, key, first, COUNT)
        _eq(unpack(packed.cpu().numpy(), COUNT), want, w + " sample_check_packed:")
        _eq_counts(c, tables, w + " sample_check_packed")
    for d in ds:  # one chain of deferred calls, then the flush
        pending.append((d, False, eng.sample_check(n, key, entry - d, COUNT, deferred=True)))
        pending.append((d, True, eng.sample_check_packed(n, key, entry - d, COUNT, deferred=True)))
    eng.flush_deferred()
    torch.cuda.synchronize()
    for d, is_packed, (rows, c) in pending:
        want, tables = wants[d]
        w = f"{what} d={d} deferred packed={is_packed}"
        got = unpack(rows.cpu().numpy(), COUNT) if is_packed else rows[:, :COUNT].cpu().numpy()
        _eq(got, want, w + ":")
        _eq_counts(c, tables, w)


@pytest.mark.parametrize("r", ANYWHERE, ids=rec_id)
def test_list_kernels_at_every_slot_and_launch_edge(engines, r):
    n = r["n"]
    assert r["entry"] >= LEAD
    _list_calls(engines.shipped, r, range(LEAD + 1), "shipped")
    try:
        for chunk, ds in CHUNKS.items():
            assert all(d % chunk in (0, chunk - 1) for d in ds)
            assert any(d % chunk == 0 and d for d in ds) and any(d % chunk == chunk - 1 for d in ds)
            engines.knobs.set_test_knobs(chunk=chunk)
            _list_calls(engines.knobs, r, ds, f"chunk={chunk}")
        if n == 11:
            engines.knobs.set_test_knobs(pb_min=0)
            _list_calls(engines.knobs, r, range(LEAD + 1), "pair bins")
    finally:
        engines.knobs.set_test_knobs()
    if n in GENERAL:
        try:
            _list_calls(engines.general, r, range(LEAD + 1), GENERAL[n])
            engines.general.set_test_knobs(chunk=8)
            _list_calls(engines.general, r, CHUNKS[8], GENERAL[n] + " chunk=8")
        finally:
            engines.general.set_test_knobs()


def _batched(eng, r, what):
    em, mc = sub("engine"), sub("montecarlo")
    n, key, entry = r["n"], r["key"], r["entry"]
    info = eng.prepare(n)
    for j in (0, 2, 4):
        base = key - j
        top = twin_lists(info, base, INST, BIG)
        assert top[j, :, entry].tolist() == r["values"], what
        for count in (entry + 1, BIG):
            clean = top[:, :, :count]
            for k in (0, 1, 0x1000):
                want = clean if k == 0 else np.stack(
                    [clean[i] ^ mc.noise_masks(n, (base + i) & MASK64, count, k) for i in range(INST)])
                with oracle_lib.single_thread():
                    tables = [oracle_lib.counts(want[i], n) for i in range(INST)]
                assert not any(t[3] for t in tables)
                for packed in (False, True):
                    w = f"{what} j={j} count={count} k={k:#x} packed={packed}"
                    lists, c = eng.sample_check_batched(n, base, INST, count, packed=packed, flip_q16=k)
                    raw = lists.cpu().numpy()
                    got = em.unpack_nibbles(raw.reshape(INST * (n + 1), -1), count).reshape(INST, n + 1, count) \
                        if packed else raw[:, :, :count]
                    _eq(got, want, w + " lists:")
                    for name, g, idx in zip("HCP", c.numpy(), range(3)):
                        _eq(g, np.stack([t[idx] for t in tables]), f"{w} {name}:")


@pytest.mark.parametrize("r", SMALL, ids=rec_id)
def test_batched_kernels_with_the_rare_instance_at_three_indices(engines, r):
    assert r["key"] >= 4 and r["entry"] < 64
    _batched(engines.shipped, r, "shipped")
    if r["n"] in GENERAL:
        _batched(engines.general, r, GENERAL[r["n"]])


def _montecarlo(eng, r, nd, sensitive, what):
    """Both fused kernels against run_host on the twin's lists, the rare
    instance in the middle of three; `sensitive`: the model's row at
    checkpoint entry + 1 must change under the naive values, under the same
    noise masks, and the one at checkpoint entry must not."""
    mc = sub("montecarlo")
    n, key, entry = r["n"], r["key"], r["entry"]
    info = eng.prepare(n)
    base, inst, cps = key - 1, 3, [entry, entry + 1, BIG]
    li = twin_lists(info, base, inst, BIG)
    assert li[1, :, entry].tolist() == r["values"], what
    naive = np.array(li)
    naive[1, :, entry] = r["naive"]
    host = lambda lists, c, k: mc.run_host(n, c, nd, inst, base, OracleEngine(), lists=lists[:, :, :c], flip_q16=k)  # noqa: E731
    for k in (0, 1):
        want = [host(li, c, k) for c in cps]
        if sensitive:
            _eq(host(naive, entry, k), want[0], f"{what} k={k} naive lists before the rare entry:")
            other = host(naive, entry + 1, k)
            assert not np.array_equal(other[1], want[1][1]), (what, k, "the model does not see the rare entry")
            _eq(other[[0, 2]], want[1][[0, 2]], f"{what} k={k} other instances:")
        for c, w in zip(cps, want):
            _eq(eng.montecarlo_sampled(n, nd, base, inst, c, flip_q16=k).cpu().numpy(), w, f"{what} k={k} single {c}:")
        got = eng.montecarlo_curve_sampled(n, nd, base, inst, cps, flip_q16=k).cpu().numpy()
        _eq(got, np.stack(want), f"{what} k={k} curve:")
        assert not got[:, :, 3].any()


@pytest.mark.parametrize("r", SENSITIVE, ids=rec_id)
def test_montecarlo_kernels_decide_the_rare_entry(engines, r):
    """General program at n = 15 (qba_sample_entry's loop inside the fused
    kernels): its not-Q entries differ from the shipped program's, so the
    recorded n_dishonest carries no promise there; rows against the model only."""
    _montecarlo(engines.shipped, r, r["n_dishonest"], True, "shipped")
    if r["n"] in GENERAL:
        _montecarlo(engines.general, r, r["n_dishonest"], False, GENERAL[r["n"]])


def test_fixture_covers_every_family_the_kernels_need():
    cells = {(r["kind"], r["n"]) for r in ANYWHERE}
    assert {("w0", n) for n in range(3, 12)} | {("retry1", n) for n in (9, 10, 11)} | \
        {("retry_late", 11), ("retry64", 14), ("retry64", 15)} <= cells
    assert {("w0", 7), ("w0", 9), ("w0", 10), ("w0", 11), ("retry1", 10), ("retry1", 11), ("retry64", 15)} <= \
        {(r["kind"], r["n"]) for r in SMALL}
    mcs = {(r["kind"], r["n"]) for r in SENSITIVE}
    assert {("w0", 7), ("w0", 11), ("retry64", 15)} <= mcs and mcs & {("retry1", 10), ("retry1", 11)}
