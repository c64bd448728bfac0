"""The trace kernels on the GPU.  The reference is
always montecarlo.trace_host on the same keys: the traced row, the exact event
counts and every stored event are compared word for word.  For n <= 11 the
host samples with the C twin; above, it takes the lists the device samples."""
import re

import numpy as np
import pytest

from conftest import sub
from montecarlo_cases import HOSTILE, HOSTILE_IDS, SWEEP, SWEEP_IDS, hostile_lists
from test_montecarlo_adversary import HostEngine, PRESETS

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 7, 11, 12, 15]
SIZES = [0, 3, 65]
FLIPS = [0, 1, 0x1000]
IDX = [0, 1, 66, 5, 5, (1 << 40) + 3]  # unsorted, repeated, large
POLICIES = {k: PRESETS[k] for k in ("reference", "reorder_low", "strip")}
GRID_BASE = 0xADA11CE
MASK64 = (1 << 64) - 1
CAP = 256    # above every rank's event count on the grid (the most is 152, n = 15 with 14 traitors)
GUARD = 0x5A5A5A5A


def _nds(n):
    return sorted({min(max(d, 0), n) for d in (0, 1, n // 3, n - 1)})


def _host(engine, n, sizeL, nd, idx, base, flip, word, lists=None):
    """trace_host of the keys base + idx; n > 11: on the device's own samples."""
    mc = sub("montecarlo")
    if lists is None and n > 11:
        lists = np.zeros((len(idx), n + 1, sizeL), np.uint8)
        for j, i in enumerate(idx if sizeL else []):
            lists[j] = engine.sample(n, (base + i) & MASK64, 0, sizeL).cpu().numpy()[:, :sizeL]
    return mc.trace_host(n, sizeL, nd, idx, base, HostEngine(), lists=lists, flip_q16=flip, adversary=word)


def _same(got, want, what, slots=None):
    """rows, counts and the stored events of a device trace against trace_host's."""
    mc = sub("montecarlo")
    rows, counts, events = (t.cpu().numpy() for t in got)
    wrows, wcounts, wevents = want
    slots = range(len(wrows)) if slots is None else slots
    cap = events.shape[2]
    for j in slots:
        assert rows[j].tolist() == wrows[j].tolist(), f"{what} slot {j}: row"
        assert counts[j].tolist() == wcounts[j].tolist(), f"{what} slot {j}: counts"
        dev = mc.trace_events(counts, events, j)
        for r, (d, h) in enumerate(zip(dev, wevents[j])):
            if d != h[:cap]:
                k = next(i for i, (a, b) in enumerate(zip(d, h)) if a != b)
                raise AssertionError(f"{what} slot {j} rank {r} event {k}: device "
                                     f"{mc.event_fields(d[k][0])} {d[k][1]:#x} != host "
                                     f"{mc.event_fields(h[k][0])} {h[k][1]:#x}")


@pytest.mark.parametrize("sizeL", SIZES)
@pytest.mark.parametrize("n", NS)
def test_main_grid_equals_the_host_specification(engine, n, sizeL):
    for nd in _nds(n):
        for name, word in POLICIES.items():
            for flip in FLIPS:
                got = engine.montecarlo_trace_sampled(n, nd, GRID_BASE, IDX, sizeL, cap=CAP, flip_q16=flip,
                                                      adversary=word)
                want = _host(engine, n, sizeL, nd, IDX, GRID_BASE, flip, word)
                assert int(want[1].max()) <= CAP
                _same(got, want, f"n={n} sizeL={sizeL} nd={nd} {name} flip={flip:#x}")


@pytest.mark.parametrize("n", [7, 11])
def test_traced_rows_equal_the_decision_kernels_rows_for_a_whole_batch(engine, n):
    inst, sizeL = 67, 65
    for nd in _nds(n):
        for name, word in POLICIES.items():
            for flip in FLIPS:
                rows, counts, _ = engine.montecarlo_trace_sampled(n, nd, GRID_BASE, list(range(inst)), sizeL, cap=4,
                                                                  flip_q16=flip, adversary=word)
                want = engine.montecarlo_sampled(n, nd, GRID_BASE, inst, sizeL, flip_q16=flip, adversary=word)
                assert rows.cpu().numpy().tolist() == want.cpu().numpy().tolist(), (n, nd, name, flip)
                assert (counts[:, 1:] > 0).all() and not counts[:, 0].any()


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_lists_form_on_every_hostile_and_sweep_set(engine, case):
    n, nd, sizeL, base, keys = case["n"], case["nDishonest"], case["sizeL"], case["base"], case["keys"]
    li = np.array(hostile_lists(case))
    idx = list(range(keys))
    for name, word in (("reference", PRESETS["reference"]), ("strip", PRESETS["strip"])):
        want = _host(engine, n, sizeL, nd, idx, base, 0, word, lists=li)
        cap = max(int(want[1].max()), 1)   # at the largest count: every event is stored
        got = engine.montecarlo_trace_lists(n, nd, base, idx, li, sizeL, cap=cap, adversary=word)
        _same(got, want, f"{case['name']} {name}")
        assert got[0].cpu().numpy().tolist() == \
            engine.montecarlo_lists(n, nd, base, li, sizeL, adversary=word).cpu().numpy().tolist()


def test_lists_form_with_noise_equals_the_host_specification(engine):
    case = next(c for c in HOSTILE if c["n"] == 7)
    n, nd, sizeL, base = 7, case["nDishonest"], case["sizeL"], case["base"]
    li = np.array(hostile_lists(case))[:6]
    for flip in (1, 0x1000):
        want = _host(engine, n, sizeL, nd, IDX, base, flip, PRESETS["strip"], lists=li)
        got = engine.montecarlo_trace_lists(n, nd, base, IDX, li, sizeL, cap=1024, flip_q16=flip,
                                            adversary=PRESETS["strip"])
        _same(got, want, f"noisy lists flip={flip:#x}")


def test_a_value_past_w_at_a_q_position_gives_status_4_and_no_events(engine):
    import torch
    mc = sub("montecarlo")
    case = next(c for c in HOSTILE if c["n"] == 3)
    n, nd, sizeL, base, w = 3, case["nDishonest"], case["sizeL"], case["base"], 4
    li = np.array(np.broadcast_to(hostile_lists(case)[0], (5, n + 1, sizeL)))
    q = int(np.nonzero(li[2, 0] != li[2, 1])[0][0])
    li[2, 2, q] = w
    out = tuple(torch.full(s, GUARD, dtype=torch.int32, device=engine.device)
                for s in ((5, 4 + 5 * (n + 1)), (5, n + 1), (5, n + 1, 64, 2)))
    rows, counts, events = engine.montecarlo_trace_lists(n, nd, base, list(range(5)), li, sizeL, cap=64, out=out)
    want = engine.montecarlo_lists(n, nd, base, li, sizeL, adversary=0xF).cpu().numpy()
    assert rows.cpu().numpy().tolist() == want.tolist()
    assert want[2].tolist() == [0, 0, 0, mc.ST_RANGE] + [0] * (5 * (n + 1))
    assert not counts[2].any() and (events[2] == GUARD).all()
    assert (counts[[0, 1, 3, 4], 1:] > 0).all()


def _guarded(engine, n, n_idx, cap, extra=64):
    """Three output tensors, each a view of the front of a GUARD-filled buffer
    with ``extra`` words behind it: (views, buffers)."""
    import torch
    shapes = ((n_idx, 4 + 5 * (n + 1)), (n_idx, n + 1), (n_idx, n + 1, cap, 2))
    bufs = [torch.full((int(np.prod(s)) + extra,), GUARD, dtype=torch.int32, device=engine.device) for s in shapes]
    return tuple(b[:int(np.prod(s))].view(s) for b, s in zip(bufs, shapes)), bufs


def test_cap_above_at_and_below_a_ranks_event_count(engine):
    n, nd, sizeL, word = 7, 2, 8, PRESETS["strip"]
    idx = [0, 1, 5]
    want = _host(engine, n, sizeL, nd, idx, 0xAD0, 0, word)
    c = int(want[1][1].max())          # the busiest rank of slot 1
    assert c > 4 and int(want[1][want[1] > 0].min()) < c - 1   # some ranks end below every cap used
    for cap in (c + 1, c, c - 1):
        out, bufs = _guarded(engine, n, len(idx), cap)
        got = engine.montecarlo_trace_sampled(n, nd, 0xAD0, idx, sizeL, cap=cap, adversary=word, out=out)
        _same(got, want, f"cap={cap}")
        counts, events = got[1].cpu().numpy(), got[2].cpu().numpy()
        for j in range(len(idx)):
            for r in range(n + 1):                      # behind each rank's stored events: untouched
                assert (events[j, r, min(int(counts[j, r]), cap):] == GUARD).all(), (cap, j, r)
        for b, t in zip(bufs, got):                     # behind the arrays: untouched
            assert (b[t.numel():] == GUARD).all()


def test_device_fed_match_count_limits_the_slots(engine):
    import torch
    n, nd, sizeL, word, n_idx = 7, 2, 8, PRESETS["reference"], 16
    idx = list(range(100, 100 + n_idx))
    want = _host(engine, n, sizeL, nd, idx, 0xAD0, 0, word)
    dev_idx = torch.tensor(idx, dtype=torch.int64, device=engine.device)
    for m in (0, 3, 1000):
        lim = min(m, n_idx)
        out, bufs = _guarded(engine, n, n_idx, CAP)
        n_match = torch.tensor([m], dtype=torch.int64, device=engine.device)
        got = engine.montecarlo_trace_sampled(n, nd, 0xAD0, dev_idx, sizeL, cap=CAP, adversary=word, n_match=n_match,
                                              out=out)
        _same(got, want, f"n_match={m}", slots=range(lim))
        for t, b in zip(got, bufs):
            assert (t[lim:] == GUARD).all() and (b[t.numel():] == GUARD).all(), m


def test_a_key_that_wraps_and_a_stream_of_its_own(engine):
    import torch
    n, nd, sizeL, word = 7, 2, 8, PRESETS["strip"]
    base, idx = MASK64 - 2, [0, 1, 2, 3, 4, 5]            # keys 2^64 - 3 .. 2^64 - 1, 0, 1, 2
    want = _host(engine, n, sizeL, nd, idx, base, 0x1000, word)
    again = _host(engine, n, sizeL, nd, [0, 1, 2], 0, 0x1000, word)
    assert want[0][3:].tolist() == again[0].tolist()
    s = torch.cuda.Stream(device=engine.device)
    with torch.cuda.stream(s):
        got = engine.montecarlo_trace_sampled(n, nd, base, idx, sizeL, cap=CAP, flip_q16=0x1000, adversary=word)
    s.synchronize()
    _same(got, want, "wrapped keys on a side stream")


E2E = dict(n=7, nd=2, sizeL=8, runs=300, seed=2768)


def test_run_with_failures_feeds_the_trace_from_the_capture_buffer(engine):
    mc = sub("montecarlo")
    n, nd, sizeL, runs, seed = (E2E[k] for k in ("n", "nd", "sizeL", "runs", "seed"))
    s = mc.run(n, sizeL, nd, runs, seed, engine, batch=128, path="fused", failures=4, explain=CAP)
    assert s["failed_total"] >= 4 and len(s["failed_runs"]) == 4
    want = _host(engine, n, sizeL, nd, s["failed_runs"], seed, 0, None)
    rows, counts, events = s["trace"]
    assert rows.tolist() == want[0].tolist() and counts.tolist() == want[1].tolist() and not rows[:, 0].any()
    for j in range(4):
        assert mc.trace_events(counts, events, j) == want[2][j]
    plain = mc.run(n, sizeL, nd, runs, seed, engine, batch=128, path="fused", failures=4)
    # more failures than slots: which four the capture keeps is up to the tally's atomics
    drop = ("trace", "failed_runs")
    assert {k: v for k, v in s.items() if k not in drop} == {k: v for k, v in plain.items() if k not in drop}


def _cli(argv, capsys):
    assert sub("tfg").main(argv) == 0
    return capsys.readouterr().out.splitlines()


@pytest.mark.parametrize("extra", [["--fused"], ["--curve", "50,100"], ["--sweep", "1,2:strip"]],
                         ids=["fused", "curve", "sweep"])
def test_cli_explain_prints_the_host_transcripts_of_the_printed_indices(engine, capsys, extra):
    mc = sub("montecarlo")
    n, nd, sizeL, runs, seed = (E2E[k] for k in ("n", "nd", "sizeL", "runs", "seed"))
    argv = [str(sizeL), str(nd), "--parties", str(n), "--runs", str(runs), "--seed", str(seed)] + extra
    lines = _cli(argv + ["--explain", "2"], capsys)
    # the lines of --failures 2, up to which two of the failed runs the capture kept
    cut = [l.split("): ")[0] for l in lines if l.startswith(("Runs:", "Failed runs"))]
    assert cut == [l.split("): ")[0] for l in _cli(argv + ["--failures", "2"], capsys)]
    at, seen = 0, 0
    while at < len(lines):
        head = re.match(r"Runs: .*sizeL=(\d+), dishonest=(\d+),.*?\)(?:.* adversary=(0x[0-9a-f]+))?", lines[at])
        assert head, lines[at]
        c, k, word = int(head.group(1)), int(head.group(2)), head.group(3)
        assert lines[at + 1].startswith("Failed runs (")
        failed = [int(x) for x in lines[at + 1].split("): ", 1)[1].split()]
        at += 2
        want = _host(engine, n, c, k, failed, seed, 0, None if word is None else int(word, 16))
        for j, i in enumerate(failed):
            text = [f"Run {i}:"] + mc.format_trace(n, want[0][j], want[1][j], want[2][j]).splitlines()
            assert lines[at:at + len(text)] == text, (c, k, word, i)
            at += len(text)
            seen += 1
    assert seen > 0
