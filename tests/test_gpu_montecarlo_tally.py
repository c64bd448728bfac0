"""qba_montecarlo_tally on the GPU: every tally word and the captured indices
against montecarlo.tally_host on the host copy of the same rows (never against
the device tally itself), on rows from all three Monte-Carlo paths, and
run / curve / the CLI with the tally against their row-copying forms."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, sub
from montecarlo_cases import HOSTILE, HOSTILE_IDS, SWEEP, SWEEP_IDS, hostile_lists
from montecarlo_tally_cases import synthetic_rows

pytestmark = pytest.mark.gpu

mc = sub("montecarlo")
COUNTS = [0, 1, 2, 3, 5, 63, 64, 65, 127, 130, 1000]   # the ladder of test_gpu_montecarlo_curve.py
INST, BASE = 67, 0xA11CE
ADDITIVE = [w for w in range(32) if w != 4]


def _nds(n):
    return sorted({min(max(d, 0), n) for d in (0, 1, n // 3, n - 1)})


def _torch():
    import torch
    return torch


def _check(engine, n, rows, inst_base=0, select=0, cap=None, what=""):
    """One call on device rows against tally_host on their host copy; the
    capture buffer holds every match when `cap` is None.  Returns the host
    tally."""
    torch = _torch()
    want, matches = mc.tally_host(n, rows.cpu().numpy(), inst_base, select)
    k = want.shape[0]
    if cap is None:
        cap = max(len(m) for m in matches) + 3
    capture = torch.full((k, cap), -7, dtype=torch.int64, device=engine.device) if select else None
    got = engine.montecarlo_tally(n, rows, inst_base=inst_base, select=select, capture=capture)
    assert got.dtype == torch.int64 and tuple(got.shape) == (k, 32)
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        j, w = np.argwhere(got != want)[0]
        raise AssertionError(f"{what} slice {j}, word {w}: {got[j, w]} != {want[j, w]}\n"
                             f"got  {got[j].tolist()}\nwant {want[j].tolist()}")
    if select:
        cp = capture.cpu().numpy()
        for j, m in enumerate(matches):
            kept = min(len(m), cap)
            assert np.all(cp[j, kept:] == -7), (what, j)
            if len(m) <= cap:
                assert sorted(cp[j, :kept].tolist()) == m, (what, j)
            else:
                assert len(set(cp[j].tolist())) == cap and set(cp[j].tolist()) <= set(m), (what, j)
    return want


# ---------------------------------------------------------------------------
# rows of the sampling kernels, every word
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 7, 11, 15])
def test_every_word_on_sampled_rows(engine, n):
    seen = np.zeros(32, np.int64)
    for nd in _nds(n):
        for size_l in (2, 8, 65):
            rows = engine.montecarlo_sampled(n, nd, BASE, INST, size_l)
            seen += _check(engine, n, rows, inst_base=BASE, select=mc.SEL_FAILED | mc.SEL_EMPTY_VI,
                           what=f"n={n} nd={nd} L={size_l}")[0]
    assert seen[mc.T_RUNS] == INST * 3 * len(_nds(n)) and seen[mc.T_STATUS_ROWS] == 0
    if n >= 3:
        assert 0 < seen[mc.T_SUCCESSES] < seen[mc.T_RUNS] and seen[mc.T_CMD_DISHONEST] > 0


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 256, 257, 4099])
def test_row_counts_around_tile_edges(engine, count):
    for n, nd in ((7, 2), (11, 3), (4, 1)):   # 44-, 64- and 29-word rows
        rows = engine.montecarlo_sampled(n, nd, 31 + count, count, 6)
        want = _check(engine, n, rows, inst_base=5, select=mc.SEL_FAILED, what=f"n={n} rows={count}")
        assert want[0, mc.T_RUNS] == count


def test_more_tiles_than_workgroups(engine):
    """Grid-stride: 20,011 rows of n = 3, and shapes with more tiles than the
    launch has workgroups for a slice (2048 over all slices, tiles of 64
    rows): one slice of 131,137 rows, 32 slices of 4,163."""
    torch = _torch()
    rows = engine.montecarlo_sampled(3, 1, 77, 20011, 7)
    want = _check(engine, 3, rows, inst_base=77, select=mc.SEL_FAILED)
    assert 0 < want[0, mc.T_SUCCESSES] < 20011
    one = torch.from_numpy(synthetic_rows(1, 2048 * 64 + 65, seed=5)).to(engine.device)
    _check(engine, 1, one, select=mc.SEL_STATUS, what="one slice:")
    many = np.stack([synthetic_rows(1, 64 * 64 + 67, seed=100 + j, status_every=5 + j) for j in range(32)])
    _check(engine, 1, torch.from_numpy(many).to(engine.device), select=mc.SEL_EMPTY_VI, cap=16, what="32 slices:")


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_hostile_and_sweep_rows(engine, case):
    rows = engine.montecarlo_lists(case["n"], case["nDishonest"], case["base"],
                                   np.ascontiguousarray(hostile_lists(case)), case["sizeL"])
    _check(engine, case["n"], rows, inst_base=case["base"], select=7, what=case["name"])


def test_hostile_rows_reach_empty_vi_and_the_minus_one_bin(engine):
    total = np.zeros(32, np.int64)
    for case in HOSTILE:
        rows = engine.montecarlo_lists(case["n"], case["nDishonest"], case["base"],
                                       np.ascontiguousarray(hostile_lists(case)), case["sizeL"])
        total += mc.tally_host(case["n"], rows.cpu().numpy())[0][0]
    assert total[mc.T_EMPTY_VI] > 0 and total[mc.T_DEC_NEG] > 0 and 0 < total[mc.T_SUCCESSES] < total[mc.T_RUNS]


# ---------------------------------------------------------------------------
# status rows
# ---------------------------------------------------------------------------
def test_range_status_rows_from_the_lists_kernel(engine):
    torch = _torch()
    case = next(c for c in HOSTILE if c["n"] == 3)
    n, nd, L, base, w = 3, case["nDishonest"], case["sizeL"], case["base"], 4
    li = np.array(np.broadcast_to(hostile_lists(case)[0], (16, n + 1, L)))
    k = int(np.nonzero(li[0, 0] != li[0, 1])[0][0])      # a Q-correlated position
    planted = [2, 7, 11]
    for i in planted:
        li[i, 2, k] = w
    rows = engine.montecarlo_lists(n, nd, base, li, L)
    host = rows.cpu().numpy()
    assert np.nonzero(host[:, 3])[0].tolist() == planted and set(host[planted, 3].tolist()) == {mc.ST_RANGE}
    capture = torch.full((1, 8), -7, dtype=torch.int64, device=engine.device)
    tally = engine.montecarlo_tally(n, rows, inst_base=base, select=mc.SEL_STATUS, capture=capture).cpu().numpy()[0]
    assert tally[mc.T_RUNS] == 16 and tally[mc.T_STATUS_ROWS] == 3 and tally[mc.T_STATUS_OR] == mc.ST_RANGE
    clean = np.delete(host, planted, 0)
    want = mc.tally_host(n, clean)[0][0]
    assert tally[mc.T_DEC0] == want[mc.T_DEC0]            # bin 16 holds the 13 live rows' zeros only
    assert np.array_equal(tally[mc.T_DEC_NEG:], want[mc.T_DEC_NEG:]) and tally[mc.T_DEC_NEG:].sum() <= 13 * n
    assert sorted(capture.cpu().numpy()[0, :3].tolist()) == [base + i for i in planted]
    assert tally[mc.T_CAPTURE] == 3 and np.all(capture.cpu().numpy()[0, 3:] == -7)
    _check(engine, n, rows, inst_base=base, select=7)


@pytest.mark.parametrize("n", [1, 3, 7, 11, 15])
def test_synthetic_rows_with_every_status_and_sums_past_32_bits(engine, n):
    torch = _torch()
    rows = torch.from_numpy(synthetic_rows(n, 301, seed=n)).to(engine.device)
    for sel in (0, 1, 2, 4, 7):
        want = _check(engine, n, rows, inst_base=(1 << 40) + 5, select=sel, what=f"n={n} select={sel}")
    assert want[0, mc.T_STATUS_OR] == 7 and want[0, mc.T_STATUS_ROWS] == 43 and want[0, mc.T_ACCEPT] > 1 << 32
    assert want[0, mc.T_CAPTURE] > 43


# ---------------------------------------------------------------------------
# accumulation, slices, capture, guards, streams
# ---------------------------------------------------------------------------
def test_calls_accumulate(engine):
    torch = _torch()
    n = 7
    rows = torch.from_numpy(synthetic_rows(n, 333, seed=9)).to(engine.device)
    want, matches = mc.tally_host(n, rows.cpu().numpy(), inst_base=50, select=7)
    tally = torch.zeros((1, 32), dtype=torch.int64, device=engine.device)
    capture = torch.full((1, 400), -7, dtype=torch.int64, device=engine.device)
    ret = engine.montecarlo_tally(n, rows[:100], tally, inst_base=50, select=7, capture=capture)
    assert ret.data_ptr() == tally.data_ptr()
    engine.montecarlo_tally(n, rows[100:], tally, inst_base=150, select=7, capture=capture)
    assert np.array_equal(tally.cpu().numpy(), want)
    m = len(matches[0])
    assert sorted(capture.cpu().numpy()[0, :m].tolist()) == matches[0] and np.all(capture.cpu().numpy()[0, m:] == -7)
    # the same block once more: every additive word doubles, the or stays
    engine.montecarlo_tally(n, rows, tally, inst_base=50, select=7, capture=capture)
    twice = tally.cpu().numpy()
    assert np.array_equal(twice[0, ADDITIVE], 2 * want[0, ADDITIVE]) and twice[0, 4] == want[0, 4]
    assert twice[0, 11:15].tolist() == [0, 0, 0, 0]
    # reserved words are left as the caller set them
    tally.fill_(1000)
    engine.montecarlo_tally(n, rows, tally)
    kept = tally.cpu().numpy()[0]
    assert kept[10:15].tolist() == [1000] * 5 and kept[0] == 1000 + 333


@pytest.mark.parametrize("counts", [[8], COUNTS, list(range(0, 64, 2))], ids=["K1", "K11", "K32"])
def test_slices_of_curve_output(engine, counts):
    n, nd = 7, 2
    out = engine.montecarlo_curve_sampled(n, nd, BASE, INST, counts)
    want = _check(engine, n, out, inst_base=BASE, select=mc.SEL_FAILED, what=f"K={len(counts)}")
    for j in range(len(counts)):
        one = engine.montecarlo_tally(n, out[j]).cpu().numpy()
        assert np.array_equal(one[0, ADDITIVE[:9]], want[j, ADDITIVE[:9]]) and np.array_equal(one[0, 15:], want[j, 15:])
        assert one[0, mc.T_CAPTURE] == 0
    if len(counts) > 1:
        assert len({want[j].tobytes() for j in range(len(counts))}) > 1


def test_capture_above_and_below_the_number_of_matches(engine):
    torch = _torch()
    n, base = 7, (1 << 40) + 5
    rows = engine.montecarlo_sampled(n, 2, 4242, 1000, 4)
    want, matches = mc.tally_host(n, rows.cpu().numpy(), base, mc.SEL_FAILED)
    m = len(matches[0])
    assert 70 < m < 1000 and min(matches[0]) > 1 << 40
    _check(engine, n, rows, inst_base=base, select=mc.SEL_FAILED, cap=m + 10, what="above:")
    _check(engine, n, rows, inst_base=base, select=mc.SEL_FAILED, cap=m, what="equal:")
    for cap in (1, 5, 64, m - 1):
        _check(engine, n, rows, inst_base=base, select=mc.SEL_FAILED, cap=cap, what=f"cap={cap}:")
    # select = 0 or cap = 0: the buffer is not touched
    capture = torch.full((1, 16), -7, dtype=torch.int64, device=engine.device)
    t0 = engine.montecarlo_tally(n, rows, inst_base=base, select=0, capture=capture).cpu().numpy()
    assert np.all(capture.cpu().numpy() == -7) and t0[0, mc.T_CAPTURE] == 0
    none = torch.zeros((1, 0), dtype=torch.int64, device=engine.device)
    for cp in (none, None):
        t1 = engine.montecarlo_tally(n, rows, inst_base=base, select=mc.SEL_FAILED, capture=cp).cpu().numpy()
        assert t1[0, mc.T_CAPTURE] == m and np.array_equal(t1, want)


def test_guard_words_and_argument_checks(engine):
    torch = _torch()
    QbaError = sub("_lib").QbaError
    n, k, cap, guard, fill = 7, 3, 4, 64, -0x5A5A5A5A5A5A5A5B
    out = engine.montecarlo_curve_sampled(n, 2, BASE, 200, [2, 4, 9])
    want, matches = mc.tally_host(n, out.cpu().numpy(), 9, mc.SEL_FAILED)
    assert all(len(m) > cap for m in matches)
    tbuf = torch.full((guard + k * 32 + guard,), fill, dtype=torch.int64, device=engine.device)
    cbuf = torch.full((guard + k * cap + guard,), fill, dtype=torch.int64, device=engine.device)
    tally, capture = tbuf[guard:guard + k * 32].view(k, 32), cbuf[guard:guard + k * cap].view(k, cap)
    tally.zero_()
    engine.montecarlo_tally(n, out, tally, inst_base=9, select=mc.SEL_FAILED, capture=capture)
    for buf in (tbuf, cbuf):
        flat = buf.cpu().numpy()
        assert np.all(flat[:guard] == fill) and np.all(flat[-guard:] == fill)
    assert np.array_equal(tally.cpu().numpy(), want)
    for j in range(k):
        got = capture.cpu().numpy()[j].tolist()
        assert len(set(got)) == cap and set(got) <= set(matches[j])
    new = lambda *shape, dtype=torch.int64, device=engine.device: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    words = 4 + 5 * (n + 1)
    for bad in (out.to(torch.int64), out[:, :, :-1], out[:, ::2], out.cpu(), out[0, 0], new(33, 1, words, dtype=torch.int32)):
        with pytest.raises(QbaError):
            engine.montecarlo_tally(n, bad)
    for bad in (new(k, 31), new(k + 1, 32), new(k, 32, dtype=torch.int32), new(k, 32, device="cpu"), new(k, 64)[:, ::2]):
        with pytest.raises(QbaError):
            engine.montecarlo_tally(n, out, bad)
    for bad in (new(k + 1, cap), new(k * cap), new(k, cap, dtype=torch.int32), new(k, cap, device="cpu"),
                new(k, 2 * cap)[:, ::2]):
        with pytest.raises(QbaError):
            engine.montecarlo_tally(n, out, select=1, capture=bad)
    for sel in (-1, 8):
        with pytest.raises(QbaError):
            engine.montecarlo_tally(n, out, select=sel)
    assert engine.montecarlo_tally(n, out[:, :0].contiguous()).cpu().numpy().tolist() == [[0] * 32] * k


def test_non_default_stream(engine):
    torch = _torch()
    n = 11
    rows = engine.montecarlo_sampled(n, 3, BASE, 500, 6)
    want, matches = mc.tally_host(n, rows.cpu().numpy(), 3, mc.SEL_FAILED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        capture = torch.zeros((1, 500), dtype=torch.int64, device=engine.device)
        got = engine.montecarlo_tally(n, rows, inst_base=3, select=mc.SEL_FAILED, capture=capture)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert sorted(capture.cpu().numpy()[0, :len(matches[0])].tolist()) == matches[0]


# ---------------------------------------------------------------------------
# run, curve and the CLI
# ---------------------------------------------------------------------------
def _rows_of(engine, n, nd, size_l, runs, seed):
    return engine.montecarlo_sampled(n, nd, seed, runs, size_l).cpu().numpy()


@pytest.mark.parametrize("path", ["tables", "fused"])
def test_run_with_tally_agrees_with_run(engine, path):
    n, nd, size_l, runs, seed = 7, 2, 6, 300, 2024
    plain = mc.run(n, size_l, nd, runs, seed, engine, batch=128, path=path)
    got = mc.run(n, size_l, nd, runs, seed, engine, batch=128, path=path, tally=True)
    assert {k: got[k] for k in plain} == plain and "failed_runs" not in got
    fails = np.nonzero(_rows_of(engine, n, nd, size_l, runs, seed)[:, 0] == 0)[0].tolist()
    assert 10 < len(fails) < runs
    full = mc.run(n, size_l, nd, runs, seed, engine, batch=128, path=path, failures=runs)
    assert full["failed_runs"] == fails and full["failed_total"] == len(fails)
    assert {k: full[k] for k in plain} == plain
    few = mc.run(n, size_l, nd, runs, seed, engine, batch=128, path=path, failures=5)
    assert few["failed_total"] == len(fails) and len(few["failed_runs"]) == 5
    assert few["failed_runs"] == sorted(set(few["failed_runs"])) and set(few["failed_runs"]) <= set(fails)
    assert mc.run(n, size_l, nd, 0, seed, engine, path=path, tally=True)["runs"] == 0


def test_curve_with_tally_agrees_with_curve(engine):
    n, nd, runs, seed, counts = 7, 2, 300, 2024, [2, 6, 40]
    plain = mc.curve(n, counts, nd, runs, seed, engine, batch=128)
    got = mc.curve(n, counts, nd, runs, seed, engine, batch=128, tally=True, failures=runs)
    assert list(got) == counts
    for c in counts:
        assert {k: got[c][k] for k in plain[c]} == plain[c], c
        fails = np.nonzero(_rows_of(engine, n, nd, c, runs, seed)[:, 0] == 0)[0].tolist()
        assert got[c]["failed_runs"] == fails and got[c]["failed_total"] == len(fails), c
    assert got[2]["failed_total"] > got[40]["failed_total"]


def test_cli_tally_and_failures(engine):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "tfg---quantum-byzantine-agreement_amd.tfg", "6", "2", "--parties", "7", "--runs",
            "300", "--seed", "2024", "--batch", "128", "--fused"]

    def lines(extra):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        return out.stdout.splitlines()

    plain = [l for l in lines([]) if l.startswith("Runs:")]
    assert len(plain) == 1 and [l for l in lines(["--tally"]) if l.startswith("Runs:")] == plain
    out = lines(["--failures", "5"])
    assert [l for l in out if l.startswith("Runs:")] == plain
    failed = [l for l in out if l.startswith("Failed runs")]
    assert len(failed) == 1
    head, _, tail = failed[0].partition("): ")
    total = 300 - int(plain[0].split()[3])
    assert head == f"Failed runs (5 of {total}, key = seed + index, seed=2024" and total > 5
    idx = [int(x) for x in tail.split()]
    assert len(idx) == 5 and idx == sorted(set(idx)) and all(0 <= i < 300 for i in idx)
    for i in idx:   # replayed alone under key seed + index
        assert engine.montecarlo_sampled(7, 2, 2024 + i, 1, 6).cpu().numpy()[0, 0] == 0
    bad = subprocess.run(base[:5] + ["--failures", "3"], capture_output=True, text=True, timeout=300, env=env,
                         cwd=str(ROOT))
    assert bad.returncode == 2 and "--runs" in bad.stderr
