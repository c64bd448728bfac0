"""The sizeL-curve Monte-Carlo calls on the GPU: slice j of
qba_montecarlo_curve_sampled / qba_montecarlo_curve_lists is, in every word of
every instance, the row block the single-count call writes at counts[j].  The
reference is always the existing single-count entry point (montecarlo_sampled,
montecarlo_lists) or the host specification, never the curve calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, sub
from montecarlo_cases import HOSTILE, HOSTILE_IDS, SWEEP, SWEEP_IDS, hostile_lists
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 7, 11, 12, 15]
# an empty first segment; checkpoints that split a pair (odd); two and three
# inside one wave-step; adjacent ones across a wave-step edge (63, 64, 65;
# 127 | 130); more than two wave-steps in one segment (130 -> 1000)
COUNTS = [0, 1, 2, 3, 5, 63, 64, 65, 127, 130, 1000]
GRID_INST, GRID_BASE = 67, 0xA11CE


def _nds(n):
    """{0, 1, n // 3, n - 1}, as the grid of the single-count tests."""
    return sorted({min(max(d, 0), n) for d in (0, 1, n // 3, n - 1)})


GRID = [(n, nd) for n in NS for nd in _nds(n)]


def _eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.int32, (got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        i, j = np.argwhere(got != want)[0]
        raise AssertionError(f"{what} instance {i}, word {j}: {got[i, j]} != {want[i, j]}\n"
                             f"got  {got[i].tolist()}\nwant {want[i].tolist()}")


def _eq_slices(got, want_of, counts, what=""):
    got = np.asarray(got)
    assert got.ndim == 3 and got.shape[0] == len(counts)
    for j, c in enumerate(counts):
        _eq(got[j], want_of(c), f"{what} checkpoint {j} (count {c}):")


@pytest.fixture(scope="module")
def single(engine):
    """montecarlo_sampled rows, computed once per (n, nd, base, inst, count)."""
    memo = {}

    def get(n, nd, base, inst, count):
        key = (n, nd, base, inst, count)
        if key not in memo:
            rows = engine.montecarlo_sampled(n, nd, base, inst, count).cpu().numpy()
            rows.setflags(write=False)
            memo[key] = rows
        return memo[key]
    return get


@pytest.mark.parametrize("n,nd", GRID, ids=[f"n{n}-d{d}" for n, d in GRID])
def test_sampled_form_equals_the_single_count_call_at_every_checkpoint(engine, single, n, nd):
    got = engine.montecarlo_curve_sampled(n, nd, GRID_BASE, GRID_INST, COUNTS).cpu().numpy()
    assert got.shape == (len(COUNTS), GRID_INST, 4 + 5 * (n + 1))
    _eq_slices(got, lambda c: single(n, nd, GRID_BASE, GRID_INST, c), COUNTS, f"n={n} nd={nd}")
    assert not got[:, :, 3].any()


def test_expected_rows_differ_between_checkpoints_and_hold_both_outcomes(single):
    """About the inputs, not the kernel: the reference rows must tell slices apart."""
    ok = total = 0
    for n, nd in GRID:
        rows = [single(n, nd, GRID_BASE, GRID_INST, c) for c in COUNTS]
        # with no traitor, or fewer than two lieutenants, a row does not depend on the
        # lists (montecarlo.run_host gives one and the same slice at every count)
        if 3 <= n <= 11 and nd >= 1:
            assert len({r.tobytes() for r in rows}) >= 2, (n, nd)   # at least two slices differ
        ok += sum(int(r[:, 0].sum()) for r in rows)
        total += sum(len(r) for r in rows)
    assert 0 < ok < total


def test_one_checkpoint_equals_the_single_count_call(engine, single):
    for n, nd, c in ((7, 2, 100), (11, 3, 65), (12, 4, 0), (3, 1, 1)):
        got = engine.montecarlo_curve_sampled(n, nd, GRID_BASE, GRID_INST, [c]).cpu().numpy()
        assert got.shape[0] == 1
        _eq(got[0], single(n, nd, GRID_BASE, GRID_INST, c), f"n={n} count={c}:")


@pytest.mark.parametrize("n,nd", [(7, 2), (12, 4)])
def test_thirty_two_checkpoints(engine, single, n, nd):
    counts = list(range(0, 64, 2))
    assert len(counts) == 32
    got = engine.montecarlo_curve_sampled(n, nd, GRID_BASE, GRID_INST, counts).cpu().numpy()
    _eq_slices(got, lambda c: single(n, nd, GRID_BASE, GRID_INST, c), counts, f"n={n}")
    QbaError = sub("_lib").QbaError
    with pytest.raises(QbaError):
        engine.montecarlo_curve_sampled(n, nd, GRID_BASE, GRID_INST, list(range(33)))


def test_more_instances_than_resident_wave_slots(engine, single):
    n, nd, inst, base, counts = 3, 1, 20011, 77, [7, 33]
    got = engine.montecarlo_curve_sampled(n, nd, base, inst, counts).cpu().numpy()
    _eq_slices(got, lambda c: single(n, nd, base, inst, c), counts)
    assert 0 < got[1, :, 0].sum() < inst


def test_key_wraps_mod_2_64(engine, single):
    n, nd, inst, base, counts = 7, 2, 8, (1 << 64) - 3, [1, 50, 100]
    got = engine.montecarlo_curve_sampled(n, nd, base, inst, counts).cpu().numpy()
    _eq_slices(got, lambda c: single(n, nd, base, inst, c), counts)
    _eq_slices(got[:, 3:], lambda c: single(n, nd, 0, inst - 3, c), counts, "keys 0..:")


def _list_counts(L):
    assert L >= 1
    return sorted({0, 1, L // 3, (L // 2) | 1, L - 1, L})


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_lists_form_equals_the_single_count_call_and_host_on_hostile_lists(engine, case):
    import torch
    mc = sub("montecarlo")
    n, nd, L, keys, base = case["n"], case["nDishonest"], case["sizeL"], case["keys"], case["base"]
    li = np.ascontiguousarray(hostile_lists(case))
    dev = torch.from_numpy(li).to(engine.device)
    counts = _list_counts(L)
    got = engine.montecarlo_curve_lists(n, nd, base, dev, counts).cpu().numpy()
    _eq_slices(got, lambda c: engine.montecarlo_lists(n, nd, base, dev, c).cpu().numpy(), counts, "lists:")
    assert not got[:, :, 3].any()
    if n <= 11:
        want = mc.curve_host(n, counts, nd, keys, base, OracleEngine(), lists=li)
        _eq_slices(got, lambda c: want[counts.index(c)], counts, "host:")
    # a host array is taken as montecarlo_lists takes it
    _eq(engine.montecarlo_curve_lists(n, nd, base, li, counts[-2:]).cpu().numpy()[1], got[-1])


def test_lists_form_on_the_devices_own_sampled_rows(engine, single):
    n, nd, L, base, inst = 7, 2, 200, 3000, 32
    lists, _ = engine.sample_check_batched(n, base, inst, L)   # rows 4 KiB apart, as sampled
    counts = _list_counts(L)
    got = engine.montecarlo_curve_lists(n, nd, base, lists, counts).cpu().numpy()
    _eq_slices(got, lambda c: engine.montecarlo_lists(n, nd, base, lists, c).cpu().numpy(), counts, "lists:")
    _eq_slices(got, lambda c: single(n, nd, base, inst, c), counts, "sampled:")
    _eq_slices(engine.montecarlo_curve_sampled(n, nd, base, inst, counts).cpu().numpy(),
               lambda c: got[counts.index(c)], counts, "curve sampled:")


def test_lists_form_second_launch_chunk(engine):
    """More than 2^20 instances: the second launch of qba_montecarlo_curve_lists,
    where the kernel adds its chunk's first instance to blockIdx.x.  Row i of
    a slice depends on key base + i and instance i's lists alone, so the rows
    across the chunk boundary are those of a small call from there on."""
    import torch
    n, nd, counts, base = 2, 1, [2, 4], 0xC0FFEE
    cut, inst = 2**20 - 2, 2**20 + 3
    gen = torch.Generator(device=engine.device).manual_seed(20)
    lists = torch.randint(0, 4, (inst, n + 1, counts[-1]), dtype=torch.uint8, device=engine.device, generator=gen)
    big = engine.montecarlo_curve_lists(n, nd, base, lists, counts)[:, cut:].cpu().numpy()
    small = engine.montecarlo_curve_lists(n, nd, base + cut, lists[cut:], counts).cpu().numpy()
    _eq_slices(big, lambda c: small[counts.index(c)], counts)
    assert not big[:, :, 3].any()
    for rows in big:
        assert any(not np.array_equal(rows[0], r) for r in rows[1:])


def test_range_status_from_the_checkpoint_after_the_plant_on(engine):
    mc = sub("montecarlo")
    case = next(c for c in HOSTILE if c["n"] == 3)
    n, nd, L, base = 3, case["nDishonest"], case["sizeL"], case["base"]
    w = 4
    li = np.array(np.broadcast_to(hostile_lists(case)[0], (5, n + 1, L)))
    li[:, 0, 0] = li[:, 1, 0]                        # entry 0 is not Q-correlated in every instance
    qs = np.nonzero(li[2, 0] != li[2, 1])[0]
    k = int(qs[len(qs) // 2])                        # a Q-correlated entry of instance 2, checkpoints on both sides
    counts = sorted({1, k, k + 1, k + 2, L} - {0})
    assert 0 < k < L - 1 and counts.index(k) + 1 == counts.index(k + 1)
    clean = engine.montecarlo_curve_lists(n, nd, base, li, counts).cpu().numpy()
    _eq_slices(clean, lambda c: engine.montecarlo_lists(n, nd, base, li, c).cpu().numpy(), counts, "clean:")
    assert not clean[:, :, 3].any()
    bad = li.copy()
    bad[2, 2, k] = w
    rows = engine.montecarlo_curve_lists(n, nd, base, bad, counts).cpu().numpy()
    flagged = [0, 0, 0, mc.ST_RANGE] + [0] * (5 * (n + 1))
    for j, c in enumerate(counts):
        if c > k:
            assert rows[j, 2].tolist() == flagged, c
            _eq(np.delete(rows[j], 2, 0), np.delete(clean[j], 2, 0), f"count {c}:")
        else:
            _eq(rows[j], clean[j], f"count {c}:")
        _eq(rows[j], engine.montecarlo_lists(n, nd, base, bad, c).cpu().numpy(), f"single, count {c}:")
    assert [c > k for c in counts].count(True) >= 2 and [c > k for c in counts].count(False) >= 2
    for g in (2, 3):                                 # the same value where L0 == L1 changes nothing
        off = li.copy()
        off[2, g, 0] = w
        _eq_slices(engine.montecarlo_curve_lists(n, nd, base, off, counts).cpu().numpy(),
                   lambda c: clean[counts.index(c)], counts, "not-Q plant:")


def test_out_is_written_in_its_words_only_and_checked(engine, single):
    import torch
    QbaError = sub("_lib").QbaError
    n, nd, inst, base, counts = 7, 2, 37, 99, [0, 3, 70]
    words, k = 4 + 5 * (n + 1), 3
    fill, guard = 0x5A5A5A5A, 64
    lists, _ = engine.sample_check_batched(n, base, inst, counts[-1])

    def sampled(o=None):
        return engine.montecarlo_curve_sampled(n, nd, base, inst, counts, out=o)

    def from_lists(o=None):
        return engine.montecarlo_curve_lists(n, nd, base, lists, counts, out=o)

    new = lambda *shape, dtype=torch.int32, device=engine.device: \
        torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    for run in (sampled, from_lists):
        buf = torch.full((guard + k * inst * words + guard,), fill, dtype=torch.int32, device=engine.device)
        out = buf[guard:guard + k * inst * words].view(k, inst, words)
        ret = run(out)
        assert ret.data_ptr() == out.data_ptr()
        flat = buf.cpu().numpy()
        assert np.all(flat[:guard] == fill) and np.all(flat[-guard:] == fill)
        rows = out.cpu().numpy()
        assert not np.any(rows == fill)
        _eq_slices(rows, lambda c: single(n, nd, base, inst, c), counts)
        for bad in (new(k, inst, words, dtype=torch.int64), new(k, inst, words, dtype=torch.float32),
                    new(k + 1, inst, words), new(k, inst + 1, words), new(k, inst, words + 1),
                    new(k * inst, words), new(k, inst, words, device="cpu"), new(k, inst, 2 * words)[:, :, ::2],
                    new(inst, k, words).transpose(0, 1)):
            with pytest.raises(QbaError):
                run(bad)
        _eq_slices(run().cpu().numpy(), lambda c: single(n, nd, base, inst, c), counts)
    for bad in (lists.cpu(), lists.to(torch.int32), lists[:, :-1], lists[:, :, :counts[-1] - 1], lists[0]):
        with pytest.raises(QbaError):
            engine.montecarlo_curve_lists(n, nd, base, bad, counts)
    for bad in ([3, 3], [5, 4], [], [1 << 31], [-1, 5]):
        with pytest.raises(QbaError):
            engine.montecarlo_curve_sampled(n, nd, base, inst, bad)
    with pytest.raises(QbaError):
        engine.montecarlo_curve_sampled(n, n + 1, base, inst, counts)
    assert tuple(engine.montecarlo_curve_sampled(n, nd, base, 0, counts).shape) == (k, 0, words)


def test_non_default_stream(engine, single):
    import torch
    n, nd, base, counts = 7, 2, 31337, [5, 50, 64]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = engine.montecarlo_curve_sampled(n, nd, base, GRID_INST, counts)
        lists, _ = engine.sample_check_batched(n, base, GRID_INST, counts[-1])
        got_l = engine.montecarlo_curve_lists(n, nd, base, lists, counts)
    side.synchronize()
    _eq_slices(got.cpu().numpy(), lambda c: single(n, nd, base, GRID_INST, c), counts)
    _eq_slices(got_l.cpu().numpy(), lambda c: single(n, nd, base, GRID_INST, c), counts, "lists:")


def test_curve_summaries_equal_run_fused_across_a_batch_split(engine):
    mc = sub("montecarlo")
    n, nd, seed, counts = 7, 2, 31337, [4, 17, 50]
    got = mc.curve(n, counts, nd, 100, seed, engine, batch=32)
    assert list(got) == counts
    for c in counts:
        assert got[c] == mc.run(n, c, nd, 100, seed, engine, batch=32, path="fused"), c
        assert got[c]["runs"] == 100
    assert got == mc.curve(n, counts, nd, 100, seed, engine)


def test_cli_curve_prints_the_lines_of_the_separate_fused_runs():
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "tfg---quantum-byzantine-agreement_amd.tfg"]
    tail = ["2", "--parties", "7", "--runs", "300", "--seed", "2024"]

    def lines(cmd):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        return [l for l in out.stdout.splitlines() if l.startswith("Runs:")]

    curve = lines(base + ["50"] + tail + ["--curve", "200,16"])
    assert len(curve) == 3 and all("Runs: 300 Successes:" in l for l in curve)
    assert ["sizeL=16," in curve[0], "sizeL=50," in curve[1], "sizeL=200," in curve[2]] == [True] * 3
    assert curve[1:2] == lines(base + ["50"] + tail + ["--fused"])
    assert curve[2:3] == lines(base + ["200"] + tail + ["--fused"])
