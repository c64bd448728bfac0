"""The scenario sweep on the GPU.  Every comparison is
exact.  The reference is always the call that existed before -- slice (j, s)
of a sweep against montecarlo_curve_sampled / montecarlo_curve_lists with
``adversary=`` and that scenario's n_dishonest -- or the host model
montecarlo.sweep_host where the C twin samples (n <= 11)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, sub
from montecarlo_cases import HOSTILE, HOSTILE_IDS, SWEEP, SWEEP_IDS, hostile_lists
from test_montecarlo_adversary import HostEngine, PRESETS

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 7, 11, 12, 15]
COUNTS = [0, 3, 65, 130]
FLIPS = [0, 1, 0x1000]
INST, BASE = 67, 0xADA11CE
REFERENCE, LOW, STRIP, RELAY = 0xF, PRESETS["reorder_low"], PRESETS["strip"], PRESETS["relay"]


def _eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        at = tuple(np.argwhere(got != want)[0].tolist())
        raise AssertionError(f"{what} first difference at {at}: {got[at]} != {want[at]}\n"
                             f"got  {got[at[:-1]].tolist()}\nwant {want[at[:-1]].tolist()}")


def _grid(n):
    """The basic grid's scenarios, n_dishonest clipped to [0, n]."""
    clip = lambda k: min(max(k, 0), n)  # noqa: E731
    return [(0, REFERENCE), (clip(1), REFERENCE), (clip(n // 3), LOW), (clip(n - 1), STRIP), (n, RELAY)]


def _separate(engine, n, base, inst, counts, scen, flip=0):
    """The sweep's rows from one montecarlo_curve_sampled call per scenario,
    [len(counts), len(scen), inst, words]."""
    memo = {}
    for k, word in scen:
        if (k, word) not in memo:
            memo[k, word] = engine.montecarlo_curve_sampled(n, k, base, inst, counts, flip_q16=flip,
                                                            adversary=word).cpu().numpy()
    return np.stack([memo[s] for s in scen], axis=1)


@pytest.fixture(scope="module")
def basic():
    """(n, flip) -> the separate calls' rows of the basic grid, computed once and read-only."""
    memo = {}

    def get(engine, n, flip):
        if (n, flip) not in memo:
            memo[n, flip] = _separate(engine, n, BASE, INST, COUNTS, _grid(n), flip)
            memo[n, flip].setflags(write=False)
        return memo[n, flip]
    return get


@pytest.mark.parametrize("flip", FLIPS, ids=[f"flip{k:#x}" for k in FLIPS])
@pytest.mark.parametrize("n", NS)
def test_sampled_form_equals_the_curve_adv_call_of_every_scenario(engine, basic, n, flip):
    scen = _grid(n)
    want = basic(engine, n, flip)
    got = engine.montecarlo_sweep_sampled(n, BASE, INST, COUNTS, scen, flip_q16=flip).cpu().numpy()
    _eq(got, want, f"n={n} flip={flip:#x}:")
    assert not got[..., 3].any()
    if n >= 3:   # not vacuous: the scenarios and the checkpoints give different rows
        assert not np.array_equal(got[-1, 0], got[-1, 3]) and not np.array_equal(got[0, 3], got[-1, 3])
    if n <= 11 and flip != 1:   # the host model on the first instances (flip = 1 is covered by the calls above)
        few = 5
        _eq(got[:, :, :few], sub("montecarlo").sweep_host(n, COUNTS, scen, few, BASE, HostEngine(), flip_q16=flip),
            f"host n={n} flip={flip:#x}:")


@pytest.mark.parametrize("n", [3, 7, 12])
def test_no_state_leaks_between_scenarios(engine, basic, n):
    """The same scenarios reversed, and with the largest n_dishonest (the most
    rounds, the fullest mailbox) first: the slices come out permuted.  One
    scenario at positions 0 and 15 gives equal slices."""
    scen = _grid(n)
    want = basic(engine, n, 0)
    for order in (list(range(len(scen)))[::-1], sorted(range(len(scen)), key=lambda s: -scen[s][0])):
        got = engine.montecarlo_sweep_sampled(n, BASE, INST, COUNTS, [scen[s] for s in order]).cpu().numpy()
        _eq(got, want[:, order], f"order {order}:")
    cps = COUNTS[1:3]
    sixteen = [scen[3]] + [scen[s % 5] for s in range(14)] + [scen[3]]
    got = engine.montecarlo_sweep_sampled(n, BASE, INST, cps, sixteen).cpu().numpy()
    _eq(got[:, 0], got[:, 15], "positions 0 and 15:")
    _eq(got[:, 15], want[1:3, 3], "position 15:")


def test_bounds_sixteen_by_two_one_by_thirty_two_and_one_by_one(engine):
    n, base, inst = 7, 0x5EED5, 33
    scen = [(k % (n + 1), w) for k, w in zip(range(16), [REFERENCE, LOW, STRIP, RELAY, PRESETS["mute"]] * 4)]
    assert len(set(scen)) == 16
    cps = [3, 65]
    _eq(engine.montecarlo_sweep_sampled(n, base, inst, cps, scen).cpu().numpy(),
        _separate(engine, n, base, inst, cps, scen), "16 x 2:")
    cps = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 64, 65, 66, 89, 100, 127, 128, 129, 130, 144, 160, 191, 192, 193, 200,
           233, 255, 256, 257, 300, 377]
    assert len(cps) == 32
    for flip in (0, 0x1000):
        _eq(engine.montecarlo_sweep_sampled(n, base, inst, cps, [(3, STRIP)], flip_q16=flip).cpu().numpy(),
            _separate(engine, n, base, inst, cps, [(3, STRIP)], flip), f"1 x 32 flip={flip:#x}:")
    for count in (0, 1, 65):
        one = engine.montecarlo_sweep_sampled(n, base, inst, [count], [(2, LOW)]).cpu().numpy()
        assert one.shape[:2] == (1, 1)
        _eq(one[0, 0], engine.montecarlo_sampled(n, 2, base, inst, count, adversary=LOW).cpu().numpy(), "1 x 1:")
    QbaError = sub("_lib").QbaError
    for counts, sc in (([3, 65, 130], [(1, LOW)] * 11), ([3], [(1, LOW)] * 17), ([3], []), ([3], [(n + 1, LOW)])):
        with pytest.raises(QbaError):
            engine.montecarlo_sweep_sampled(n, base, inst, counts, sc)


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_lists_form_on_hostile_and_sweep_sets(engine, case):
    import torch
    mc = sub("montecarlo")
    n, nd, L, keys, base = case["n"], case["nDishonest"], case["sizeL"], case["keys"], case["base"]
    li = np.ascontiguousarray(hostile_lists(case))
    dev = torch.from_numpy(li).to(engine.device)
    counts = sorted({0, 1, L // 3, L})
    scen = [(nd, REFERENCE), (nd, LOW), (0, STRIP)]
    got = engine.montecarlo_sweep_lists(n, base, dev, counts, scen).cpu().numpy()
    assert got.shape == (len(counts), len(scen), keys, mc.out_words(n))
    for s, (k, word) in enumerate(scen):
        _eq(got[:, s], engine.montecarlo_curve_lists(n, k, base, dev, counts, adversary=word).cpu().numpy(),
            f"scenario {s} against curve_lists_adv:")
    assert not got[..., 3].any()
    if n <= 11:
        _eq(got, mc.sweep_host(n, counts, scen, keys, base, HostEngine(), lists=li), "host:")
    # a value >= w planted at a Q-correlated position k_pos of one instance: status 4 in exactly the
    # slices with counts[j] > k_pos, under every scenario, and every other row as it was
    at, w = keys // 2, 1 << mc._nq(n)
    qs = np.nonzero(li[at, 0] != li[at, 1])[0]
    k_pos = int(qs[len(qs) // 2])
    bad = li.copy()
    bad[at, 1, k_pos] = w
    rows = engine.montecarlo_sweep_lists(n, base, bad, counts, scen).cpu().numpy()
    flagged = [0, 0, 0, mc.ST_RANGE] + [0] * (5 * (n + 1))
    for j, c in enumerate(counts):
        for s in range(len(scen)):
            if c > k_pos:
                assert rows[j, s, at].tolist() == flagged, (c, s)
            else:
                assert rows[j, s, at, 3] == 0, (c, s)
    keep = np.arange(keys) != at
    _eq(rows[:, :, keep], got[:, :, keep], "the other instances:")
    below = [j for j, c in enumerate(counts) if c <= k_pos]
    _eq(rows[below], got[below], "checkpoints up to the plant:")
    assert below and len(below) < len(counts)


def test_lists_form_on_the_devices_own_sampled_rows_equals_the_sampled_form(engine):
    n, base, inst, counts = 7, 3000, 32, [0, 1, 66, 200]
    scen = _grid(n)
    lists, _ = engine.sample_check_batched(n, base, inst, counts[-1])   # rows 4 KiB apart, as sampled
    _eq(engine.montecarlo_sweep_lists(n, base, lists, counts, scen).cpu().numpy(),
        engine.montecarlo_sweep_sampled(n, base, inst, counts, scen).cpu().numpy(), "lists against sampled:")


# ---- launch and buffer edges, once each ------------------------------------------
def test_more_instances_than_resident_wave_slots(engine):
    n, inst, base, cps = 3, 20011, 0xAD0, [3, 8]
    scen = [(2, REFERENCE), (3, LOW), (1, STRIP)]
    got = engine.montecarlo_sweep_sampled(n, base, inst, cps, scen).cpu().numpy()
    _eq(got, _separate(engine, n, base, inst, cps, scen), "20,011 instances:")
    mc = sub("montecarlo")
    _eq(got[:, :, -6:], mc.sweep_host(n, cps, scen, 6, base + inst - 6, HostEngine()), "host, last:")


def test_past_the_resident_waves_at_n11(engine):
    import torch
    n, base, cps = 11, 0xAD0, [3, 8]
    scen = [(3, LOW), (0, REFERENCE), (10, STRIP)]
    engine.prepare(n)
    sh = engine.montecarlo_program_shape(n, curve=True)
    assert (sh["waves_run"], sh["lds_bytes"], sh["wgs_per_cu"]) == engine.montecarlo_curve_shape(n)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    inst = cus * sh["wgs_per_cu"] * sh["waves_run"] + 2 * sh["waves_run"] + 1
    got = engine.montecarlo_sweep_sampled(n, base, inst, cps, scen).cpu().numpy()
    _eq(got, _separate(engine, n, base, inst, cps, scen), "past the resident waves:")
    _eq(got[:, :, -4:], sub("montecarlo").sweep_host(n, cps, scen, 4, base + inst - 4, HostEngine()), "host, last:")


def test_key_wraps_mod_2_64(engine):
    mc = sub("montecarlo")
    n, inst, base, cps, k = 7, 8, (1 << 64) - 3, [3, 8], 0x1000
    scen = [(2, LOW), (6, STRIP)]
    got = engine.montecarlo_sweep_sampled(n, base, inst, cps, scen, flip_q16=k).cpu().numpy()
    _eq(got, mc.sweep_host(n, cps, scen, inst, base, HostEngine(), flip_q16=k), "host:")
    _eq(got[:, :, 3:], engine.montecarlo_sweep_sampled(n, 0, inst - 3, cps, scen, flip_q16=k).cpu().numpy(),
        "keys 0..4:")
    lists, _ = engine.sample_check_batched(n, base & ((1 << 64) - 1), inst, cps[-1], flip_q16=k)
    _eq(got, engine.montecarlo_sweep_lists(n, base, lists, cps, scen).cpu().numpy(), "lists:")


def test_guard_words_around_out_and_out_is_checked(engine):
    import torch
    QbaError = sub("_lib").QbaError
    n, inst, base, cps = 7, 37, 99, [0, 3, 70]
    scen = [(2, LOW), (7, REFERENCE)]
    k, s, words, fill, guard = len(cps), len(scen), 4 + 5 * (n + 1), 0x5A5A5A5A, 64
    lists, _ = engine.sample_check_batched(n, base, inst, cps[-1])
    want = _separate(engine, n, base, inst, cps, scen)
    runs = {"sampled": lambda o: engine.montecarlo_sweep_sampled(n, base, inst, cps, scen, out=o),
            "lists": lambda o: engine.montecarlo_sweep_lists(n, base, lists, cps, scen, out=o)}
    for what, run in runs.items():
        for shape in ((k, s, inst, words), (k * s, inst, words)):   # the grid, or the slices as the tally takes them
            buf = torch.full((guard + k * s * inst * words + guard,), fill, dtype=torch.int32, device=engine.device)
            out = buf[guard:guard + k * s * inst * words].view(shape)
            ret = run(out)
            assert ret.data_ptr() == out.data_ptr() and tuple(ret.shape) == (k, s, inst, words)
            flat = buf.cpu().numpy()
            assert np.all(flat[:guard] == fill) and np.all(flat[-guard:] == fill), what
            _eq(ret.cpu().numpy(), want, f"{what}:")
        z = lambda *sh, **kw: torch.zeros(sh, dtype=kw.get("dtype", torch.int32), device=engine.device)  # noqa: E731
        for bad in (z(k, s, inst, words, dtype=torch.int64), z(k, s + 1, inst, words), z(s, k, inst, words + 1),
                    z(k, s, inst, 2 * words)[..., ::2], z(k * s * inst, words)):
            with pytest.raises(QbaError):
                run(bad)
    assert tuple(engine.montecarlo_sweep_sampled(n, base, 0, cps, scen).shape) == (k, s, 0, words)


def test_non_default_stream(engine):
    import torch
    n, base, cps = 7, 31337, [5, 50, 64]
    scen = _grid(n)[1:4]
    want = _separate(engine, n, base, INST, cps, scen)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = engine.montecarlo_sweep_sampled(n, base, INST, cps, scen)
        lists, _ = engine.sample_check_batched(n, base, INST, cps[-1])
        got_l = engine.montecarlo_sweep_lists(n, base, lists, cps, scen)
    side.synchronize()
    _eq(got.cpu().numpy(), want, "sampled:")
    _eq(got_l.cpu().numpy(), want, "lists:")


# ---- host paths -------------------------------------------------------------------
def test_sweep_across_a_batch_split_with_tally_and_failures(engine):
    mc = sub("montecarlo")
    n, runs, seed, cps, k = 7, 300, 0xAD0, [3, 8], 0x1000
    scen = [(2, STRIP), (2, REFERENCE), (5, LOW)]
    for flip in (0, k):
        kw = {"flip_q16": flip} if flip else {}
        want = mc.sweep(n, cps, scen, runs, seed, engine, batch=128, **kw)
        assert list(want) == [(c, kd, word) for c in cps for kd, word in scen]
        got = mc.sweep(n, cps, scen, runs, seed, engine, batch=128, tally=True, failures=4, **kw)
        for kd, word in scen:
            curve = mc.curve(n, cps, kd, runs, seed, engine, batch=128, adversary=word, **kw)
            rows = engine.montecarlo_curve_sampled(n, kd, seed, runs, cps, adversary=word, **kw).cpu().numpy()
            for j, c in enumerate(cps):
                key = (c, kd, word)
                assert want[key] == curve[c], key
                assert all(got[key][f] == want[key][f] for f in want[key]), key
                failed = {int(i) for i in np.nonzero(rows[j, :, 0] == 0)[0]}
                assert got[key]["failed_total"] == len(failed) == runs - want[key]["successes"]
                assert set(got[key]["failed_runs"]) <= failed and len(got[key]["failed_runs"]) == min(4, len(failed))
    assert len({want[key]["successes"] for key in want}) > 1   # the grid is not one number


def test_cli_sweep_prints_the_lines_of_the_curve_adversary_runs():
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "tfg---quantum-byzantine-agreement_amd.tfg"]
    tail = ["--parties", "7", "--runs", "300", "--seed", "2768", "--curve", "3", "--flip", "4096"]

    def lines(cmd):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        return [l for l in out.stdout.splitlines() if l.startswith("Runs:")]

    grid = lines(base + ["8", "2"] + tail + ["--sweep", "strip,4:reorder_low"])
    assert len(grid) == 4 and all(l.startswith("Runs: 300 Successes:") for l in grid)
    strip = lines(base + ["8", "2"] + tail + ["--adversary", "strip"])
    low = lines(base + ["8", "4"] + tail + ["--adversary", "reorder_low"])
    assert len(strip) == len(low) == 2
    assert grid == [strip[0], low[0], strip[1], low[1]]
    assert "sizeL=3, dishonest=2," in grid[0] and grid[3].endswith(f"flip=4096/65536 adversary={LOW:#x}")
