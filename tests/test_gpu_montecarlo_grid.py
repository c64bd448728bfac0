"""The (traitors, policy, loss) grid on the GPU.
Every comparison is exact, status included.  The reference is always a call
that existed before: slice (j, s) of a grid against
montecarlo_curve_sampled_net / montecarlo_curve_lists_net under scenario s, the
slices on the perfect network also against montecarlo_sweep_sampled, and the
host model montecarlo.grid_host where the C twin samples (n <= 11) or on
injected lists."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, sub
from montecarlo_cases import HOSTILE, HOSTILE_IDS, SWEEP, SWEEP_IDS, hostile_lists
from test_gpu_montecarlo_sweep import _eq
from test_montecarlo_adversary import HostEngine, PRESETS

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 7, 11, 12, 15]
COUNTS = [0, 3, 65, 130]  # 65 and 130 straddle a 64-entry step
FLIPS = [0, 1, 0x1000]
INST, BASE = 67, 0x6D1D5EED
CMD = 1 << 16
REFERENCE, LOW, FIVE = 0xF, PRESETS["reorder_low"], 0x1F
PERFECT, DEAD = 0, 0xFFFF | CMD  # the perfect network; nearly every packet lost, the commander's too


def _grid(n):
    """The main grid: k in {0, 1, n // 3, n - 1} (clipped to [0, n]), three
    policies, and every one of the six network words once."""
    clip = lambda k: min(max(k, 0), n)  # noqa: E731
    return [(clip(1), LOW, PERFECT), (0, REFERENCE, 1), (clip(n // 3), FIVE, 0x2000),
            (clip(n - 1), REFERENCE, 0x8000 | CMD), (clip(1), FIVE, 0xFFFF), (clip(n // 3), LOW, DEAD)]


def _separate(engine, n, base, inst, counts, scen, flip=0):
    """The grid's rows from one montecarlo_curve_sampled_net call per scenario,
    [len(counts), len(scen), inst, words]."""
    memo = {}
    for t in scen:
        if t not in memo:
            k, word, net = t
            memo[t] = engine.montecarlo_curve_sampled_net(n, k, base, inst, counts, flip_q16=flip, adversary=word,
                                                          net=net).cpu().numpy()
    return np.stack([memo[t] for t in scen], axis=1)


@pytest.fixture(scope="module")
def basic():
    """(n, flip) -> the separate calls' rows of the main grid, computed once and read-only."""
    memo = {}

    def get(engine, n, flip):
        if (n, flip) not in memo:
            memo[n, flip] = _separate(engine, n, BASE, INST, COUNTS, _grid(n), flip)
            memo[n, flip].setflags(write=False)
        return memo[n, flip]
    return get


@pytest.mark.parametrize("flip", FLIPS, ids=[f"flip{k:#x}" for k in FLIPS])
@pytest.mark.parametrize("n", NS)
def test_sampled_form_equals_the_net_curve_call_of_every_scenario(engine, basic, n, flip):
    scen = _grid(n)
    want = basic(engine, n, flip)
    got = engine.montecarlo_grid_sampled(n, BASE, INST, COUNTS, scen, flip_q16=flip).cpu().numpy()
    _eq(got, want, f"n={n} flip={flip:#x}:")
    assert not got[..., 3].any()
    perfect = [s for s, t in enumerate(scen) if t[2] == PERFECT]
    _eq(got[:, perfect], engine.montecarlo_sweep_sampled(n, BASE, INST, COUNTS, [scen[s][:2] for s in perfect],
                                                         flip_q16=flip).cpu().numpy(), "the sweep call:")
    if n >= 3:  # not vacuous: the networks and the checkpoints give different rows
        assert not np.array_equal(got[-1, 2], got[-1, 5]) and not np.array_equal(got[1, 2], got[-1, 2])
    if n <= 11 and flip != 1:  # the host model on the first instances (flip = 1 is covered by the calls above)
        few = 3 if n <= 7 else 2
        _eq(got[:, :, :few], sub("montecarlo").grid_host(n, COUNTS, scen, few, BASE, HostEngine(), flip_q16=flip),
            f"host n={n} flip={flip:#x}:")


@pytest.mark.parametrize("n", [3, 7, 12])
def test_no_state_leaks_between_scenarios(engine, basic, n):
    """The scenario list reversed; a network that loses the commander's
    packets (the sentinel in S.cv) between two perfect ones; one scenario at
    positions 0 and 15."""
    scen = _grid(n)
    want = basic(engine, n, 0)
    order = list(range(len(scen)))[::-1]
    got = engine.montecarlo_grid_sampled(n, BASE, INST, COUNTS, [scen[s] for s in order]).cpu().numpy()
    _eq(got, want[:, order], "reversed:")
    k = scen[5][0]
    between = [(k, LOW, PERFECT), (k, LOW, DEAD), (k, LOW, PERFECT), (k, REFERENCE, DEAD), (n, FIVE, PERFECT)]
    got = engine.montecarlo_grid_sampled(n, BASE, INST, COUNTS, between).cpu().numpy()
    _eq(got[:, 1], want[:, 5], "the lossy one:")
    _eq(got[:, 0], got[:, 2], "the perfect ones around it:")
    _eq(got[:, [0, 4]], engine.montecarlo_sweep_sampled(n, BASE, INST, COUNTS, [(k, LOW), (n, FIVE)]).cpu().numpy(),
        "perfect after lossy against the sweep call:")
    assert not np.array_equal(got[-1, 0], got[-1, 1])  # the loss shows
    cps = COUNTS[1:3]
    sixteen = [scen[3]] + [scen[s % 6] for s in range(14)] + [scen[3]]
    got = engine.montecarlo_grid_sampled(n, BASE, INST, cps, sixteen).cpu().numpy()
    _eq(got[:, 0], got[:, 15], "positions 0 and 15:")
    _eq(got[:, 15], want[1:3, 3], "position 15:")


def test_bounds_sixteen_by_two_one_by_thirty_two_and_one_by_one(engine):
    n, base, inst = 7, 0x5EED5, 33
    nets = [PERFECT, 1, 0x100, 0x2000, 0x8000 | CMD, 0xFFFF, DEAD, 0x400 | CMD]
    scen = [(k % (n + 1), w, nets[(k + k // 8) % 8])
            for k, w in zip(range(16), [REFERENCE, LOW, FIVE, PRESETS["strip"]] * 4)]
    assert len(set(scen)) == 16
    cps = [3, 65]
    _eq(engine.montecarlo_grid_sampled(n, base, inst, cps, scen).cpu().numpy(),
        _separate(engine, n, base, inst, cps, scen), "16 x 2:")
    cps = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 64, 65, 66, 89, 100, 127, 128, 129, 130, 144, 160, 191, 192, 193, 200,
           233, 255, 256, 257, 300, 377]
    assert len(cps) == 32
    for flip in (0, 0x1000):
        one = [(3, FIVE, 0x2000 | CMD)]
        _eq(engine.montecarlo_grid_sampled(n, base, inst, cps, one, flip_q16=flip).cpu().numpy(),
            _separate(engine, n, base, inst, cps, one, flip), f"1 x 32 flip={flip:#x}:")
    for count in (0, 1, 65):
        one = engine.montecarlo_grid_sampled(n, base, inst, [count], [(2, LOW, 0x4000)]).cpu().numpy()
        assert one.shape[:2] == (1, 1)
        _eq(one[0], engine.montecarlo_curve_sampled_net(n, 2, base, inst, [count], adversary=LOW, net=0x4000)
            .cpu().numpy(), "1 x 1:")
    QbaError = sub("_lib").QbaError
    for counts, sc in (([3, 65, 130], [(1, LOW, 1)] * 11), ([3], [(1, LOW, 1)] * 17), ([3], []),
                       ([3], [(n + 1, LOW, 1)]), ([3], [(1, LOW, CMD)]), ([3], [(1, LOW, 1 << 17)])):
        with pytest.raises(QbaError):
            engine.montecarlo_grid_sampled(n, base, inst, counts, sc)


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_lists_form_on_hostile_and_sweep_sets(engine, case):
    """Deep rounds, duplicated rows, many traitors, six packets in a mailbox
    cell (n15-d8-L96-dup_cmd: seq >= 4, the second loss block) under three
    scenarios, against the _net lists call and the host model; then a value
    >= w planted at a Q-correlated position: status 4 in exactly the slices
    past it under every scenario."""
    import torch
    mc = sub("montecarlo")
    n, nd, L, keys, base = case["n"], case["nDishonest"], case["sizeL"], case["keys"], case["base"]
    li = np.array(hostile_lists(case), order="C")  # a writable, contiguous copy
    dev = torch.from_numpy(li).to(engine.device)
    counts = [L // 2, L]
    scen = [(nd, REFERENCE, 0x1000), (nd, LOW, 0x8000 | CMD), (nd, REFERENCE, PERFECT)]
    got = engine.montecarlo_grid_lists(n, base, dev, counts, scen).cpu().numpy()
    assert got.shape == (len(counts), len(scen), keys, mc.out_words(n))
    for s, (k, word, net) in enumerate(scen):
        _eq(got[:, s], engine.montecarlo_curve_lists_net(n, k, base, dev, counts, adversary=word, net=net)
            .cpu().numpy(), f"scenario {s} against curve_lists_net:")
    assert not got[..., 3].any()
    _eq(got, mc.grid_host(n, counts, scen, keys, base, HostEngine(), lists=li), "host:")
    at, w = keys // 2, 1 << mc._nq(n)
    qs = np.nonzero(li[at, 0] != li[at, 1])[0]
    k_pos = int(qs[qs >= counts[0]][0])  # past the first checkpoint, inside the second
    bad = li.copy()
    bad[at, 1, k_pos] = w
    rows = engine.montecarlo_grid_lists(n, base, bad, counts, scen).cpu().numpy()
    flagged = [0, 0, 0, mc.ST_RANGE] + [0] * (5 * (n + 1))
    for s in range(len(scen)):
        assert rows[1, s, at].tolist() == flagged, s
        assert rows[0, s, at, 3] == 0, s
    assert int((rows[..., 3] != 0).sum()) == len(scen)
    keep = np.arange(keys) != at
    _eq(rows[:, :, keep], got[:, :, keep], "the other instances:")
    _eq(rows[0], got[0], "the checkpoint before the plant:")


def test_lists_form_on_the_devices_own_sampled_rows_equals_the_sampled_form(engine):
    n, base, inst, counts = 7, 3000, 32, [0, 1, 66, 200]
    scen = _grid(n)
    lists, _ = engine.sample_check_batched(n, base, inst, counts[-1])  # rows 4 KiB apart, as sampled
    _eq(engine.montecarlo_grid_lists(n, base, lists, counts, scen).cpu().numpy(),
        engine.montecarlo_grid_sampled(n, base, inst, counts, scen).cpu().numpy(), "lists against sampled:")


# ---- launch and buffer edges, once each ------------------------------------------
def test_past_the_resident_waves_at_n11(engine):
    import torch
    n, base, cps, inst = 11, 0xAD0, [3, 8], 20011
    scen = [(3, LOW, 0x2000), (0, REFERENCE, PERFECT), (10, FIVE, 0x8000 | CMD)]
    engine.prepare(n)
    sh = engine.montecarlo_program_shape(n, curve=True)
    assert (sh["waves_run"], sh["lds_bytes"], sh["wgs_per_cu"]) == engine.montecarlo_curve_shape(n)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert inst > cus * sh["wgs_per_cu"] * sh["waves_run"] + sh["waves_run"]  # every wave takes a second trip
    got = engine.montecarlo_grid_sampled(n, base, inst, cps, scen).cpu().numpy()
    _eq(got, _separate(engine, n, base, inst, cps, scen), "20,011 instances:")
    _eq(got[:, :, -3:], sub("montecarlo").grid_host(n, cps, scen, 3, base + inst - 3, HostEngine()), "host, last:")


def test_key_wraps_mod_2_64(engine):
    mc = sub("montecarlo")
    n, inst, base, cps, k = 7, 8, (1 << 64) - 3, [3, 8], 0x1000
    scen = [(2, LOW, 0x4000 | CMD), (6, FIVE, PERFECT), (2, LOW, 0x4000)]
    got = engine.montecarlo_grid_sampled(n, base, inst, cps, scen, flip_q16=k).cpu().numpy()
    _eq(got, mc.grid_host(n, cps, scen, inst, base, HostEngine(), flip_q16=k), "host:")
    _eq(got[:, :, 3:], engine.montecarlo_grid_sampled(n, 0, inst - 3, cps, scen, flip_q16=k).cpu().numpy(),
        "keys 0..4:")
    lists, _ = engine.sample_check_batched(n, base & ((1 << 64) - 1), inst, cps[-1], flip_q16=k)
    _eq(got, engine.montecarlo_grid_lists(n, base, lists, cps, scen).cpu().numpy(), "lists:")
    assert not np.array_equal(got[:, 0], got[:, 2])  # the commander's links matter on these keys


def test_guard_words_around_out_and_out_is_checked(engine):
    import torch
    QbaError = sub("_lib").QbaError
    n, inst, base, cps = 7, 37, 99, [0, 3, 70]
    scen = [(2, LOW, 0x2000 | CMD), (7, REFERENCE, PERFECT)]
    k, s, words, fill, guard = len(cps), len(scen), 4 + 5 * (n + 1), 0x5A5A5A5A, 64
    lists, _ = engine.sample_check_batched(n, base, inst, cps[-1])
    want = _separate(engine, n, base, inst, cps, scen)
    runs = {"sampled": lambda o: engine.montecarlo_grid_sampled(n, base, inst, cps, scen, out=o),
            "lists": lambda o: engine.montecarlo_grid_lists(n, base, lists, cps, scen, out=o)}
    for what, run in runs.items():
        for shape in ((k, s, inst, words), (k * s, inst, words)):  # the grid, or the slices as the tally takes them
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
    assert tuple(engine.montecarlo_grid_sampled(n, base, 0, cps, scen).shape) == (k, s, 0, words)


def test_non_default_stream(engine):
    import torch
    n, base, cps = 7, 31337, [5, 50, 64]
    scen = _grid(n)[1:5]
    want = _separate(engine, n, base, INST, cps, scen)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = engine.montecarlo_grid_sampled(n, base, INST, cps, scen)
        lists, _ = engine.sample_check_batched(n, base, INST, cps[-1])
        got_l = engine.montecarlo_grid_lists(n, base, lists, cps, scen)
    side.synchronize()
    _eq(got.cpu().numpy(), want, "sampled:")
    _eq(got_l.cpu().numpy(), want, "lists:")


# ---- host paths -------------------------------------------------------------------
def test_grid_across_a_batch_split_with_tally_and_failures(engine):
    mc = sub("montecarlo")
    n, runs, seed, cps, k = 7, 300, 0xAD0, [3, 8], 0x1000
    scen = [(2, REFERENCE, PERFECT), (2, REFERENCE, 0x2000), (2, LOW, 0x8000 | CMD), (5, LOW, 0x2000)]
    for flip in (0, k):
        kw = {"flip_q16": flip} if flip else {}
        want = mc.grid(n, cps, scen, runs, seed, engine, batch=128, **kw)
        assert list(want) == [(c, kd, word, net) for c in cps for kd, word, net in scen]
        got = mc.grid(n, cps, scen, runs, seed, engine, batch=128, tally=True, failures=4, **kw)
        for kd, word, net in scen:
            curve = mc.curve(n, cps, kd, runs, seed, engine, batch=128, adversary=word, net=net, **kw)
            rows = engine.montecarlo_curve_sampled_net(n, kd, seed, runs, cps, adversary=word, net=net, **kw)
            rows = rows.cpu().numpy()
            for j, c in enumerate(cps):
                key = (c, kd, word, net)
                assert want[key] == curve[c], key
                assert all(got[key][f] == want[key][f] for f in want[key]), key
                failed = {int(i) for i in np.nonzero(rows[j, :, 0] == 0)[0]}
                assert got[key]["failed_total"] == len(failed) == runs - want[key]["successes"]
                assert set(got[key]["failed_runs"]) <= failed and len(got[key]["failed_runs"]) == min(4, len(failed))
        sweep = mc.sweep(n, cps, [(2, REFERENCE)], runs, seed, engine, batch=128, **kw)
        assert all(want[c, 2, REFERENCE, PERFECT] == sweep[c, 2, REFERENCE] for c in cps)
    assert len({want[key]["successes"] for key in want}) > 1  # the grid is not one number


def test_cli_grid_prints_the_lines_of_the_curve_adversary_drop_runs(engine, capsys):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "tfg---quantum-byzantine-agreement_amd.tfg"]
    tail = ["--parties", "7", "--runs", "300", "--seed", "2768", "--curve", "3", "--flip", "4096"]

    def lines(cmd):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        return [l for l in out.stdout.splitlines() if l.startswith("Runs:")]

    grid = lines(base + ["8", "2"] + tail + ["--grid", "strip@0x2000,4:reorder_low@0x8000:cmd,strip"])
    assert len(grid) == 6 and all(l.startswith("Runs: 300 Successes:") for l in grid)
    strip = lines(base + ["8", "2"] + tail + ["--adversary", "strip", "--drop", "0x2000"])
    low = lines(base + ["8", "4"] + tail + ["--adversary", "reorder_low", "--drop", "0x8000:cmd"])
    # the item on the perfect network prints its --sweep line: taken in this process, on the session's engine
    tfg = sub("tfg")
    capsys.readouterr()
    assert tfg._montecarlo(tfg._args(["8", "2"] + tail + ["--sweep", "strip"]), engine, 8) == 0
    perfect = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Runs:")]
    assert len(strip) == len(low) == len(perfect) == 2
    assert grid == [strip[0], low[0], perfect[0], strip[1], low[1], perfect[1]]
    assert "sizeL=3, dishonest=2," in grid[0] and grid[0].endswith(" drop=8192/65536")
    assert grid[4].endswith(f"flip=4096/65536 adversary={LOW:#x} drop=32768/65536 cmd")
    assert grid[5].endswith(f"adversary={PRESETS['strip']:#x}") and "drop=" not in grid[5]
