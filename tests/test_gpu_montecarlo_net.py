"""The lossy-network kernels on the GPU.  Every
comparison is exact, status included.  At net = 0 both calls must write the rows
of the _adv curve calls word for word; under every other word they must write
the rows of the host model (montecarlo.curve_host with ``net=``), on a grid of
shapes, on the reach sets of tests/montecarlo_net_cases.py and on the hostile
and sweep sets; at n = 15, beyond the C twin's sampler, the host model takes the
device's own lists.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, sub
from montecarlo_cases import HOSTILE, HOSTILE_IDS, SWEEP, SWEEP_IDS, hostile_lists
from montecarlo_net_cases import CMD, FIVE, REACH, reach_rows
from test_gpu_montecarlo_adversary import _batched, _eq, _nds
from test_montecarlo_adversary import HostEngine, NOISE_K, PRESETS

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 7, 11, 15]
COUNTS = [0, 3, 65, 130]  # 65 and 130 straddle a 64-entry step
NETS = [0, 1, 0x2000, 0x8000 | CMD, 0xFFFF, 0xFFFF | CMD]
FLIPS = [0, 1, 0x1000]
LOW = PRESETS["reorder_low"]
POLICIES = [0xF, LOW, FIVE]
INST, GRID_BASE = 67, 0x4E4757  # one wavefront's worth of instances and a ragged tail
GRID = [(n, nd) for n in NS for nd in _nds(n)]  # traitors {0, 1, n // 3, n - 1}


def _flip_and_policy(i, gi):
    return FLIPS[(i + gi) % 3], POLICIES[(i + gi // 3) % 3]


CASES = [(gi, i) for gi in range(len(GRID)) for i in range(len(NETS))]


@pytest.mark.parametrize("gi,i", CASES, ids=[f"n{GRID[gi][0]}-d{GRID[gi][1]}-net{NETS[i]:#x}" for gi, i in CASES])
def test_every_word_on_the_grid_equals_the_host_model(engine, gi, i):
    """Both kernels at the checkpoints [0, 3, 65, 130], all 67 instances against
    curve_host.  Word i at grid point gi runs under flip FLIPS[(i + gi) % 3] and
    policy POLICIES[(i + gi // 3) % 3]
    (test_the_grid_rotation_covers_every_word_flip_and_policy)."""
    mc = sub("montecarlo")
    (n, nd), word = GRID[gi], NETS[i]
    k, adv = _flip_and_policy(i, gi)
    got = engine.montecarlo_curve_sampled_net(n, nd, GRID_BASE, INST, COUNTS, flip_q16=k, adversary=adv, net=word)
    got = got.cpu().numpy()
    lists, _ = _batched(engine, n, GRID_BASE, INST, COUNTS[-1], flip=k)
    _eq(engine.montecarlo_curve_lists_net(n, nd, GRID_BASE, lists, COUNTS, adversary=adv, net=word).cpu().numpy(), got,
        f"flip={k:#x} adv={adv:#x} lists:")
    if n <= 11:
        want = mc.curve_host(n, COUNTS, nd, INST, GRID_BASE, HostEngine(), flip_q16=k, adversary=adv, net=word)
    else:  # the lists the device sampled (noise included) go to the host model as they are
        li = lists.cpu().numpy()[:, :, :COUNTS[-1]]
        want = mc.curve_host(n, COUNTS, nd, INST, GRID_BASE, HostEngine(), lists=li, adversary=adv, net=word)
    _eq(got, want, f"flip={k:#x} adv={adv:#x} host:")
    assert not got[:, :, 3].any()


def test_the_grid_rotation_covers_every_word_flip_and_policy():
    """Every net word meets every flip under every policy, and at n >= 7 too."""
    everything = len(NETS) * len(FLIPS) * len(POLICIES)
    seen = {(i, *_flip_and_policy(i, gi)) for gi, i in CASES}
    assert len(seen) == everything
    large = {(i, *_flip_and_policy(i, gi)) for gi, i in CASES if GRID[gi][0] >= 7}
    assert len(large) == everything


@pytest.mark.parametrize("n", NS)
def test_the_perfect_network_equals_the_adv_curve_calls(engine, n):
    """net = 0 (and None): both calls against the _adv curve calls for whole
    batches, every word, status included."""
    for nd in _nds(n):
        lists, _ = _batched(engine, n, GRID_BASE, INST, COUNTS[-1])
        for adv in POLICIES:
            want = engine.montecarlo_curve_lists(n, nd, GRID_BASE, lists, COUNTS, adversary=adv).cpu().numpy()
            for word in (0, None):
                _eq(engine.montecarlo_curve_lists_net(n, nd, GRID_BASE, lists, COUNTS, adversary=adv, net=word)
                    .cpu().numpy(), want, f"lists nd={nd} adv={adv:#x}:")
            for k in FLIPS:
                _eq(engine.montecarlo_curve_sampled_net(n, nd, GRID_BASE, INST, COUNTS, flip_q16=k, adversary=adv,
                                                        net=0).cpu().numpy(),
                    engine.montecarlo_curve_sampled(n, nd, GRID_BASE, INST, COUNTS, flip_q16=k, adversary=adv)
                    .cpu().numpy(), f"sampled nd={nd} adv={adv:#x} flip={k:#x}:")


def test_a_whole_batch_on_the_perfect_network_equals_the_adv_call(engine):
    n, nd, inst, cps = 11, 3, 4096, [200]
    for adv in (0xF, LOW):
        _eq(engine.montecarlo_curve_sampled_net(n, nd, 0xAD0, inst, cps, adversary=adv, net=0).cpu().numpy(),
            engine.montecarlo_curve_sampled(n, nd, 0xAD0, inst, cps, adversary=adv).cpu().numpy(), f"adv={adv:#x}:")
    lists, _ = _batched(engine, n, 0xAD0, inst, cps[0])
    _eq(engine.montecarlo_curve_lists_net(n, nd, 0xAD0, lists, cps, net=0).cpu().numpy(),
        engine.montecarlo_curve_lists(n, nd, 0xAD0, lists, cps, adversary=0xF).cpu().numpy(), "lists:")


@pytest.mark.parametrize("name", list(REACH))
def test_reach_sets_through_both_kernels_equal_the_host_model(engine, name):
    """The sets on which the host model shows partial loss on a link, seq >= 4,
    broken agreement, a changed V_i, lost commander packets (relayed and not)
    and lost mutated packets."""
    mc = sub("montecarlo")
    n, nd, sizeL, base, inst, injected, adv, word, _ = REACH[name]
    cps = [sizeL // 2, sizeL]
    want = reach_rows(mc, name, counts=cps)
    if injected is None:
        eng = HostEngine()
        li = np.stack([eng.sample(n, base + i, 0, sizeL) for i in range(inst)])
        _eq(engine.montecarlo_curve_sampled_net(n, nd, base, inst, cps, adversary=adv, net=word).cpu().numpy(), want,
            "sampled:")
    else:
        li = np.ascontiguousarray(injected)
    _eq(engine.montecarlo_curve_lists_net(n, nd, base, li, cps, adversary=adv, net=word).cpu().numpy(), want, "lists:")
    assert not want[:, :, 3].any()


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_lists_form_on_hostile_and_sweep_sets_with_a_planted_range_error(engine, case):
    """Deep rounds, duplicated rows, many traitors, six packets in a mailbox
    cell: two network words against the host model, no status bit.  Then a
    value >= w planted once at a Q-correlated position of instance 1: status 4
    in exactly the checkpoints past it, as the _adv call gives, and every other
    row unchanged."""
    mc = sub("montecarlo")
    n, nd, sizeL, keys, base = case["n"], case["nDishonest"], case["sizeL"], case["keys"], case["base"]
    li = hostile_lists(case)
    cps = [sizeL // 2, sizeL]
    planted = np.array(li)
    inst = min(1, keys - 1)
    q = np.nonzero(planted[inst, 0] != planted[inst, 1])[0]
    at = int(q[q >= cps[0]][0])  # past the first checkpoint, inside the second
    planted[inst, n, at] = 1 << n.bit_length()
    for adv, word in ((0xF, 0x2000), (LOW, 0x8000 | CMD)):
        want = mc.curve_host(n, cps, nd, keys, base, HostEngine(), lists=li, adversary=adv, net=word)
        got = engine.montecarlo_curve_lists_net(n, nd, base, np.ascontiguousarray(li), cps, adversary=adv, net=word)
        got = got.cpu().numpy()
        _eq(got, want, f"adv={adv:#x} net={word:#x}:")
        assert not got[:, :, 3].any()
        bad = engine.montecarlo_curve_lists_net(n, nd, base, planted, cps, adversary=adv, net=word).cpu().numpy()
        adv_bad = engine.montecarlo_curve_lists(n, nd, base, planted, cps, adversary=adv).cpu().numpy()
        assert np.array_equal(bad[:, :, 3], adv_bad[:, :, 3])
        assert bad[1, inst, 3] == 4 and not bad[1, inst, :3].any() and not bad[1, inst, 4:].any()
        assert bad[0, inst, 3] == 0 and int((bad[:, :, 3] != 0).sum()) == 1
        bad[1, inst] = got[1, inst]
        _eq(bad, got, f"adv={adv:#x} net={word:#x} beside the planted value:")


def test_key_wraps_mod_2_64(engine):
    mc = sub("montecarlo")
    n, nd, cps, inst, base, word = 7, 2, [3, 8], 8, (1 << 64) - 3, 0x4000 | CMD
    got = engine.montecarlo_curve_sampled_net(n, nd, base, inst, cps, flip_q16=NOISE_K, adversary=LOW, net=word)
    got = got.cpu().numpy()
    _eq(got, mc.curve_host(n, cps, nd, inst, base, HostEngine(), flip_q16=NOISE_K, adversary=LOW, net=word), "host:")
    _eq(got[:, 3:], engine.montecarlo_curve_sampled_net(n, nd, 0, inst - 3, cps, flip_q16=NOISE_K, adversary=LOW,
                                                        net=word).cpu().numpy(), "keys 0..4:")
    lists, _ = _batched(engine, n, base, inst, cps[-1], flip=NOISE_K)
    _eq(engine.montecarlo_curve_lists_net(n, nd, base, lists, cps, adversary=LOW, net=word).cpu().numpy(), got,
        "lists:")
    plain = engine.montecarlo_curve_sampled(n, nd, base, inst, cps, flip_q16=NOISE_K, adversary=LOW).cpu().numpy()
    assert (got != plain).any()  # the loss shows on these keys


def test_a_capture_of_both_calls_replayed_twice_gives_equal_rows(engine):
    """The calls allocate and copy nothing: legal in a stream capture."""
    import torch
    mc = sub("montecarlo")
    n, nd, cps, inst, base, word = 7, 2, [3, 65], 67, 0xAD0, 0x2000 | CMD
    words = 4 + 5 * (n + 1)
    lists, _ = _batched(engine, n, base, inst, cps[-1])
    outs = [torch.zeros((2, inst, words), dtype=torch.int32, device=engine.device) for _ in range(2)]
    engine.montecarlo_curve_sampled_net(n, nd, base, inst, cps, out=outs[0], adversary=LOW, net=word)  # warm: the program
    engine.montecarlo_curve_lists_net(n, nd, base, lists, cps, out=outs[1], adversary=LOW, net=word)
    torch.cuda.synchronize()
    for o in outs:
        o.zero_()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            engine.montecarlo_curve_sampled_net(n, nd, base, inst, cps, out=outs[0], adversary=LOW, net=word)
            engine.montecarlo_curve_lists_net(n, nd, base, lists, cps, out=outs[1], adversary=LOW, net=word)
    torch.cuda.synchronize()
    assert not outs[0].any() and not outs[1].any()  # captured, not run
    want = mc.curve_host(n, cps, nd, inst, base, HostEngine(), adversary=LOW, net=word)
    for replay in range(2):
        g.replay()
        torch.cuda.synchronize()
        for what, o in zip(("sampled", "lists"), outs):
            _eq(o.cpu().numpy(), want, f"replay {replay} {what}:")
            o.zero_()


def test_run_and_curve_across_a_batch_split_with_tally_and_failures(engine):
    mc = sub("montecarlo")
    n, nd, sizeL, runs, base, word = 7, 2, 8, 300, 0xAD0, 0x2000
    cps = [3, sizeL]
    for k, adv in ((0, None), (NOISE_K, LOW)):
        kw = ({"flip_q16": k} if k else {}) | ({"adversary": adv} if adv is not None else {})
        rows = engine.montecarlo_curve_sampled_net(n, nd, base, runs, cps, net=word, **kw).cpu().numpy()
        want = mc.curve(n, cps, nd, runs, base, engine, batch=128, net=word, **kw)
        got = mc.curve(n, cps, nd, runs, base, engine, batch=128, net=word, tally=True, failures=4, **kw)
        for j, c in enumerate(cps):
            assert want[c] == mc.summarize(n, rows[j]), (k, c)
            assert all(got[c][key] == want[c][key] for key in want[c]), (k, c)
            failed = {int(i) for i in np.nonzero(rows[j][:, 0] == 0)[0]}
            assert got[c]["failed_total"] == len(failed) and set(got[c]["failed_runs"]) <= failed
            assert len(got[c]["failed_runs"]) == min(4, len(failed))
        assert mc.run(n, sizeL, nd, runs, base, engine, batch=128, path="fused", net=word, **kw) == want[sizeL]
        few = mc.run(n, sizeL, nd, runs, base, engine, batch=128, path="fused", net=word, tally=True, failures=4, **kw)
        assert set(few["failed_runs"]) <= failed and len(few["failed_runs"]) == min(4, len(failed))
        assert few["failed_runs"] == sorted(few["failed_runs"]) and few["failed_total"] == len(failed)
        assert all(few[key] == want[sizeL][key] for key in want[sizeL])
        plain = mc.curve(n, cps, nd, runs, base, engine, batch=128, **kw)
        assert mc.curve(n, cps, nd, runs, base, engine, batch=128, net=0, **kw) == plain
        assert want != plain  # it matters
        host = mc.summarize(n, mc.run_host(n, sizeL, nd, 64, base, HostEngine(), net=word, **kw))
        assert mc.run(n, sizeL, nd, 64, base, engine, path="fused", net=word, tally=True, failures=4, **kw)[
            "successes"] == host["successes"]


def test_cli_with_drop_against_the_host_models_summary(engine):
    mc = sub("montecarlo")
    cmd = [sys.executable, "-m", "tfg---quantum-byzantine-agreement_amd.tfg", "65", "2", "--parties", "7", "--runs",
           "48", "--drop", "0x2000", "--curve", "3,65", "--seed", "2768"]
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    res = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("Runs:")]
    rows = mc.curve_host(7, [3, 65], 2, 48, 2768, HostEngine(), net=0x2000)
    assert len(lines) == 2
    for line, c, r in zip(lines, (3, 65), rows):
        s = mc.summarize(7, r)
        assert line.startswith(f"Runs: 48 Successes: {s['successes']} Rate: {s['rate']:.6f} ") and f"sizeL={c}," in line
        assert f"empty-V_i runs={s['empty_vi_runs']})" in line and line.endswith(" drop=8192/65536")
    res = subprocess.run(cmd[:cmd.index("0x2000")] + ["0x2000:cmd"] + cmd[cmd.index("0x2000") + 1:], cwd=str(ROOT),
                         capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("Runs:")]
    rows = mc.curve_host(7, [3, 65], 2, 48, 2768, HostEngine(), net=0x2000 | CMD)
    for line, r in zip(lines, rows):
        assert line.startswith(f"Runs: 48 Successes: {mc.summarize(7, r)['successes']} ")
        assert line.endswith(" drop=8192/65536 cmd")
