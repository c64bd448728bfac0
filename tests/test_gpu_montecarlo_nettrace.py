"""The trace kernels on a lossy network on the GPU.
The reference is always montecarlo.trace_net_host on the same keys: the traced
row, the exact event counts and every stored event are compared word for word.
For n <= 11 the host samples with the C twin; above, it takes the lists the
device samples."""
import numpy as np
import pytest

from conftest import sub
from montecarlo_net_cases import CMD
from montecarlo_nettrace_cases import CAP, CASES, LISTS, SAMPLED, reach_trace
from test_montecarlo_adversary import HostEngine, PRESETS

pytestmark = pytest.mark.gpu

IDX = [0, 1, 66, 5, 5, (1 << 40) + 3]  # unsorted, repeated, large
GRID_BASE = 0xADA11CE
MASK64 = (1 << 64) - 1
GUARD = 0x5A5A5A5A
NETS = [0x8000, 0xFFFF | CMD]


def _host(engine, n, sizeL, nd, idx, base, flip, word, net, lists=None):
    """trace_net_host of the keys base + idx; n > 11: on the device's own samples."""
    mc = sub("montecarlo")
    if lists is None and n > 11:
        lists = np.zeros((len(idx), n + 1, sizeL), np.uint8)
        for j, i in enumerate(idx if sizeL else []):
            lists[j] = engine.sample(n, (base + i) & MASK64, 0, sizeL).cpu().numpy()[:, :sizeL]
    return mc.trace_net_host(n, sizeL, nd, idx, base, HostEngine(), lists=lists, flip_q16=flip, adversary=word,
                             net=net)


def _same(got, want, what, slots=None):
    """rows, counts and the stored events of a device trace against the host's."""
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


def _trace(engine, name, idx=None, **kw):
    """The device trace of a case's keys through the form its lists call for."""
    n, nd, sizeL, base, inst, lists, adv, word, _ = CASES[name]
    idx = list(range(inst)) if idx is None else idx
    kw = {"cap": CAP, "adversary": adv, "net": word, **kw}
    if lists is None:
        return engine.montecarlo_trace_sampled_net(n, nd, base, idx, sizeL, **kw)
    return engine.montecarlo_trace_lists_net(n, nd, base, idx, np.array(lists)[idx], sizeL, **kw)


@pytest.mark.parametrize("name", CASES)
def test_every_reach_set_equals_the_host_specification(engine, name):
    want = reach_trace(name)
    assert int(want[1].max()) <= CAP
    _same(_trace(engine, name), want, name)


@pytest.mark.parametrize("flip", [1, 0x1000])
@pytest.mark.parametrize("name", SAMPLED)
def test_sampled_reach_sets_with_noise(engine, name, flip):
    _same(_trace(engine, name, flip_q16=flip), reach_trace(name, flip), f"{name} flip={flip:#x}")


@pytest.mark.parametrize("sizeL", [0, 3, 65])
@pytest.mark.parametrize("n", [1, 2, 3, 12, 15])
def test_small_grid_equals_the_host_specification(engine, n, sizeL):
    for nd in sorted({0, n - 1}):
        for net in NETS:
            got = engine.montecarlo_trace_sampled_net(n, nd, GRID_BASE, IDX, sizeL, cap=CAP, net=net)
            want = _host(engine, n, sizeL, nd, IDX, GRID_BASE, 0, None, net)
            assert int(want[1].max()) <= CAP
            _same(got, want, f"n={n} sizeL={sizeL} nd={nd} net={net:#x}")


@pytest.mark.parametrize("name", CASES)
def test_traced_rows_equal_the_decision_calls_rows_for_a_whole_batch(engine, name):
    n, nd, sizeL, base, _, lists, adv, word, _ = CASES[name]
    inst = 67
    if lists is None:
        rows, counts, _ = engine.montecarlo_trace_sampled_net(n, nd, base, list(range(inst)), sizeL, cap=4,
                                                              adversary=adv, net=word)
        want = engine.montecarlo_curve_sampled_net(n, nd, base, inst, [sizeL], adversary=adv, net=word)
    else:
        li = np.array(lists)[np.arange(inst) % len(lists)]   # the set's lists, repeated under 67 keys
        rows, counts, _ = engine.montecarlo_trace_lists_net(n, nd, base, list(range(inst)), li, sizeL, cap=4,
                                                            adversary=adv, net=word)
        want = engine.montecarlo_curve_lists_net(n, nd, base, li, [sizeL], adversary=adv, net=word)
    assert rows.cpu().numpy().tolist() == want.cpu().numpy().reshape(inst, -1).tolist(), name
    assert (counts[:, 1:] > 0).all() and not counts[:, 0].any()


def _guarded(engine, n, n_idx, cap, extra=64):
    """Three output tensors, each a view of the front of a GUARD-filled buffer
    with ``extra`` words behind it: (views, buffers)."""
    import torch
    shapes = ((n_idx, 4 + 5 * (n + 1)), (n_idx, n + 1), (n_idx, n + 1, cap, 2))
    bufs = [torch.full((int(np.prod(s)) + extra,), GUARD, dtype=torch.int32, device=engine.device) for s in shapes]
    return tuple(b[:int(np.prod(s))].view(s) for b, s in zip(bufs, shapes)), bufs


@pytest.mark.parametrize("name", [SAMPLED[1], LISTS[0]])
def test_net_zero_writes_what_the_trace_calls_write(engine, name):
    n, nd, sizeL, base, inst, lists, adv, _, _ = CASES[name]
    idx = list(range(inst))
    for flip in (0, 0x1000):
        for word in (0, None):
            out, bufs = _guarded(engine, n, inst, 64)
            if lists is None:
                got = engine.montecarlo_trace_sampled_net(n, nd, base, idx, sizeL, cap=64, flip_q16=flip,
                                                          adversary=adv, net=word, out=out)
                want = engine.montecarlo_trace_sampled(n, nd, base, idx, sizeL, cap=64, flip_q16=flip, adversary=adv,
                                                       out=_guarded(engine, n, inst, 64)[0])
            else:
                got = engine.montecarlo_trace_lists_net(n, nd, base, idx, np.array(lists), sizeL, cap=64,
                                                        flip_q16=flip, adversary=adv, net=word, out=out)
                want = engine.montecarlo_trace_lists(n, nd, base, idx, np.array(lists), sizeL, cap=64, flip_q16=flip,
                                                     adversary=adv, out=_guarded(engine, n, inst, 64)[0])
            for g, w in zip(got, want):   # every word, the guard pattern behind a rank's events included
                assert g.cpu().numpy().tolist() == w.cpu().numpy().tolist(), (name, flip, word)


def test_cap_above_at_and_below_a_ranks_event_count(engine):
    name = "n7-d2-L8-cmd-half"
    n = CASES[name][0]
    idx = [0, 1, 5]
    full = reach_trace(name)
    want = (full[0][idx], full[1][idx], [full[2][j] for j in idx])
    c = int(want[1][1].max())          # the busiest rank of slot 1
    assert c > 4 and int(want[1][want[1] > 0].min()) < c - 1   # some ranks end below every cap used
    for cap in (c + 1, c, c - 1):
        out, bufs = _guarded(engine, n, len(idx), cap)
        got = _trace(engine, name, idx=idx, cap=cap, out=out)
        _same(got, want, f"cap={cap}")
        counts, events = got[1].cpu().numpy(), got[2].cpu().numpy()
        for j in range(len(idx)):
            for r in range(n + 1):                      # behind each rank's stored events: untouched
                assert (events[j, r, min(int(counts[j, r]), cap):] == GUARD).all(), (cap, j, r)
        for b, t in zip(bufs, got):                     # behind the arrays: untouched
            assert (b[t.numel():] == GUARD).all()


def test_device_fed_match_count_limits_the_slots(engine):
    import torch
    name = "n7-d2-L8-quarter"
    n, nd, sizeL, base, _, _, adv, word, _ = CASES[name]
    n_idx = 16
    idx = list(range(n_idx))
    full = reach_trace(name)
    want = (full[0][:n_idx], full[1][:n_idx], full[2][:n_idx])
    dev_idx = torch.tensor(idx, dtype=torch.int64, device=engine.device)
    for m in (0, 3, 1000):
        lim = min(m, n_idx)
        out, bufs = _guarded(engine, n, n_idx, 256)
        n_match = torch.tensor([m], dtype=torch.int64, device=engine.device)
        got = engine.montecarlo_trace_sampled_net(n, nd, base, dev_idx, sizeL, cap=256, adversary=adv, net=word,
                                                  n_match=n_match, out=out)
        _same(got, want, f"n_match={m}", slots=range(lim))
        for t, b in zip(got, bufs):
            assert (t[lim:] == GUARD).all() and (b[t.numel():] == GUARD).all(), m


def test_a_value_past_w_at_a_q_position_gives_status_4_and_no_events(engine):
    import torch
    from montecarlo_cases import HOSTILE, hostile_lists
    mc = sub("montecarlo")
    case = next(c for c in HOSTILE if c["n"] == 3)
    n, nd, sizeL, base, w, net = 3, case["nDishonest"], case["sizeL"], case["base"], 4, 0x8000 | CMD
    li = np.array(np.broadcast_to(hostile_lists(case)[0], (5, n + 1, sizeL)))
    q = int(np.nonzero(li[2, 0] != li[2, 1])[0][0])
    li[2, 2, q] = w
    out = tuple(torch.full(s, GUARD, dtype=torch.int32, device=engine.device)
                for s in ((5, 4 + 5 * (n + 1)), (5, n + 1), (5, n + 1, 64, 2)))
    rows, counts, events = engine.montecarlo_trace_lists_net(n, nd, base, list(range(5)), li, sizeL, cap=64, out=out,
                                                             net=net)
    want = engine.montecarlo_curve_lists_net(n, nd, base, li, [sizeL], adversary=0xF, net=net).cpu().numpy()
    want = want.reshape(5, -1)
    assert rows.cpu().numpy().tolist() == want.tolist()
    assert want[2].tolist() == [0, 0, 0, mc.ST_RANGE] + [0] * (5 * (n + 1))
    assert not counts[2].any() and (events[2] == GUARD).all()
    assert (counts[[0, 1, 3, 4], 1:] > 0).all()


# ---- the front ends ----------------------------------------------------------------------------

E2E = dict(n=7, nd=2, sizeL=8, seed=0x4E47, idx=[3, 0, 17, 3])


def _texts(n, want):
    mc = sub("montecarlo")
    return [mc.format_trace(n, r, c, e) for r, c, e in zip(*want)]


def test_replay_equals_the_host_specification(engine):
    import torch
    mc = sub("montecarlo")
    n, nd, sizeL, seed, idx = (E2E[k] for k in ("n", "nd", "sizeL", "seed", "idx"))
    for net, adv, flip in ((0x4000, None, 0), (0x8000 | CMD, PRESETS["strip"], 0x1000), (0, None, 0), (None, None, 9)):
        want = mc.trace_net_host(n, sizeL, nd, idx, seed, HostEngine(), flip_q16=flip, adversary=adv, net=net)
        for indices in (idx, torch.tensor(idx, dtype=torch.int64, device=engine.device)):
            got = mc.replay(n, sizeL, nd, indices, seed, engine, flip_q16=flip, adversary=adv, net=net)
            assert got["indices"] == idx and set(got) == {"indices", "rows", "counts", "events"}
            assert got["rows"].tolist() == want[0].tolist() and got["counts"].tolist() == want[1].tolist()
            assert _texts(n, (got["rows"], got["counts"], got["events"])) == _texts(n, want)
            for j in range(len(idx)):
                assert mc.trace_events(got["counts"], got["events"], j) == want[2][j]


@pytest.mark.parametrize("extra,net,curve", [(["--drop", "0x4000"], 0x4000, None),
                                             (["--drop", "0x8000:cmd"], 0x8000 | CMD, None),
                                             (["--drop", "0x8000:cmd", "--curve", "3,16", "--adversary", "strip"],
                                              0x8000 | CMD, [3, 8, 16]),
                                             ([], 0, None)], ids=["drop", "cmd", "curve", "perfect"])
def test_cli_replay_prints_the_host_transcripts(engine, capsys, extra, net, curve):
    mc = sub("montecarlo")
    n, nd, sizeL, seed, idx = (E2E[k] for k in ("n", "nd", "sizeL", "seed", "idx"))
    argv = [str(sizeL), str(nd), "--parties", str(n), "--seed", str(seed), "--replay", ",".join(map(str, idx))] + extra
    assert sub("tfg").main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    adv = PRESETS["strip"] if "--adversary" in extra else None
    want = []
    for c in curve or [sizeL]:
        host = mc.trace_net_host(n, c, nd, idx, seed, HostEngine(), adversary=adv, net=net)
        for i, text in zip(idx, _texts(n, host)):
            want += [f"sizeL={c} run {i}" if curve else f"run {i}"] + text.splitlines()
    assert lines == want
    if net & CMD:
        assert any("no packet arrived" in l for l in lines) and any("loses in flight" in l for l in lines)
