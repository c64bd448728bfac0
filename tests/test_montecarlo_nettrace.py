"""The transcript on a lossy network without a GPU:
the exports, the argument checks of the two C entry points and their order
(through a null ctx), the host specification montecarlo.trace_net_host against
run_host(..., net=) and, at net = 0, against trace_host, its events against the
rows and against what the observer of tests/montecarlo_net_cases.py sees, the
lost events the reach sets were chosen for, the formatter against a golden
text, the CLI's --replay, and the static resources of the new kernels read
from the cross-compiled library."""
import collections
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, sub
from kd_util import kernel_descriptors
from montecarlo_net_cases import CMD, REACH, observing, reach_rows
from montecarlo_nettrace_cases import CASES, DUP, case_rows, fields, reach_trace
from test_montecarlo_adversary import BAD_WORDS, HostEngine, PRESETS
from test_montecarlo_net import BAD_NET, GOOD_NET

REFERENCE = 0xF
SYMBOLS = ("qba_montecarlo_trace_sampled_net", "qba_montecarlo_trace_lists_net")


def test_symbols_are_exported_and_bound():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES
        assert getattr(lib, name).argtypes == lib_mod.SIGNATURES[name]
        # the trace call's arguments, then net
        assert lib_mod.SIGNATURES[name] == lib_mod.SIGNATURES[name[:-4]] + [C.c_uint32]
    header = (Path(__file__).resolve().parent.parent / "include" / "qba.h").read_text()
    assert all(f"QBA_API int {name}(" in header for name in SYMBOLS)
    assert "#define QBA_EV_SLOT_LOST 29u" in header and "#define QBA_EV_NO_PACKET 6u" in header
    mc, eng = sub("montecarlo"), sub("engine").Engine
    assert mc.EV_SLOT_LOST == 29 and mc.EV_NO_PACKET == 6
    assert callable(eng.montecarlo_trace_sampled_net) and callable(eng.montecarlo_trace_lists_net)
    assert len(mc.VERDICTS) == 6   # code 6 is rendered on its own


def _calls(lib):
    """name -> f(**arguments away from a valid call): the entry point with a null ctx"""
    ok = dict(n=7, idx=1, n_idx=4, count=60, nd=2, adv=REFERENCE, net=0x2000, flip=0, cap=16, out=1)

    def sampled(**kw):
        a = {**ok, **kw}
        p = C.c_void_p(64)   # never dereferenced: every refusal comes before the device is looked at
        return lib.qba_montecarlo_trace_sampled_net(None, a["n"], 0, p if a["idx"] else None, a["n_idx"], None,
                                                    a["count"], a["nd"], a["adv"], a["flip"], a["cap"],
                                                    p if a["out"] else None, p, p, None, a["net"])

    def lists(**kw):
        a = {**ok, **kw}
        p = C.c_void_p(64)
        return lib.qba_montecarlo_trace_lists_net(None, a["n"], 0, p if a["idx"] else None, a["n_idx"], None,
                                                  a["count"], a["nd"], a["adv"], a["flip"], a["cap"], None, 64, 8 * 64,
                                                  p, p if a["out"] else None, p, None, a["net"])
    return {"sampled": sampled, "lists": lists}


def test_every_argument_check_and_its_order_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()

    def refused(rc, needle):
        msg = lib.qba_last_error().decode()
        assert rc == lib_mod.QBA_EINVAL and needle in msg, (rc, msg, needle)

    bad = [("n", 16, "n_parties"), ("count", 1 << 31, "count"), ("flip", 65536, "flip_q16"),
           ("nd", 8, "n_dishonest"), ("adv", 0x2F, ": adv"), ("net", 1 << 17, ": net"), ("n_idx", -1, "n_idx"),
           ("cap", 0, "cap"), ("out", 0, "events is NULL")]
    for name, f in _calls(lib).items():
        refused(f(), "ctx is NULL")                       # only the device is missing
        refused(f(n_idx=0, idx=0, out=0), "ctx is NULL")  # nothing to trace needs no pointer
        refused(f(cap=4096, flip=65535, nd=7, count=(1 << 31) - 1, net=0xFFFF | CMD), "ctx is NULL")
        for key, value, needle in bad:
            refused(f(**{key: value}), needle)
        refused(f(n=0), "n_parties")
        refused(f(nd=-1), "n_dishonest")
        refused(f(adv=0), ": adv")
        refused(f(idx=0), "idx is NULL")
        refused(f(cap=4097), "cap")
        for word, field in BAD_NET.items():
            rc = f(net=word)
            refused(rc, ": net")
            refused(rc, field)
        for word in GOOD_NET:
            refused(f(net=word), "ctx is NULL")
        for bad_adv in BAD_WORDS:                          # adv is looked at before net ...
            refused(f(adv=bad_adv, net=CMD), ": adv")
        refused(f(net=CMD, idx=0), ": net")                # ... and net before idx
        refused(f(net=CMD, n_idx=-1), ": net")
        # the order: every argument bad, then mended one at a time from the front
        wrong = {key: value for key, value, _ in bad}
        for key, _, needle in bad:
            refused(f(**wrong), needle)
            del wrong[key]
        refused(f(n_idx=-1, idx=0), "n_idx")              # n_idx before the pointer it sizes


# ---- trace_net_host against the host model -------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_rows_equal_run_host_on_the_network(name):
    mc = sub("montecarlo")
    rows, counts, events = reach_trace(name)
    assert len(rows) == CASES[name][4]   # every key of the set
    want = reach_rows(mc, name) if name in REACH else case_rows(name)
    assert np.array_equal(rows, want) and not rows[:, 3].any()


@pytest.mark.parametrize("name", REACH)
def test_net_zero_is_trace_host(name):
    mc = sub("montecarlo")
    n, nd, sizeL, base, inst, lists, adv, _, _ = REACH[name]
    keys = range(min(inst, 6))
    want = mc.trace_host(n, sizeL, nd, keys, base, HostEngine(), lists=lists, adversary=adv)
    for word in (0, None):
        got = mc.trace_net_host(n, sizeL, nd, keys, base, HostEngine(), lists=lists, adversary=adv, net=word)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_the_recording_party_at_net_zero_records_what_trace_party_records():
    """TraceNetParty itself (not the shortcut of trace_net_host) on the perfect network."""
    mc = sub("montecarlo")
    n, nd, sizeL, base, _, _, adv, _, _ = REACH["n7-d2-L8-quarter"]
    for key in range(4):
        sinks = []
        for base_cls in (mc.TraceNetParty, mc.TraceParty):
            sink = {}
            cls = type("Rec", (base_cls,), {"adv": adv, "sink": sink})
            mc.run_host(n, sizeL, nd, 1, base + key, HostEngine(), party_cls=cls)
            sinks.append({r: p.events for r, p in sink.items()})
        assert sinks[0] == sinks[1] and any(sinks[0].values())


@pytest.fixture(scope="module")
def observed():
    """name -> what observing() records on the keys of the reach set"""
    mc = sub("montecarlo")
    out = {}
    assert set(REACH) <= set(CASES)
    for name in CASES:
        seen = {}
        case_rows(name, party_cls=observing(mc, seen))
        out[name] = seen
    return out


@pytest.mark.parametrize("name", CASES)
def test_events_add_up_to_the_row_and_to_what_the_observer_sees(observed, name):
    mc = sub("montecarlo")
    n, nd, _, base, inst, _, _, word, _ = CASES[name]
    rows, counts, events = reach_trace(name)
    seen = observed[name]
    for j in range(inst):
        assert counts[j, 0] == 0 and events[j][0] == []
        for r in range(1, n + 1):
            ev = fields(events[j][r])
            assert len(ev) == counts[j, r] and all(h >> 26 == 0 for h, _ in events[j][r])
            dec, vi, accept, reject, sent = (int(x) for x in rows[j, 4 + 5 * r:9 + 5 * r])
            recv = [f for f, _ in ev if f["kind"] == mc.EV_RECV]
            send = [f for f, _ in ev if f["kind"] == mc.EV_SEND]
            assert sum(f["code"] in (0, 4, 5) for f in recv) == accept
            assert sum(f["code"] in (1, 2, 3) for f in recv) == reject
            assert sum(f["slot"] < 30 for f in send) == sent
            last, pkt = ev[-1]
            assert last == {"kind": mc.EV_DECIDE, "round": 0, "peer": 0, "slot": 0, "code": 0,
                            "len": bin(vi).count("1")} and pkt == dec & 0xFFFFFFFF
            for e in range(nd + 2):   # the lost sends of every epoch
                lost = sum(f["slot"] == mc.EV_SLOT_LOST and f["round"] == e for f in send)
                assert lost == seen["links"].get((base + j, r, e), [0, 0])[1], (j, r, e)
            if not word & CMD:
                assert all(f["slot"] != mc.EV_SLOT_LOST for f in send if r == 1)
            # a lost packet takes no slot: the delivered ones of a (round, destination) fill slots 0, 1, ...
            nxt = collections.Counter()
            for f in send:
                if r > 1 and f["slot"] < mc.EV_SLOT_LOST:
                    assert f["slot"] == nxt[f["round"], f["peer"]]
                    nxt[f["round"], f["peer"]] += 1
            nopkt = [(f, p) for f, p in ev if f["kind"] == mc.EV_RECV and f["code"] == mc.EV_NO_PACKET]
            if (base + j, r) in seen["cmd_lost"]:
                want = {"kind": mc.EV_RECV, "round": 0, "peer": 1, "slot": 0, "code": mc.EV_NO_PACKET, "len": 0}
                assert nopkt == [(want, 0)]
                # no other event of the commander's epoch (the closing DECIDE carries round 0 by definition)
                assert [f for f, _ in ev[:-1] if f["round"] == 0] == [want]
            else:
                assert not nopkt
                if r > 1:
                    assert recv[0]["peer"] == 1 and recv[0]["round"] == 0 and recv[0]["code"] != mc.EV_NO_PACKET
    assert sum(len(seen["cmd_lost"]) for seen in observed.values()) > 0


def _lost_sends(name):
    """(key index, rank, fields, pkt, seq, the slot it would have had, the next
    delivered send to the same (round, destination) or None) of every lost
    SEND of a reach set"""
    mc = sub("montecarlo")
    n = CASES[name][0]
    _, _, events = reach_trace(name)
    for j, inst in enumerate(events):
        for r in range(1, n + 1):
            send = [(f, p) for f, p in fields(inst[r]) if f["kind"] == mc.EV_SEND]
            seq, delivered = collections.Counter(), collections.Counter()
            for i, (f, p) in enumerate(send):
                if f["slot"] == mc.EV_SLOT_MUTED:
                    continue
                link = (f["round"], f["peer"])
                if f["slot"] == mc.EV_SLOT_LOST:
                    after = next((g for g, _ in send[i + 1:] if (g["round"], g["peer"]) == link and
                                  g["slot"] < mc.EV_SLOT_LOST), None)
                    yield j, r, f, p, seq[link], delivered[link], after
                else:
                    delivered[link] += 1
                seq[link] += 1


def test_a_lost_first_send_leaves_its_slot_to_the_second():
    pairs = 0
    for name in DUP:
        for j, r, f, p, seq, slot, after in _lost_sends(name):
            if r > 1 and after is not None:   # the next delivered packet of the link takes the lost one's slot
                assert after["slot"] == slot
                pairs += seq == 0
    assert pairs > 0


def test_the_reach_sets_lose_what_they_were_chosen_for(observed):
    """On the host model, so that the GPU comparison cannot pass vacuously."""
    mc = sub("montecarlo")
    got = collections.Counter()
    for name in CASES:
        n, _, _, base, _, _, _, _, _ = CASES[name]
        rows, _, events = reach_trace(name)
        for j, r, f, p, seq, _, after in _lost_sends(name):
            dishonest = (int(rows[j, 1]) >> r) & 1
            got["honest"] += f["code"] == mc.EV_HONEST and r > 1 and not dishonest
            got["mutated"] += f["code"] in (1, 2, 3) and bool(dishonest)
            got["seq4"] += seq >= 4
            got["cmd"] += r == 1
        got["mutated_lost"] += observed[name]["mutated_lost"]
        for key, r in observed[name]["cmd_lost"]:
            j = key - base
            ev = fields(events[j][r])
            assert ev[0][0]["code"] == mc.EV_NO_PACKET
            if not (int(rows[j, 1]) >> r) & 1:
                got["cmd_relayed" if ev[-1][0]["len"] else "cmd_empty"] += 1
                assert bool(ev[-1][0]["len"]) == bool(rows[j, 5 + 5 * r])
    for what in ("honest", "mutated", "mutated_lost", "seq4", "cmd", "cmd_empty", "cmd_relayed"):
        assert got[what] > 0, (what, dict(got))


# ---- the formatter and the CLI ----------------------------------------------------------------

FORMAT_CASE = ("n4-d1-L16-cmd-most", 0)   # the reach set and the position among its keys with a lost commander packet


def format_case():
    """(n, row, counts, events) of the golden transcript"""
    mc = sub("montecarlo")
    name, which = FORMAT_CASE
    n = REACH[name][0]
    rows, counts, events = reach_trace(name)
    hit = [j for j in range(len(rows))
           if any(f["kind"] == mc.EV_RECV and f["code"] == mc.EV_NO_PACKET for r in range(2, n + 1)
                  for f, _ in fields(events[j][r]))
           and any(f["kind"] == mc.EV_SEND and f["slot"] == mc.EV_SLOT_LOST for f, _ in fields(events[j][1]))
           and any(f["kind"] == mc.EV_SEND and f["slot"] == mc.EV_SLOT_LOST for r in range(2, n + 1)
                   for f, _ in fields(events[j][r]))]
    j = hit[which]
    return n, rows[j], counts[j], events[j]


def test_format_trace_against_the_golden_text():
    mc = sub("montecarlo")
    n, row, counts, events = format_case()
    text = mc.format_trace(n, row, counts, events)
    assert text + "\n" == (GOLDEN / "nettrace_lossy.txt").read_text()
    assert "loses in flight v=" in text and "no packet arrived" in text
    assert any(l.startswith("[1 -> ") or l.startswith("[B1 -> ") for l in text.splitlines() if "loses in flight" in l)
    assert any("<- " in l and l.endswith("round 0: no packet arrived") for l in text.splitlines())
    # the device layout renders the same
    cap = int(max(counts))
    dev = np.zeros((n + 1, cap, 2), np.uint32)
    for r, ev in enumerate(events):
        if ev:
            dev[r, :len(ev)] = np.array(ev, np.uint32).reshape(-1, 2)
    assert mc.format_trace(n, row, counts, dev.view(np.int32)) == text


def test_a_lost_send_of_a_traitor_keeps_its_action_suffix():
    mc = sub("montecarlo")
    head = mc.event_head(mc.EV_SEND, 2, 5, mc.EV_SLOT_LOST, mc.ACT_CLEAR_P if hasattr(mc, "ACT_CLEAR_P") else 2, 2)
    row = np.zeros(4 + 5 * 8, np.int32)
    row[1] = 1 << 3
    ev = [[] for _ in range(8)]
    ev[3] = [(head, 3 | 1 << 8)]
    text = mc.format_trace(7, row, [0, 0, 0, 1, 0, 0, 0, 0], ev)
    assert text.splitlines()[1] == "[B3 -> 5] round 2: loses in flight v=3, P cleared, 2 lists (action: clear P)"


def test_cli_parses_replay_and_refuses_what_it_is_not_built_for(capsys):
    tfg = sub("tfg")
    base = ["8", "2", "--parties", "7", "--seed", "5"]
    a = tfg._args(base + ["--replay", "3"])
    assert a.replay == [3] and a.runs is None and a.drop is None and a.curve is None
    a = tfg._args(base + ["--replay", "7,0x10,3,3", "--drop", "0x2000:cmd", "--flip", "9", "--adversary", "strip",
                          "--curve", "3,50"])
    assert a.replay == [7, 16, 3, 3] and a.drop == 0x12000 and a.flip == 9 and a.adversary == PRESETS["strip"]
    assert a.curve == [3, 8, 50]
    assert tfg._args(base + ["--replay", str((1 << 64) - 1)]).replay == [(1 << 64) - 1]
    assert tfg._args(base + ["--runs", "4"]).replay is None
    refused = {"--runs": ["--runs", "4"], "--collude": ["--collude", "late"], "--sweep": ["--sweep", "1,2"],
               "--grid": ["--grid", "2@0x100"], "--tables": ["--tables"], "--explain": ["--explain", "2"]}
    for flag, extra in refused.items():
        with pytest.raises(SystemExit):
            tfg._args(base + ["--replay", "3"] + extra)
        err = capsys.readouterr().err
        assert "--replay: not with" in err and flag in err.split("--replay: not with")[1].split("(")[0], (flag, err)
    for bad, needle in ((["8", "2", "--replay", "3"], "--replay needs --seed"),
                        (base + ["--replay", "x"], "--replay"), (base + ["--replay", ""], "--replay"),
                        (base + ["--replay", "-1"], "--replay"), (base + ["--replay", str(1 << 64)], "--replay"),
                        (base + ["--replay", "3", "--drop", "0:cmd"], "--drop"),
                        (base + ["--replay", "3", "--failures", "2"], "--failures"),
                        (base + ["--replay", "3", "--tally"], "--tally")):
        with pytest.raises(SystemExit):
            tfg._args(bad)
        assert needle in capsys.readouterr().err, bad
    # the flags that --replay lets stand without --runs still need one of the two
    for extra in (["--drop", "1"], ["--flip", "3"], ["--adversary", "strip"], ["--curve", "3,8"]):
        with pytest.raises(SystemExit):
            tfg._args(["8", "2"] + extra)
        assert "needs --runs" in capsys.readouterr().err


def test_replay_and_the_existing_refusals_stand():
    mc = sub("montecarlo")
    with pytest.raises(TypeError):
        mc.replay(3, 8, 1, [0], 0, None, coalition=0x1)
    with pytest.raises(mc.QbaError):
        mc.replay(3, 8, 1, [0], 0, None, net=CMD)
    with pytest.raises(ValueError, match="not built for a lossy network"):
        mc.run(3, 8, 1, 4, 0, None, path="fused", net=0x2000, explain=4, failures=4)


# ---- the code objects --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kds():
    return kernel_descriptors(Path(sub("_lib").LIB_PATH))


def test_nettrace_kernels_use_no_scratch_no_static_lds_and_a_stated_vgpr_bound(kds):
    new = {k: v for k, v in kds.items() if "qba_k_nettrace_" in k}
    assert sum("20qba_k_nettrace_listsE" in k for k in new) == 1
    for n in range(1, 16):   # every sampler of the n: the closed form's up to 11
        assert sum(k.startswith(f"_Z22qba_k_nettrace_sampledILi{n}E") for k in new) == (3 if n <= 11 else 2), n
    assert len(new) == 1 + 11 * 3 + 4 * 2
    for k, v in new.items():
        # 128 VGPRs keep four waves a SIMD, the occupancy the launch shape assumes (the bound the
        # trace kernels are held to); the n = 15 kernels may take 136, as theirs (three waves a SIMD)
        bound = 136 if k.startswith("_Z22qba_k_nettrace_sampledILi15E") else 128
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= bound, (k, v)
    lists = next(v for k, v in new.items() if "qba_k_nettrace_lists" in k)
    assert lists["vgprs"] <= 64
    for name in new:   # none is collected by the names the sibling tests use
        assert not any(s in name for s in ("qba_k_trace_", "qba_k_mc_", "qba_k_protocol", "qba_k_grid_", "_adv"))
    lib = sub("_lib").lib()
    for n in range(1, 16):   # compiled for the wave count of the single-count decision kernels
        waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
        assert lib.qba_montecarlo_shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
        samp = 2 if n <= 11 else 1
        assert any(k.startswith(f"_Z22qba_k_nettrace_sampledILi{n}ELi{samp}ELi{waves.value}E") for k in new), n
