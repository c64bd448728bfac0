"""The run transcript without a GPU: the exports, the
argument checks of the two C entry points and their order (through a null
ctx), the host specification montecarlo.trace_host against run_host and
against its own rows, the verdicts and actions the hostile sets reach, the
formatter against a golden text, the CLI's --explain, and the static resources
of the new kernels read from the cross-compiled library."""
import collections
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, sub
from kd_util import kernel_descriptors
from montecarlo_cases import HOSTILE, hostile_lists
from test_montecarlo_adversary import HostEngine

REFERENCE, STRIP, ALL_FIVE = 0xF, 0x100C, 0x1F
SYMBOLS = ("qba_montecarlo_trace_sampled", "qba_montecarlo_trace_lists")


def test_symbols_are_exported_and_bound():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES
        assert getattr(lib, name).argtypes == lib_mod.SIGNATURES[name]
    eng = sub("engine").Engine
    assert eng.TRACE_CAP_MAX == 4096 == sub("montecarlo").TRACE_CAP_MAX
    assert callable(eng.montecarlo_trace_sampled) and callable(eng.montecarlo_trace_lists)


def _calls(lib):
    """name -> f(**arguments away from a valid call): the entry point with a null ctx"""
    ok = dict(n=7, idx=1, n_idx=4, count=60, nd=2, adv=REFERENCE, flip=0, cap=16, out=1)

    def sampled(**kw):
        a = {**ok, **kw}
        p = C.c_void_p(64)   # never dereferenced: every refusal comes before the device is looked at
        return lib.qba_montecarlo_trace_sampled(None, a["n"], 0, p if a["idx"] else None, a["n_idx"], None, a["count"],
                                                a["nd"], a["adv"], a["flip"], a["cap"], p if a["out"] else None, p,
                                                p, None)

    def lists(**kw):
        a = {**ok, **kw}
        p = C.c_void_p(64)
        return lib.qba_montecarlo_trace_lists(None, a["n"], 0, p if a["idx"] else None, a["n_idx"], None, a["count"],
                                              a["nd"], a["adv"], a["flip"], a["cap"], None, 64, 8 * 64, p,
                                              p if a["out"] else None, p, None)
    return {"sampled": sampled, "lists": lists}


def test_every_argument_check_and_its_order_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()

    def refused(rc, needle):
        msg = lib.qba_last_error().decode()
        assert rc == lib_mod.QBA_EINVAL and needle in msg, (rc, msg, needle)

    bad = [("n", 16, "n_parties"), ("count", 1 << 31, "count"), ("flip", 65536, "flip_q16"),
           ("nd", 8, "n_dishonest"), ("adv", 0x2F, "adv"), ("n_idx", -1, "n_idx"), ("cap", 0, "cap"),
           ("out", 0, "events is NULL")]
    for name, f in _calls(lib).items():
        refused(f(), "ctx is NULL")                       # only the device is missing
        refused(f(n_idx=0, idx=0, out=0), "ctx is NULL")  # nothing to trace needs no pointer
        refused(f(cap=4096, flip=65535, nd=7, count=(1 << 31) - 1), "ctx is NULL")
        for key, value, needle in bad:
            refused(f(**{key: value}), needle)
        refused(f(n=0), "n_parties")
        refused(f(nd=-1), "n_dishonest")
        refused(f(adv=0), "adv")
        refused(f(idx=0), "idx is NULL")
        refused(f(cap=4097), "cap")
        # the order: every argument bad, then mended one at a time from the front
        wrong = {key: value for key, value, _ in bad}
        for key, _, needle in bad:
            refused(f(**wrong), needle)
            del wrong[key]
        refused(f(n_idx=-1, idx=0), "n_idx")              # n_idx before the pointer it sizes


def _host(n, sizeL, nd, idx, base, word, **kw):
    return sub("montecarlo").trace_host(n, sizeL, nd, idx, base, HostEngine(), adversary=word, **kw)


GRID = [(n, nd, word) for n in (3, 7) for nd in sorted({0, 1, n // 3}) for word in (REFERENCE, STRIP)]
BASE, KEYS, SIZEL = 0xAD0, 12, 8


@pytest.fixture(scope="module")
def traces():
    """trace_host of KEYS keys at every grid point, computed once and left unchanged."""
    out = {}
    for n, nd, word in GRID:
        rows, counts, events = _host(n, SIZEL, nd, range(KEYS), BASE, word)
        rows.setflags(write=False)
        counts.setflags(write=False)
        out[n, nd, word] = rows, counts, events
    return out


@pytest.mark.parametrize("n,nd,word", GRID)
def test_trace_host_rows_equal_run_host(traces, n, nd, word):
    mc = sub("montecarlo")
    rows = traces[n, nd, word][0]
    assert np.array_equal(rows, mc.run_host(n, SIZEL, nd, KEYS, BASE, HostEngine(), adversary=word))
    assert not rows[:, 3].any()
    if word == REFERENCE:   # ... and without a policy
        assert np.array_equal(rows, mc.run_host(n, SIZEL, nd, KEYS, BASE, HostEngine()))
        assert np.array_equal(rows, _host(n, SIZEL, nd, range(KEYS), BASE, None)[0])


@pytest.mark.parametrize("n,nd,word", GRID)
def test_events_add_up_to_the_row(traces, n, nd, word):
    mc = sub("montecarlo")
    rows, counts, events = traces[n, nd, word]
    for row, cnt, per_rank in zip(rows, counts, events):
        assert cnt[0] == 0 and per_rank[0] == []
        for r in range(1, n + 1):
            ev = [(mc.event_fields(h), p) for h, p in per_rank[r]]
            assert len(ev) == cnt[r]
            dec, vi, accept, reject, sent = (int(x) for x in row[4 + 5 * r:9 + 5 * r])
            recv = [f for f, _ in ev if f["kind"] == mc.EV_RECV]
            send = [f for f, _ in ev if f["kind"] == mc.EV_SEND]
            assert sum(f["code"] in (0, 4, 5) for f in recv) == accept
            assert sum(f["code"] in (1, 2, 3) for f in recv) == reject
            assert sum(f["slot"] < 30 for f in send) == sent
            assert sum(f["code"] == 0 for f in recv) == bin(vi).count("1")
            last, pkt = ev[-1]
            assert last == {"kind": mc.EV_DECIDE, "round": 0, "peer": 0, "slot": 0, "code": 0,
                            "len": bin(vi).count("1")} and pkt == dec & 0xFFFFFFFF
            assert all(f["kind"] != mc.EV_DECIDE for f, _ in ev[:-1])
            assert all(h >> 26 == 0 for h, _ in per_rank[r])
            honest = not (int(row[1]) >> r) & 1
            assert all((f["code"] == mc.EV_HONEST) == (honest or r == 1) for f in send)
            if r == 1:
                assert [f["peer"] for f in send] == list(range(2, n + 1)) and not recv
            else:
                assert recv[0]["peer"] == 1 and recv[0]["round"] == 0 and recv[0]["slot"] == 0


def test_lists_follow_their_indices_and_flips_follow_the_key():
    mc = sub("montecarlo")
    n, nd, sizeL = 7, 2, 8
    eng = HostEngine()
    idx = [5, 0, 5, (1 << 40) + 3]
    li = np.stack([mc._host_lists(eng.sample(n, BASE + i, 0, sizeL), sizeL) for i in idx])
    for flip in (0, 0x1000):
        a = _host(n, sizeL, nd, idx, BASE, STRIP, flip_q16=flip)
        b = _host(n, sizeL, nd, idx, BASE, STRIP, flip_q16=flip, lists=li)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert a[2][0] == a[2][2] and np.array_equal(a[0][0], a[0][2])
        assert np.array_equal(a[0], np.stack([mc.run_host(n, sizeL, nd, 1, BASE + i, eng, flip_q16=flip,
                                                          adversary=STRIP)[0] for i in idx]))
    wrap = _host(n, sizeL, nd, [0, 3], (1 << 64) - 2, STRIP)
    assert np.array_equal(wrap[0][1], _host(n, sizeL, nd, [1], 0, STRIP)[0][0])


def test_hostile_sets_reach_every_verdict_and_every_action():
    """Counted on the host specification alone: the reference's traitor on every
    hostile set, and on one of them the policy that may draw all five actions."""
    mc = sub("montecarlo")
    codes, actions, slots = collections.Counter(), collections.Counter(), collections.Counter()

    def count(case, word, keys):
        li = hostile_lists(case)[:keys]
        _, _, events = _host(case["n"], case["sizeL"], case["nDishonest"], range(len(li)), case["base"], word,
                             lists=li)
        for inst in events:
            for per_rank in inst:
                for head, _ in per_rank:
                    f = mc.event_fields(head)
                    if f["kind"] == mc.EV_RECV:
                        codes[f["code"]] += 1
                    elif f["kind"] == mc.EV_SEND:
                        actions[f["code"]] += 1
                        slots[f["slot"]] += 1
    for case in HOSTILE:
        count(case, REFERENCE, 4)
    count(next(c for c in HOSTILE if c["n"] == 7), ALL_FIVE, 4)
    assert all(codes[c] > 0 for c in range(6)) and set(codes) == set(range(6)), codes
    assert all(actions[a] > 0 for a in (0, 1, 2, 3, 4, mc.EV_HONEST)), actions
    assert slots[mc.EV_SLOT_MUTED] > 0 and slots[1] > 0 and slots[mc.EV_SLOT_FULL] == 0, slots


def test_packet_word_and_head_fields():
    mc, PRef = sub("montecarlo"), sub("countmode").PRef
    assert mc.packet_word(PRef(5), 5, set()) == 0x55
    assert mc.packet_word(PRef(5), 3, {(5, 2), (5, 0)}) == 3 | 5 << 4 | 5 << 9 | 0b101 << 16
    assert mc.packet_word(PRef(None), 3, {(), (5, 2)}) == 3 | 1 << 8 | 5 << 9 | 1 << 13 | 1 << 18
    assert mc.packet_word(PRef(None), 0, {()}) == 1 << 8 | 1 << 13
    head = mc.event_head(mc.EV_SEND, 16, 15, 31, 7, 17)
    assert mc.event_fields(head) == {"kind": 2, "round": 16, "peer": 15, "slot": 31, "code": 7, "len": 17}
    assert head < 1 << 26


FORMAT_CASES = {"honest": (3, 0, [0], REFERENCE), "failed": (7, 2, [3], REFERENCE)}


@pytest.mark.parametrize("name", FORMAT_CASES)
def test_format_trace_against_the_golden_text(name):
    mc = sub("montecarlo")
    n, nd, idx, word = FORMAT_CASES[name]
    rows, counts, events = _host(n, SIZEL, nd, idx, 2768, word)
    assert bool(rows[0, 0]) == (name == "honest")
    text = mc.format_trace(n, rows[0], counts[0], events[0])
    assert text + "\n" == (GOLDEN / f"trace_{name}.txt").read_text()
    # the device layout, cut to 5 events a rank, reports the rest as a count
    cap = 5
    dev = np.zeros((n + 1, cap, 2), np.uint32)
    for r, ev in enumerate(events[0]):
        dev[r, :min(len(ev), cap)] = np.array(ev[:cap], np.uint32).reshape(-1, 2)
    cut = mc.format_trace(n, rows[0], counts[0], dev.view(np.int32)).splitlines()
    full = text.splitlines()
    assert cut[0] == full[0] and all(l in full or "more event" in l for l in cut)
    for r in range(1, n + 1):
        more = int(counts[0, r]) - cap
        assert (f"] ... {more} more event{'' if more == 1 else 's'} counted, not stored" in "\n".join(cut)) == (more > 0)


def test_cli_parses_explain():
    tfg = sub("tfg")
    base = ["8", "2", "--parties", "7", "--runs", "10"]
    a = tfg._args(base + ["--explain", "3"])
    assert a.explain == 3 and a.failures == 3
    assert tfg._args(base + ["--explain", "3", "--failures", "9"]).failures == 3
    assert vars(tfg._args(base + ["--explain", "0"])) == vars(tfg._args(base))
    assert vars(tfg._args(base + ["--explain", "0", "--failures", "2"])) == vars(tfg._args(base + ["--failures", "2"]))
    for extra in (["--fused"], ["--curve", "50,100"], ["--sweep", "1,2:strip"], ["--flip", "16"],
                  ["--adversary", "strip"], ["--tables"]):
        assert tfg._args(base + extra + ["--explain", "2"]).explain == 2
    for bad in (["8", "2", "--explain", "2"], base + ["--explain", "-1"], base + ["--explain", "x"]):
        with pytest.raises(SystemExit):
            tfg._args(bad)


@pytest.fixture(scope="module")
def kds():
    return kernel_descriptors(Path(sub("_lib").LIB_PATH))


def test_trace_kernels_use_no_scratch_no_static_lds_and_a_stated_vgpr_bound(kds):
    new = {k: v for k, v in kds.items() if "qba_k_trace_" in k}
    assert sum("17qba_k_trace_listsE" in k for k in new) == 1
    for n in range(1, 16):   # every sampler of the n: the closed form's up to 11
        assert sum(k.startswith(f"_Z19qba_k_trace_sampledILi{n}E") for k in new) == (3 if n <= 11 else 2), n
    assert len(new) == 1 + 11 * 3 + 4 * 2   # one instantiation serves flip = 0 and flip > 0
    for k, v in new.items():
        # 128 VGPRs keep four waves a SIMD, the occupancy the launch shape assumes; the
        # two n = 15 kernels may take 136 (three waves a SIMD)
        bound = 136 if k.startswith("_Z19qba_k_trace_sampledILi15E") else 128
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= bound, (k, v)
    lists = next(v for k, v in new.items() if "qba_k_trace_lists" in k)
    assert lists["vgprs"] <= 64
    # the kernels that were there stay findable by the names the sibling tests use
    for name in new:
        assert not any(s in name for s in ("qba_k_protocol", "qba_k_mc_"))
    lib = sub("_lib").lib()
    for n in range(1, 16):   # compiled for the wave count of the single-count decision kernels
        waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
        assert lib.qba_montecarlo_shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
        samp = 2 if n <= 11 else 1
        assert any(k.startswith(f"_Z19qba_k_trace_sampledILi{n}ELi{samp}ELi{waves.value}E") for k in new), n
