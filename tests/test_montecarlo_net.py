"""Lossy links without a GPU: the network word's
checks from Python and through the two C entry points, the loss function
montecarlo.net_lost against a direct Philox evaluation, the host model
montecarlo.NetParty at net = 0 against the unchanged path, the events the model
reaches on the recorded reach sets (tests/montecarlo_net_cases.py, shared with
tests/test_gpu_montecarlo_net.py, which holds both kernels to the host model on
them), `sent` against the packets an observer sees handed over, and the static
resources of the lossy-network kernels read from the cross-compiled library."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from conftest import sub
from kd_util import kernel_descriptors
from montecarlo_net_cases import CMD, EVENTS, REACH, observing, reach_events, reach_rows
from oracle_engine import OracleEngine
from test_montecarlo_adversary import BAD_WORDS, PRESETS

GOOD_NET = [0, 1, 0x2000, 0xFFFF, 1 | CMD, 0x8000 | CMD, 0xFFFF | CMD]
BAD_NET = {  # word -> what the message names
    CMD: "cmd", 1 << 17: "reserved", 1 << 18 | 5: "reserved", 1 << 24 | CMD | 1: "reserved", 1 << 31: "reserved",
    0xFFFE0000: "reserved", 0x20001: "reserved",
}


def test_builder_parser_and_checks():
    mc = sub("montecarlo")
    assert mc.NET_TAG == 0x4E455457 and mc.NET_TAG not in (0, 1, mc.CTR_TAG, mc.NOISE_TAG)
    assert mc.net(0) == 0 and mc.net(0x2000) == 0x2000 and mc.net(0x2000, cmd=True) == 0x12000
    assert mc.net(65535, True) == 0x1FFFF
    for word in GOOD_NET:
        assert mc.check_net(word) == word
        assert sub("engine").Engine._check_net(word) == word
    assert sub("engine").Engine._check_net(None) == 0
    assert mc.parse_net("8192") == 0x2000 and mc.parse_net("0x2000") == 0x2000 and mc.parse_net(8192) == 0x2000
    assert mc.parse_net("0x2000:cmd") == 0x12000 and mc.parse_net("1:cmd") == 0x10001 and mc.parse_net("0") == 0
    for bad, field in list(BAD_NET.items()) + [(-1, "reserved"), (1 << 32, "reserved")]:
        with pytest.raises(mc.QbaError, match=field):
            mc.check_net(bad)
        with pytest.raises(mc.QbaError):
            mc.run_host(3, 4, 1, 1, 0, OracleEngine(), net=bad)
        with pytest.raises(mc.QbaError):
            mc.curve_host(3, [4], 1, 1, 0, OracleEngine(), net=bad)
        with pytest.raises(mc.QbaError):
            sub("engine").Engine._check_net(bad)
    with pytest.raises(mc.QbaError):
        mc.check_net("half")
    for kw in ({"drop_q16": -1}, {"drop_q16": 65536}, {"drop_q16": 0, "cmd": True}):
        with pytest.raises(mc.QbaError):
            mc.net(**kw)
    for text in ("0:cmd", "cmd", "0x2000:", "0x2000:all", "65536", "-1", "half", "0x2000:cmd:cmd", ""):
        with pytest.raises(mc.QbaError):
            mc.parse_net(text)


def test_refusals_come_before_the_engine_is_touched():
    """A non-zero word with a coalition, explain, the tables paths or a sweep:
    ValueError that says the path is not built for a lossy network."""
    mc = sub("montecarlo")
    msg = "not built for a lossy network"
    for path in ("tables", "tables_noisy"):
        with pytest.raises(ValueError, match=msg):
            mc.run(3, 8, 1, 4, 0, None, path=path, net=0x2000)
    with pytest.raises(ValueError, match=msg):
        mc.run(3, 8, 1, 4, 0, None, path="fused", net=0x2000, coalition=0x1)
    with pytest.raises(ValueError, match=msg):
        mc.run(3, 8, 1, 4, 0, None, path="fused", net=0x2000, explain=4, failures=4)
    with pytest.raises(ValueError, match=msg):
        mc.curve(3, [8], 1, 4, 0, None, net=0x2000 | CMD, coalition=0x11)
    with pytest.raises(ValueError, match=msg):
        mc.curve(3, [8], 1, 4, 0, None, net=1, explain=4, failures=4)
    with pytest.raises(ValueError, match=msg):
        mc.sweep(3, [8], [(1, 0xF)], 4, 0, None, net=0x2000)
    with pytest.raises(ValueError, match=msg):
        mc.run_host(3, 8, 1, 1, 0, OracleEngine(), net=0x2000, coalition=0x1)
    for f in (mc.run, mc.curve):  # a bad word is refused as a bad word, also before the engine
        with pytest.raises(mc.QbaError):
            f(3, 8 if f is mc.run else [8], 1, 4, 0, None, net=CMD)
    with pytest.raises(mc.QbaError):
        mc.run(3, 8, 1, 4, 0, None, path="fused", net=1 << 17)


def _calls(lib):
    counts = (C.c_uint32 * 2)(5, 60)
    return {
        "sampled": lambda flip, a, w, cs=counts: lib.qba_montecarlo_curve_sampled_net(None, 7, 2, 0, 4, cs, 2, flip,
                                                                                      None, None, a, w),
        "lists": lambda flip, a, w, cs=counts: lib.qba_montecarlo_curve_lists_net(None, 7, 2, 0, 4, cs, 2, None, 64,
                                                                                  8 * 64, None, None, a, w),
    }


def test_symbols_are_exported_and_the_word_is_checked_after_adv_and_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    u32, p, u64, i64 = C.c_uint32, C.c_void_p, C.c_uint64, C.c_int64
    head = [p, C.c_int, C.c_int, u64, i64, C.POINTER(u32), C.c_int]
    want = {"qba_montecarlo_curve_sampled_net": head + [u32, p, p, u32, u32],
            "qba_montecarlo_curve_lists_net": head + [p, u64, u64, p, p, u32, u32]}
    for name, sig in want.items():
        assert hasattr(lib, name) and lib_mod.SIGNATURES[name] == sig
        assert lib_mod.SIGNATURES[name][:-1] == lib_mod.SIGNATURES[name[:-4] + "_adv"]  # the _adv call's, then net
        assert list(getattr(lib, name).argtypes) == sig
    header = (Path(__file__).resolve().parent.parent / "include" / "qba.h").read_text()
    assert all(f"QBA_API int {name}(" in header for name in want)
    err = lambda: lib.qba_last_error().decode()
    for name, f in _calls(lib).items():
        for bad, field in BAD_NET.items():
            assert f(0, 0xF, bad) == lib_mod.QBA_EINVAL, (name, hex(bad))
            assert ": net" in err() and field in err(), (name, hex(bad), err())
        for ok in GOOD_NET:  # only the device is missing: a NULL ctx is reported after a good word
            assert f(0, 0xF, ok) == lib_mod.QBA_EINVAL and "ctx is NULL" in err(), (name, hex(ok), err())
        for bad_adv in BAD_WORDS:  # adv is looked at first
            assert f(0, bad_adv, CMD) == lib_mod.QBA_EINVAL and ": adv" in err(), (name, err())
    # the rejection order of the other arguments is that of the _adv curve calls
    sampled = _calls(lib)["sampled"]
    assert sampled(65536, 0, CMD) == lib_mod.QBA_EINVAL and "flip_q16" in err()
    down = (C.c_uint32 * 2)(60, 5)
    for f in _calls(lib).values():
        assert f(65536, 0, CMD, down) == lib_mod.QBA_EINVAL and "counts" in err()
    assert lib.qba_montecarlo_curve_sampled_net(None, 16, 2, 0, 4, down, 2, 65536, None, None, 0, CMD) == \
        lib_mod.QBA_EINVAL and "n_parties" in err()
    assert lib.qba_montecarlo_curve_lists_net(None, 7, 8, 0, 4, down, 2, None, 64, 512, None, None, 0, CMD) == \
        lib_mod.QBA_EINVAL and "n_dishonest" in err()


def test_cli_takes_drop_and_refuses_it_where_it_is_not_built():
    tfg = sub("tfg")
    a = tfg._args(["8", "2", "--parties", "7", "--runs", "16", "--drop", "0x2000:cmd", "--curve", "3,8", "--flip", "9",
                   "--adversary", "strip", "--tally", "--failures", "2"])
    assert a.drop == 0x12000 and a.fused and a.adversary == PRESETS["strip"] and a.curve == [3, 8]
    assert tfg._args(["8", "2", "--runs", "16", "--drop", "8192"]).drop == 0x2000
    assert tfg._args(["8", "2", "--runs", "16"]).drop is None
    for bad in (["--drop", "1"], ["--runs", "4", "--drop", "0:cmd"], ["--runs", "4", "--drop", "half"],
                ["--runs", "4", "--drop", "65536"], ["--runs", "4", "--drop", "1:all"],
                ["--runs", "4", "--drop", "1", "--collude", "late"],
                ["--runs", "4", "--drop", "1", "--sweep", "1,2"],
                ["--runs", "4", "--drop", "1", "--explain", "2"],
                ["--runs", "4", "--drop", "1", "--tables"]):
        with pytest.raises(SystemExit):
            tfg._args(["8", "1"] + bad)


# (key, epoch, src, dest, seq): seq 3 -> 4 crosses the block boundary; two keys wrap 2^64 when taken as seed + i
PACKETS = [(0, 0, 1, 2, 0), (0x5EED, 0, 2, 3, 0), (0x5EED, 1, 2, 3, 3), (0x5EED, 1, 2, 3, 4), (0x5EED, 1, 3, 2, 4),
           (0x5EED, 9, 15, 14, 15), ((1 << 64) - 1, 2, 7, 5, 1), ((1 << 64) + 5, 2, 7, 5, 1), (5, 2, 7, 5, 1)]


def test_net_lost_is_the_documented_philox_word():
    mc = sub("montecarlo")
    seen = set()
    for key, e, src, dest, seq in PACKETS:
        words = mc.philox4x32((e, src | dest << 8, seq >> 2, 0x4E455457), key & ((1 << 64) - 1))
        x = words[seq & 3] & 0xFFFF
        seen.add(x)
        for drop in (0, 1, x, x + 1, 0x8000, 0xFFFF):
            assert mc.net_lost(key, e, src, dest, seq, drop) == (x < drop), (key, e, src, dest, seq, drop)
        assert not mc.net_lost(key, e, src, dest, seq, 0)
    assert mc.net_lost((1 << 64) + 5, 2, 7, 5, 1, 0x8000) == mc.net_lost(5, 2, 7, 5, 1, 0x8000)  # the key wraps
    assert len(seen) >= len(PACKETS) - 2  # src and dest, the epoch and the block all enter the counter
    # the same block serves seq 0..3, the next one seq 4
    b0 = mc.philox4x32((1, 2 | 3 << 8, 0, mc.NET_TAG), 0x5EED)
    b1 = mc.philox4x32((1, 2 | 3 << 8, 1, mc.NET_TAG), 0x5EED)
    for seq in range(8):
        assert mc.net_lost(0x5EED, 1, 2, 3, seq, 0x4000) == (((b0 + b1)[seq] & 0xFFFF) < 0x4000)


def test_net_lost_loses_a_quarter_at_0x4000_and_nothing_at_0():
    """2^16 packets: the lost fraction within 5 binomial standard deviations of 1 / 4."""
    mc = sub("montecarlo")
    N, p, lost, lost0 = 1 << 16, 0.25, 0, 0
    for i in range(N):
        args = (0xC0FFEE + (i >> 12), (i >> 8) & 3, 2 + (i & 7), 2 + ((i >> 3) & 7), (i >> 6) & 3 | (i >> 10 & 1) << 2)
        lost += mc.net_lost(*args, 0x4000)
        lost0 += mc.net_lost(*args, 0)
    sd = math.sqrt(p * (1 - p) / N)
    print(f"lost {lost} of {N}: {lost / N:.5f}, 1/4 +- 5 sd = [{p - 5 * sd:.5f}, {p + 5 * sd:.5f}]")
    assert lost0 == 0
    assert abs(lost / N - p) <= 5 * sd


@pytest.mark.parametrize("n", [3, 7])
def test_the_perfect_network_gives_run_hosts_rows(n):
    """net = 0 and net=None against run_host without the argument, word for
    word: 0, 1 and n // 3 traitors, under reference and strip."""
    mc = sub("montecarlo")
    for nd in sorted({0, 1, n // 3}):
        for adv in (PRESETS["reference"], PRESETS["strip"]):
            want = mc.run_host(n, 8, nd, 12, 0xAD0, OracleEngine(), adversary=adv)
            assert np.array_equal(mc.run_host(n, 8, nd, 12, 0xAD0, OracleEngine(), adversary=adv, net=0), want)
            assert np.array_equal(mc.run_host(n, 8, nd, 12, 0xAD0, OracleEngine(), adversary=adv, net=None), want)
            cls = mc.net_party(adv, 0)  # the class itself at net = 0 is AdversaryParty
            assert np.array_equal(mc.run_host(n, 8, nd, 12, 0xAD0, OracleEngine(), party_cls=cls), want)
        plain = mc.run_host(n, 8, nd, 12, 0xAD0, OracleEngine())
        assert np.array_equal(mc.run_host(n, 8, nd, 12, 0xAD0, OracleEngine(), net=0), plain)
        assert np.array_equal(mc.curve_host(n, [3, 8], nd, 12, 0xAD0, OracleEngine(), net=0)[1], plain)


@pytest.fixture(scope="module")
def reached():
    """name -> (rows, the events of reach_events, what observing() recorded)"""
    memo = {}

    def get(name):
        if name not in memo:
            mc = sub("montecarlo")
            n, base = REACH[name][0], REACH[name][3]
            seen = {}
            rows = reach_rows(mc, name, party_cls=observing(mc, seen))
            assert np.array_equal(rows, reach_rows(mc, name))  # observing changes nothing
            plain = reach_rows(mc, name, net=False)
            assert not rows[:, 3].any()
            memo[name] = (rows, reach_events(n, base, rows, plain, seen), seen)
        return memo[name]
    return get


@pytest.mark.parametrize("name", list(REACH))
def test_reach_sets_show_the_events_they_were_chosen_for(reached, name):
    """Counted on the host model alone: no comparison of a kernel with the
    model on these sets can pass by never reaching the event."""
    rows, ev, _ = reached(name)
    print(name, ev)
    for event in REACH[name][8]:
        assert ev[event] > 0, (name, event, ev)


def test_every_listed_event_is_reached_by_some_set(reached):
    """Lost and delivered packets of one sender in one epoch; seq >= 4 on a
    link; a run the loss breaks; a loss that changes an honest V_i and not the
    outcome; under cmd an honest lieutenant without the commander's packet that
    a relay fills, and one that ends empty; a traitor's mutated packet lost."""
    total = {e: sum(reached(name)[1][e] for name in REACH) for e in EVENTS}
    print(total)
    for event in EVENTS:
        assert total[event] > 0, event
    for name in REACH:  # cmd_relayed and cmd_empty only where the word has cmd
        if not REACH[name][7] & CMD:
            assert reached(name)[1]["cmd_lost"] == 0, name


@pytest.mark.parametrize("name", list(REACH))
def test_sent_counts_every_packet_handed_over_lost_or_not(reached, name):
    n, _, _, base, inst = REACH[name][:5]
    rows, _, seen = reached(name)
    lost = sum(l for _, l in seen["links"].values())
    assert lost > 0
    for i in range(inst):
        for r in range(1, n + 1):
            assert rows[i, 8 + 5 * r] == seen["handed"].get((base + i, r), 0), (name, i, r)
    assert sum(seen["handed"].values()) == sum(h for h, _ in seen["links"].values()) == int(rows[:, 8::5].sum())


def test_lossy_network_kernels_keep_the_curve_shapes_resident_waves():
    """No scratch, no static LDS; VGPRs within what the resident waves of
    qba_montecarlo_curve_shape leave a wave (512 per SIMD lane, granule 8), at
    most 128."""
    lib = sub("_lib").lib()
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    new = {k: v for k, v in kds.items() if "qba_k_mc_net_" in k}
    assert sum("18qba_k_mc_net_listsE" in k for k in new) == 1
    for n in range(1, 16):
        kernel = f"_Z20qba_k_mc_net_sampledILi{n}E"
        mine = {k: v for k, v in new.items() if k.startswith(kernel)}
        assert len(mine) == (3 if n <= 11 else 2), n
        waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
        assert lib.qba_montecarlo_curve_shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
        samp = 2 if n <= 11 else 1
        assert any(k.startswith(f"{kernel}Li{samp}ELi{waves.value}E") for k in mine), (n, waves.value)
        per_simd = -(-waves.value * wgs.value // 4)
        budget = 512 // per_simd // 8 * 8
        for k, v in mine.items():
            assert v["vgprs"] <= budget, (k, v, budget)
        # the compiled wave counts are those of the _adv curve kernels
        adv = {k[len("_Z26qba_k_mc_curve_sampled_adv"):].split("EEvPK")[0] for k in kds
               if k.startswith(f"_Z26qba_k_mc_curve_sampled_advILi{n}E")}
        assert {k[len("_Z20qba_k_mc_net_sampled"):].split("EEvPK")[0] for k in mine} == adv, n
    assert len(new) == 1 + 11 * 3 + 4 * 2  # only curve forms; one instantiation serves flip = 0 and flip > 0
    for k, v in new.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= 128, (k, v)
        assert not any(s in k for s in ("qba_k_protocol", "qba_k_mc_curve_", "qba_k_mc_lists", "qba_k_mc_sweep", "_adv",
                                        "coal", "trace"))
