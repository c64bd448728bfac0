"""The (traitors, policy, loss) grid without a GPU:
the two exports and their argument checks through a NULL ctx, the host model
montecarlo.grid_host against the stack of run_host calls and against
sweep_host on the perfect network, the nesting of the loss decisions along
drop_q16, the refusals of montecarlo.grid and of `tfg --grid`, and the static
resources of the grid kernels read from the cross-compiled library."""
import ctypes as C
import random
from pathlib import Path

import numpy as np
import pytest

from conftest import sub
from kd_util import kernel_descriptors
from oracle_engine import OracleEngine
from test_montecarlo_adversary import BAD_WORDS, PRESETS

CMD = 1 << 16
REFERENCE, LOW, STRIP, FIVE = 0xF, PRESETS["reorder_low"], PRESETS["strip"], 0x1F
BAD_NETS = {1 << 17: "reserved", CMD: "cmd"}  # a reserved bit, and cmd with drop_q16 == 0
BAD_ADV = BAD_WORDS[0]


def _scen(lib_mod, triples):
    return (lib_mod.GridScenario * max(len(triples), 1))(*(lib_mod.GridScenario(*t) for t in triples))


def _calls(lib_mod):
    """name -> f(triples, counts=[5, 60], n=7, flip=0, n_scen=None, scen_null=False) through a NULL ctx"""
    lib = lib_mod.lib()

    def make(name):
        def f(triples, counts=(5, 60), n=7, flip=0, n_scen=None, scen_null=False):
            cs = (C.c_uint32 * len(counts))(*counts)
            sc = None if scen_null else _scen(lib_mod, triples)
            ns = len(triples) if n_scen is None else n_scen
            if name == "sampled":
                return lib.qba_montecarlo_grid_sampled(None, n, 0, 4, cs, len(counts), sc, ns, flip, None, None)
            return lib.qba_montecarlo_grid_lists(None, n, 0, 4, cs, len(counts), sc, ns, None, 64, 8 * 64, None, None)
        return f
    return {"sampled": make("sampled"), "lists": make("lists")}


def test_both_exports_are_bound_and_declared_at_the_end_of_the_header():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    u32, p, u64, i64 = C.c_uint32, C.c_void_p, C.c_uint64, C.c_int64
    head = [p, C.c_int, u64, i64, C.POINTER(u32), C.c_int, C.POINTER(lib_mod.GridScenario), C.c_int]
    want = {"qba_montecarlo_grid_sampled": head + [u32, p, p],
            "qba_montecarlo_grid_lists": head + [p, u64, u64, p, p]}
    header = (Path(__file__).resolve().parent.parent / "include" / "qba.h").read_text()
    for name, sig in want.items():
        assert hasattr(lib, name) and lib_mod.SIGNATURES[name] == sig
        assert list(getattr(lib, name).argtypes) == sig
        assert f"QBA_API int {name}(" in header
        # appended: every declaration that was there before stands above them
        assert header.index(f"QBA_API int {name}(") > header.index("QBA_API int qba_montecarlo_curve_lists_net(")
    assert "#define QBA_MC_GRID_MAX 16" in header and "} qba_mc_grid_scenario;" in header
    assert C.sizeof(lib_mod.GridScenario) == 12
    assert [f[0] for f in lib_mod.GridScenario._fields_] == ["n_dishonest", "adv", "net"]
    assert sub("engine").Engine.GRID_MAX == 16


def test_every_check_and_its_order_through_both_entry_points():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    err = lambda: lib.qba_last_error().decode()  # noqa: E731
    good = [(2, REFERENCE, 0), (1, LOW, 0x2000), (7, FIVE, 0xFFFF | CMD)]
    for name, f in _calls(lib_mod).items():
        who = f"qba_montecarlo_grid_{name}: "
        einval = lambda rc: rc == lib_mod.QBA_EINVAL  # noqa: E731
        # only the device is missing: everything before ctx is in order
        assert einval(f(good)) and err() == who + "ctx is NULL", err()
        assert einval(f([good[0]] * 16, counts=(3, 9))) and "ctx is NULL" in err()  # equal scenarios are legal
        assert einval(f([good[1]], counts=tuple(range(32)))) and "ctx is NULL" in err()
        # the scenario list: pointer, n_scen 0 and 17, the product 33
        assert einval(f(good, scen_null=True)) and "scen is NULL" in err()
        assert einval(f([], n_scen=0)) and "n_scen must be in [1, 16]" in err()
        assert einval(f([good[0]] * 17, counts=(5,))) and "n_scen must be in [1, 16]" in err()
        assert einval(f([good[0]] * 3, counts=tuple(range(11)))) and "n_counts * n_scen must be <= 32" in err()
        assert einval(f([good[0]], counts=tuple(range(33)))) and "n_counts must be in [1, 32]" in err()
        # a bad adv and a bad net in scenario 0 and in the last scenario
        for at, scen in ((0, lambda bad: [bad] + good), (3, lambda bad: good + [bad])):
            for net, field in BAD_NETS.items():
                assert einval(f(scen((1, REFERENCE, net)))), (name, at, hex(net))
                assert err().startswith(who + f"scenario {at}: net") and field in err(), err()
            assert einval(f(scen((1, BAD_ADV, 0)))) and err().startswith(who + f"scenario {at}: adv"), err()
            # adv is reported before net within a scenario, n_dishonest before both
            assert einval(f(scen((1, BAD_ADV, CMD)))) and err().startswith(who + f"scenario {at}: adv"), err()
            for k in (-1, 8):
                assert einval(f(scen((k, BAD_ADV, CMD)))), (name, at, k)
                assert err() == who + f"scenario {at}: n_dishonest must be in [0, n_parties]", err()
        # the first bad scenario is the one named
        assert einval(f([good[0], (1, REFERENCE, CMD), (1, BAD_ADV, 0)])) and "scenario 1: net" in err()
        # n + 1 traitors depends on n: 8 is fine at n = 15
        assert einval(f([(8, REFERENCE, 0)], n=15)) and "ctx is NULL" in err()
        # a bad count before a bad scenario, n_parties before a bad count
        assert einval(f([(9, BAD_ADV, CMD)], counts=(60, 5))) and "counts must be strictly increasing" in err()
        assert einval(f([(9, BAD_ADV, CMD)], counts=(60, 5), n=16)) and "n_parties" in err()
        assert einval(f([(9, BAD_ADV, CMD)], counts=(60, 5), n=0)) and "n_parties" in err()
    sampled = _calls(lib_mod)["sampled"]
    # flip_q16 before the scenarios and after the counts
    assert sampled([(9, BAD_ADV, CMD)], flip=65536) == lib_mod.QBA_EINVAL and "flip_q16" in err()
    assert sampled(good, flip=65536, scen_null=True) == lib_mod.QBA_EINVAL and "flip_q16" in err()
    assert sampled(good, flip=65536, counts=(60, 5)) == lib_mod.QBA_EINVAL and "counts" in err()
    assert sampled(good, flip=65535) == lib_mod.QBA_EINVAL and "ctx is NULL" in err()


def test_engine_and_montecarlo_check_the_triples_and_name_the_scenario():
    mc, Engine = sub("montecarlo"), sub("engine").Engine
    cs, sc = Engine._check_grid(7, 4, [5, 60], [(2, REFERENCE, 0), (1, LOW, None), (0, FIVE, 0xFFFF | CMD)])
    assert cs == [5, 60] and sc == [(2, REFERENCE, 0), (1, LOW, 0), (0, FIVE, 0xFFFF | CMD)]
    arr = Engine._grid_array(sc)
    assert [(a.n_dishonest, a.adv, a.net) for a in arr] == sc
    for bad, what in (([], "between 1 and 16"), ([(1, LOW, 0)] * 17, "between 1 and 16"),
                      ([(1, LOW, 0), (8, LOW, 0)], "scenario 1: n_dishonest"),
                      ([(1, LOW, 0), (1, LOW, CMD)], "scenario 1: .*cmd"),
                      ([(1, LOW, 1 << 17)], "scenario 0: .*reserved"),
                      ([(1, LOW, 0), (1, LOW, 1), (1, BAD_ADV, 1)], "scenario 2: "),
                      ([(1, None, 0)], "scenario 0: the policy word is None"),
                      ([(1, LOW)], "triples"), (5, "triples")):
        with pytest.raises(mc.QbaError, match=what):
            Engine._check_grid(7, 4, [5, 60], bad)
    with pytest.raises(mc.QbaError, match="must be <= 32"):
        Engine._check_grid(7, 4, list(range(11)), [(1, LOW, 0)] * 3)
    for bad, what in (([(1, LOW, 0), (1, LOW, CMD)], "scenario 1: .*cmd"), ([(1, BAD_ADV, CMD)], "scenario 0: "),
                      ([(0, LOW, 0), (-1, LOW, 0)], "scenario 1: n_dishonest"), ([(1, LOW)], "triples")):
        with pytest.raises(mc.QbaError, match=what):
            mc.grid_host(7, [3], bad, 1, 0, OracleEngine())
        with pytest.raises(mc.QbaError, match=what):
            mc.grid(7, [3], bad, 4, 0, None)
    # duplicates are refused before the engine is touched; the same pair on two networks is no duplicate
    with pytest.raises(ValueError, match="duplicate"):
        mc.grid(7, [3], [(1, LOW, 0x2000), (2, LOW, 0x2000), (1, LOW, 0x2000)], 4, 0, None)
    assert mc._grid_scenarios(7, [(1, LOW, 0), (1, LOW, 1), (1, REFERENCE, 0)])  # same pair, two networks: legal
    assert "explain" not in mc.grid.__code__.co_varnames[:mc.grid.__code__.co_argcount]
    # the existing refusals stay
    with pytest.raises(ValueError, match="not built for a lossy network"):
        mc.sweep(3, [8], [(1, 0xF)], 4, 0, None, net=0x2000)


@pytest.mark.parametrize("n,inst", [(3, 6), (7, 4)])
def test_grid_host_is_the_stack_of_run_host_and_sweep_host_on_the_perfect_network(n, inst):
    mc = sub("montecarlo")
    base, counts = 0xAD0, [3, 8]
    scen = [(1, REFERENCE, 0), (n // 3, LOW, 0x2000), (n - 1, FIVE, 0), (1, LOW, 0x8000 | CMD), (n - 1, FIVE, 0xFFFF)]
    got = mc.grid_host(n, counts, scen, inst, base, OracleEngine())
    assert got.shape == (len(counts), len(scen), inst, mc.out_words(n)) and got.dtype == np.int32
    for j, c in enumerate(counts):
        for s, (k, word, net) in enumerate(scen):
            want = mc.run_host(n, c, k, inst, base, OracleEngine(), adversary=word, net=net)
            assert np.array_equal(got[j, s], want), (c, s)
    perfect = [s for s, t in enumerate(scen) if t[2] == 0]
    sweep = mc.sweep_host(n, counts, [scen[s][:2] for s in perfect], inst, base, OracleEngine())
    assert np.array_equal(got[:, perfect], sweep)
    assert not np.array_equal(got[-1, 1], mc.run_host(n, 8, n // 3, inst, base, OracleEngine(), adversary=LOW))
    assert mc.grid_host(n, counts, [], inst, base, OracleEngine()).shape == (2, 0, inst, mc.out_words(n))


def test_net_lost_is_monotone_in_drop_q16():
    """A packet's loss word does not depend on drop_q16: it is lost at K iff
    it is lost at any smaller K, on a few thousand random packets."""
    mc = sub("montecarlo")
    rnd = random.Random(0x6D1D)
    ladder = [0, 1, 2, 0x100, 0x400, 0x1000, 0x2000, 0x4000, 0x8000, 0xC000, 0xFFFE, 0xFFFF]
    flips = 0
    for _ in range(3000):
        pkt = (rnd.getrandbits(64), rnd.randrange(0, 16), rnd.randrange(1, 16), rnd.randrange(2, 16),
               rnd.randrange(0, 16))
        lost = [mc.net_lost(*pkt, k) for k in ladder]
        assert not lost[0]
        assert lost == sorted(lost), (pkt, lost)  # False ... False True ... True
        word = mc.philox4x32((pkt[1], pkt[2] | pkt[3] << 8, pkt[4] >> 2, mc.NET_TAG), pkt[0])[pkt[4] & 3] & 0xFFFF
        assert lost == [word < k for k in ladder]
        flips += lost[-1] and not lost[1]
    assert flips > 2900  # the ladder is crossed in between on nearly all of them


def test_cli_takes_a_grid_and_refuses_it_where_it_is_not_built():
    tfg = sub("tfg")
    a = tfg._args(["8", "2", "--parties", "7", "--runs", "16", "--curve", "3,8", "--flip", "9", "--tally", "--failures",
                   "2", "--grid", "2@0,2@0x0100,2@0x0400,2@0x1000:cmd,2:reorder_low@0x0400"])
    assert a.grid == [(2, REFERENCE, 0), (2, REFERENCE, 0x100), (2, REFERENCE, 0x400), (2, REFERENCE, 0x11000),
                      (2, LOW, 0x400)]
    assert a.fused and a.curve == [3, 8] and a.flip == 9 and a.tally and a.failures == 2
    # SCENARIO follows --sweep's grammar: K:POLICY, a bare K, a bare POLICY; no @ is the perfect network
    a = tfg._args(["8", "3", "--runs", "16", "--grid", "strip, 4:reorder_low@8192 ,1,relay@1:cmd,0x1F@65535"])
    assert a.grid == [(3, STRIP, 0), (4, LOW, 0x2000), (1, REFERENCE, 0), (3, PRESETS["relay"], 0x10001),
                      (3, FIVE, 0xFFFF)]
    assert [t[:2] for t in a.grid[:3]] == tfg._args(["8", "3", "--runs", "16", "--sweep",
                                                     "strip,4:reorder_low,1"]).sweep
    assert tfg._args(["8", "2", "--runs", "16"]).grid is None
    sixteen = ",".join(f"2@{k}" for k in range(16))
    assert len(tfg._args(["8", "2", "--runs", "4", "--grid", sixteen]).grid) == 16
    assert len(tfg._args(["8", "2", "--runs", "4", "--curve", "3", "--grid", sixteen]).grid) == 16  # 32 lines
    seventeen = sixteen + ",2@16"
    for bad in (["--grid", "2@0"],                                             # needs --runs
                ["--runs", "4", "--grid", ""], ["--runs", "4", "--grid", seventeen],
                ["--runs", "4", "--curve", "3,5", "--grid", sixteen],          # 48 lines
                ["--runs", "4", "--grid", "2@0,2@0x0"],                        # an item twice
                ["--runs", "4", "--grid", "2@0:cmd"], ["--runs", "4", "--grid", "2@65536"],
                ["--runs", "4", "--grid", "2@half"], ["--runs", "4", "--grid", "2@"],
                ["--runs", "4", "--grid", "2@1:all"], ["--runs", "4", "--grid", "2@1@2"],
                ["--runs", "4", "--grid", "nobody@1"], ["--runs", "4", "--grid", "2:0x100000@1"],
                ["--runs", "4", "--grid", "2@1", "--sweep", "1,2"],
                ["--runs", "4", "--grid", "2@1", "--drop", "1"],
                ["--runs", "4", "--grid", "2@1", "--adversary", "strip"],
                ["--runs", "4", "--grid", "2@1", "--collude", "late"],
                ["--runs", "4", "--grid", "2@1", "--explain", "2"],
                ["--runs", "4", "--grid", "2@1", "--tables"]):
        with pytest.raises(SystemExit):
            tfg._args(["8", "1"] + bad)
    # what was refused before still is
    with pytest.raises(SystemExit):
        tfg._args(["8", "1", "--runs", "4", "--drop", "1", "--sweep", "1,2"])


def test_grid_kernels_keep_the_curve_shapes_resident_waves():
    """Names and counts; no scratch, no static LDS; the sampled kernels' VGPRs
    within what the resident waves of qba_montecarlo_curve_shape leave a wave
    (512 per SIMD lane over the waves per SIMD, granule 8) for every n and
    sampler; the compiled wave counts those of the _adv curve kernels."""
    lib = sub("_lib").lib()
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    new = {k: v for k, v in kds.items() if "qba_k_grid_" in k}
    assert sum("16qba_k_grid_listsE" in k for k in new) == 1
    for n in range(1, 16):
        kernel = f"_Z18qba_k_grid_sampledILi{n}E"
        mine = {k: v for k, v in new.items() if k.startswith(kernel)}
        assert len(mine) == (3 if n <= 11 else 2), n
        waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
        assert lib.qba_montecarlo_curve_shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
        samp = 2 if n <= 11 else 1
        assert any(k.startswith(f"{kernel}Li{samp}ELi{waves.value}E") for k in mine), (n, waves.value)
        per_simd = -(-waves.value * wgs.value // 4)
        budget = 512 // per_simd // 8 * 8
        for k, v in mine.items():
            print(f"n={n} {k[len(kernel):].split('EEvPK')[0]} vgprs {v['vgprs']} budget {budget}")
            assert v["vgprs"] <= budget, (k, v, budget)
        adv = {k[len("_Z26qba_k_mc_curve_sampled_adv"):].split("EEvPK")[0] for k in kds
               if k.startswith(f"_Z26qba_k_mc_curve_sampled_advILi{n}E")}
        assert {k[len("_Z18qba_k_grid_sampled"):].split("EEvPK")[0] for k in mine} == adv, n
    assert len(new) == 1 + 11 * 3 + 4 * 2  # one instantiation serves flip = 0 and flip > 0
    for k, v in new.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)
        # outside the patterns the sibling descriptor tests find their kernels by
        assert not any(s in k for s in ("qba_k_mc_", "qba_k_protocol", "qba_k_trace_", "_adv", "coal"))
