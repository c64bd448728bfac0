"""The scenario sweep without a GPU: the exports, the
argument checks of the two C entry points and their order (through a null
ctx), the host model montecarlo.sweep_host against the stack of run_host, the
nesting of the traitor sets of one key, and the static resources and compiled
wave counts of the new kernels read from the cross-compiled library."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from conftest import sub
from kd_util import kernel_descriptors
from oracle_engine import OracleEngine

REFERENCE, RELAY, LOW, STRIP = 0xF, 0x10, 0x11102, 0x100C
SYMBOLS = ("qba_montecarlo_sweep_sampled", "qba_montecarlo_sweep_lists")


def test_symbols_are_exported_and_bound():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES
        assert getattr(lib, name).argtypes == lib_mod.SIGNATURES[name]
    assert C.sizeof(lib_mod.Scenario) == 8
    eng = sub("engine").Engine
    assert eng.SWEEP_MAX == 16 and callable(eng.montecarlo_sweep_sampled) and callable(eng.montecarlo_sweep_lists)


def _scen(pairs):
    S = sub("_lib").Scenario
    return (S * max(len(pairs), 1))(*(S(k, w) for k, w in pairs))


def _calls(lib):
    """name -> f(n, counts, scenarios, n_scen=None, flip=0): the entry point with a null ctx"""
    def sampled(n, counts, pairs, n_scen=None, flip=0):
        cs = (C.c_uint32 * len(counts))(*counts)
        return lib.qba_montecarlo_sweep_sampled(None, n, 0, 4, cs, len(counts), _scen(pairs),
                                                len(pairs) if n_scen is None else n_scen, flip, None, None)

    def lists(n, counts, pairs, n_scen=None, flip=0):
        cs = (C.c_uint32 * len(counts))(*counts)
        return lib.qba_montecarlo_sweep_lists(None, n, 0, 4, cs, len(counts), _scen(pairs),
                                              len(pairs) if n_scen is None else n_scen, None, 64, 8 * 64, None, None)
    return {"sampled": sampled, "lists": lists}


def test_every_argument_check_and_its_order_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    n, ok = 7, [(0, REFERENCE), (2, LOW), (7, STRIP)]

    def refused(rc, *needles):
        msg = lib.qba_last_error().decode()
        assert rc == lib_mod.QBA_EINVAL and all(s in msg for s in needles), (rc, msg, needles)

    for name, f in _calls(lib).items():
        refused(f(n, [5, 60], ok), "ctx is NULL")                          # only the device is missing
        refused(f(n, [5, 60], [(2, LOW)] * 16), "ctx is NULL")             # 16 x 2, equal scenarios are legal
        refused(f(n, list(range(32)), [(2, LOW)]), "ctx is NULL")          # 1 x 32
        refused(f(n, [5, 60], ok, n_scen=0), "n_scen")
        refused(f(n, [5], [(2, LOW)] * 17), "n_scen")
        refused(f(n, [1, 2, 3], [(2, LOW)] * 11), "n_counts * n_scen")     # product 33
        refused(f(n, list(range(11)), [(2, LOW)] * 3), "n_counts * n_scen")
        refused(f(n, [5, 60], [(0, 0x2F)] + ok), "scenario 0", "adv")      # a bad word in scenario 0
        refused(f(n, [5, 60], ok + [(1, 0x300)]), "scenario 3", "adv")     # ... and in the last one
        refused(f(n, [5, 60], ok + [(1, 0)]), "scenario 3", "adv")
        refused(f(n, [5, 60], [(-1, REFERENCE)] + ok), "scenario 0", "n_dishonest")
        refused(f(n, [5, 60], ok + [(n + 1, REFERENCE)]), "scenario 3", "n_dishonest")
        refused(f(n, [5, 60], [(n + 1, 0x2F)]), "scenario 0", "n_dishonest")   # n_dishonest before the word
        refused(f(n, [5, 60], [(1, 0x2F), (-1, 0xF)]), "scenario 0", "adv")     # index order
        # the order: n_parties, counts, (flip_q16,) the scenario list, the scenarios
        refused(f(16, [60, 5], [(-1, 0)] * 17), "n_parties")
        refused(f(n, [60, 5], [(-1, 0)] * 17), "counts")                    # a bad count before a bad scenario
        refused(f(n, [60, 5], [(n + 1, REFERENCE)]), "counts")
        refused(f(n, [], ok), "n_counts")
        refused(f(n, [1 << 31], ok), "counts")
        refused(f(n, [5, 60], [(-1, 0)] * 17), "n_scen")
        refused(f(n, [1, 2, 3], [(-1, 0)] * 11), "n_counts * n_scen")
    sampled = _calls(lib)["sampled"]
    refused(sampled(n, [60, 5], ok, flip=65536), "counts")
    refused(sampled(n, [5, 60], [(-1, 0)] * 17, flip=65536), "flip_q16")    # flip_q16 before the scenarios
    refused(sampled(n, [5, 60], ok, flip=65535), "ctx is NULL")
    cs = (C.c_uint32 * 2)(5, 60)
    assert lib.qba_montecarlo_sweep_sampled(None, n, 0, 4, cs, 2, None, 1, 0, None, None) == lib_mod.QBA_EINVAL
    assert "scen is NULL" in lib.qba_last_error().decode()


def test_engine_validation_mirrors_the_entry_points():
    eng, QbaError = sub("engine").Engine, sub("_lib").QbaError
    cs, sc = eng._check_sweep(7, 4, [5, 60], [(0, REFERENCE), (7, STRIP)])
    assert cs == [5, 60] and sc == [(0, REFERENCE), (7, STRIP)]
    for counts, scen in (([5, 60], []), ([5], [(1, LOW)] * 17), ([1, 2, 3], [(1, LOW)] * 11), ([60, 5], [(1, LOW)]),
                         ([5], [(-1, LOW)]), ([5], [(8, LOW)]), ([5], [(1, 0x2F)]), ([5], [(1, None)]), ([5], [1]),
                         ([], [(1, LOW)])):
        with pytest.raises(QbaError):
            eng._check_sweep(7, 4, counts, scen)


COUNTS = [0, 1, 5, 40]


@pytest.mark.parametrize("n,base", [(3, 0x5EED0), (7, 0xAD0)])
def test_sweep_host_is_the_stack_of_run_host(n, base):
    mc = sub("montecarlo")
    eng, inst = OracleEngine(), 6
    scen = [(0, REFERENCE), (1, REFERENCE), (n // 3, LOW), (n - 1, STRIP), (n, RELAY)]
    got = mc.sweep_host(n, COUNTS, scen, inst, base, eng)
    assert got.shape == (len(COUNTS), len(scen), inst, mc.out_words(n)) and got.dtype == np.int32
    for j, c in enumerate(COUNTS):
        for s, (k, word) in enumerate(scen):
            assert np.array_equal(got[j, s], mc.run_host(n, c, k, inst, base, eng, adversary=word)), (c, k, hex(word))
    assert np.array_equal(got[:, 1], mc.curve_host(n, COUNTS, 1, inst, base, eng))  # 0xF: the rows without a policy
    assert not got[:, :, :, 3].any()
    assert any(not np.array_equal(got[:, 0], got[:, s]) for s in range(1, len(scen)))  # the scenarios matter
    for bad in ([(n + 1, REFERENCE)], [(-1, REFERENCE)], [(1, 0x2F)], [3]):
        with pytest.raises(mc.QbaError):
            mc.sweep_host(n, COUNTS, bad, inst, base, eng)


@pytest.mark.parametrize("n", [1, 3, 7, 11, 15])
def test_traitor_sets_of_one_key_are_nested(n):
    """The pairing of a sweep over n_dishonest: under one key the traitors at k
    are the first k of the traitors at k + 1 (ProtocolRng.choice is a partial
    Fisher-Yates), read from the draw and, where the host model runs, from the
    rows' dishonest masks; the commander's order does not depend on k."""
    mc = sub("montecarlo")
    for key in (0, 0xAD0, (1 << 64) - 1):
        draws = [[int(r) for r in mc.ProtocolRng(key, 0).choice(np.arange(1, n + 1), k)] for k in range(n + 1)]
        for k in range(n):
            assert draws[k + 1][:k] == draws[k] and len(set(draws[k + 1])) == k + 1, (key, k)
    if n > 7:
        return
    inst, base = 5, 0xAD0
    rows = mc.sweep_host(n, [6], [(k, REFERENCE) for k in range(n + 1)], inst, base, OracleEngine())[0]
    assert not rows[:, :, 3].any()
    masks = rows[:, :, 1]
    for k in range(n + 1):
        for i in range(inst):
            want = sum(1 << int(r) for r in mc.ProtocolRng(base + i, 0).choice(np.arange(1, n + 1), k))
            assert int(masks[k, i]) == want
            assert k == 0 or int(masks[k - 1, i]) & ~int(masks[k, i]) == 0
    honest_cmd = (masks[-2] >> 1) & 1 == 0   # the commander stays honest up to k = n - 1: one order in all of them
    for i in np.nonzero(honest_cmd)[0]:
        assert len({int(rows[k, i, 4 + 5 * 1]) for k in range(n)}) == 1


def test_sweep_refuses_duplicates_before_it_touches_the_engine():
    mc = sub("montecarlo")
    with pytest.raises(ValueError, match="duplicate"):
        mc.sweep(7, [5, 60], [(2, LOW), (1, LOW), (2, LOW)], 10, 0, None)
    with pytest.raises(ValueError, match="duplicate"):
        mc.sweep(7, [5], [(2, "15"), (2, 0xF)], 10, 0, None)
    with pytest.raises(mc.QbaError):
        mc.sweep(7, [5], [(8, LOW)], 10, 0, None)


def test_cli_parses_and_rejects_sweep_arguments():
    tfg, mc = sub("tfg"), sub("montecarlo")
    a = tfg._args(["8", "2", "--parties", "7", "--runs", "10", "--sweep", "1:strip,relay,3,0:0x10"])
    assert a.sweep == [(1, STRIP), (2, RELAY), (3, REFERENCE), (0, RELAY)]
    assert mc.ADVERSARIES["strip"] == STRIP and mc.ADVERSARIES["reorder_low"] == LOW
    for bad in (["--sweep", "1:strip"], ["--runs", "10", "--sweep", "1:nobody"], ["--runs", "10", "--sweep", ""],
                ["--runs", "10", "--sweep", "1:strip,1:strip"], ["--runs", "10", "--sweep", "1,reference", "--parties", "7"],
                ["--runs", "10", "--sweep", "1:strip", "--adversary", "strip"],
                ["--runs", "10", "--sweep", "1:strip", "--tables"],
                ["--runs", "10", "--sweep", ",".join(f"{k}:strip" for k in range(17)), "--parties", "15"],
                ["--runs", "10", "--sweep", "0,1,2", "--curve", ",".join(str(c) for c in range(20, 30))]):
        with pytest.raises(SystemExit):
            tfg._args(["8", "1"] + bad)


@pytest.fixture(scope="module")
def kds():
    return kernel_descriptors(Path(sub("_lib").LIB_PATH))


def test_sweep_kernels_use_no_scratch_no_static_lds_and_at_most_128_vgprs(kds):
    new = {k: v for k, v in kds.items() if "qba_k_mc_sweep_" in k}
    assert sum("20qba_k_mc_sweep_listsE" in k for k in new) == 1
    for n in range(1, 16):   # every sampler of the n: the closed form's up to 11
        assert sum(k.startswith(f"_Z22qba_k_mc_sweep_sampledILi{n}E") for k in new) == (3 if n <= 11 else 2), n
    for n in range(1, 12):
        assert sum(k.startswith(f"_Z22qba_k_mc_sweep_sampledILi{n}ELi2E") for k in new) == 1, n
    assert len(new) == 1 + 11 * 3 + 4 * 2   # one instantiation serves flip = 0 and flip > 0
    for k, v in new.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= 128, (k, v)
    # the kernels that were there stay findable by the names the sibling tests use
    for name in new:
        assert not any(s in name for s in ("qba_k_protocol", "qba_k_mc_curve_", "qba_k_mc_lists"))
    assert sum("qba_k_protocol" in k for k in kds) == 1
    assert sum("qba_k_mc_curve_lists" in k for k in kds) == 1
    for k, v in kds.items():
        if "qba_k_mc_" in k:
            assert v["scratch"] == 0 and v["vgprs"] <= 128, (k, v)


def test_curve_shape_is_the_sweep_kernels_shape(kds):
    """qba_montecarlo_curve_shape stays the shape query: the wave count the
    shipped sampler's sweep kernel is compiled for is the one it reports, and
    the curve _adv kernel's."""
    lib = sub("_lib").lib()
    for n in range(1, 16):
        waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
        assert lib.qba_montecarlo_curve_shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
        samp = 2 if n <= 11 else 1
        tail = f"ILi{n}ELi{samp}ELi{waves.value}E"
        assert any(k.startswith("_Z22qba_k_mc_sweep_sampled" + tail) for k in kds), n
        assert any(k.startswith("_Z26qba_k_mc_curve_sampled_adv" + tail) for k in kds), n
