"""Noise profiles without a GPU: the definition
montecarlo.noise_masks_profile against montecarlo.noise_masks and against a
scalar restatement, the per-row rates and the depolarised entries, the builder,
the parser and every refusal, the three C entry points' checks with a NULL ctx,
the static resources of the new kernels read from the cross-compiled library,
and the events the host model reaches on the recorded reach sets
(tests/montecarlo_noise_profile_cases.py)."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from conftest import sub
from kd_util import kernel_descriptors
from montecarlo_noise_profile_cases import (CASES, EVENTS, GRID, MEAN, PROFILES, REACH, REACH_BASE, REACH_KEYS,
                                            commander_only, depol_hits, observing, policy_at, q_events, rates_of,
                                            scalar_masks)
from test_montecarlo_adversary import BAD_WORDS, HostEngine

KEY = 0x4E50AB


@pytest.mark.parametrize("n", [1, 3, 7, 11, 15])
def test_uniform_profile_is_the_flip_model_and_a_zero_row_stays_zero(n):
    mc = sub("montecarlo")
    for k in (1, 0x1000, 0x8000, 0xFFFF):
        want = mc.noise_masks(n, KEY, 130, k)
        got = mc.noise_masks_profile(n, KEY, 130, [k] * (n + 1), 0)
        assert got.dtype == np.uint8 and got.shape == (n + 1, 130) and np.array_equal(got, want), (n, k)
        for zero in range(n + 1):  # a row with rate 0 is all zero whatever the others hold; the others keep theirs
            rates = [k] * (n + 1)
            rates[zero] = 0
            got = mc.noise_masks_profile(n, KEY, 130, rates, 0)
            assert not got[zero].any()
            assert np.array_equal(np.delete(got, zero, 0), np.delete(want, zero, 0))
    assert not mc.noise_masks_profile(n, KEY, 130, [0] * (n + 1), 0).any()
    lists = np.arange((n + 1) * 130, dtype=np.uint8).reshape(n + 1, 130) & 1
    assert np.array_equal(mc.noisy_lists_profile(n, KEY, lists, [0x1000] * (n + 1), 0),
                          mc.noisy_lists(n, KEY, lists, 0x1000))


@pytest.mark.parametrize("n", [3, 7, 15])
def test_mixed_profile_equals_the_scalar_restatement(n):
    mc = sub("montecarlo")
    for key in (KEY, (1 << 64) - 1):
        for depol in (0, 0x4000):
            rates = rates_of("mixed", n)
            assert rates[:4] == [0x8000, 0, 0x1000, 2]
            got = mc.noise_masks_profile(n, key, 40, rates, depol)
            assert np.array_equal(got, scalar_masks(mc, n, key, 40, rates, depol)), (n, depol)
            assert np.array_equal(mc.noise_masks_profile(n, key + (1 << 64), 40, rates, depol), got)  # the key wraps


def test_every_row_flips_at_its_own_rate():
    """2^16 entries at n = 7 (nQ = 3 bits a value): the count of set mask bits
    of row g is Binomial(N * nQ, rate[g] / 65536); 5 standard deviations leave
    a false alarm below 6e-7 per row (the normal tail, N * nQ * p * (1 - p) >=
    5952 here)."""
    mc = sub("montecarlo")
    n, N, nq = 7, 1 << 16, 3
    rates = [0x4000, 0, 0x0800, 0x4000, 0x0800, 0x8000, 1, 0xFFFF]
    masks = mc.noise_masks_profile(n, KEY, N, rates, 0)
    for g, k in enumerate(rates):
        ones, p = int(np.unpackbits(masks[g]).sum()), k / 65536
        mean, sd = N * nq * p, math.sqrt(N * nq * p * (1 - p))
        print(f"row {g} rate {k:#x}: {ones} set bits, {mean:.1f} +- 5 * {sd:.2f}")
        assert abs(ones - mean) <= 5 * sd, (g, ones, mean, sd)
    assert not masks[1].any()


def test_depolarised_entries():
    mc = sub("montecarlo")
    n, N = 7, 1 << 16
    w = 8
    zero = [0] * (n + 1)
    full = mc.noise_masks_profile(n, KEY, N, zero, 0xFFFF)
    hit = depol_hits(mc, KEY, N, 0xFFFF)
    print(f"depol 0xFFFF: {int((~hit).sum())} entries of {N} not depolarised")
    assert 0 <= int((~hit).sum()) <= 16  # about 2^-16 of them: one expected, 16 is beyond any Poisson(1) tail
    assert not full[:, ~hit].any()
    for g in range(n + 1):  # uniform below w in every row: all w values, each within 5 sd of N / w
        cnt = np.bincount(full[g, hit], minlength=w)
        assert len(cnt) == w and np.all(np.abs(cnt - hit.sum() / w) <= 5 * math.sqrt(N / w * (1 - 1 / w))), (g, cnt)
    one = mc.noise_masks_profile(n, KEY, N, zero, 1)
    hit1 = depol_hits(mc, KEY, N, 1)
    print(f"depol 1: entries {np.nonzero(hit1)[0].tolist()}")
    assert not one[:, ~hit1].any()
    assert np.array_equal(one[:, hit1], full[:, hit1])  # the value does not depend on depol_q16
    for e in np.nonzero(hit1)[0]:
        assert np.array_equal(one[:, e], scalar_masks(mc, n, KEY, int(e) + 1, zero, 1)[:, e])
    nested = depol_hits(mc, KEY, 4096, 0x4000)
    assert np.all(nested >= depol_hits(mc, KEY, 4096, 0x1000))  # hit at K is hit at every K' >= K


def test_builder_parser_and_checks_name_the_field():
    mc, E = sub("montecarlo"), sub("montecarlo").QbaError
    assert mc.noise_profile(3) == ((0, 0, 0, 0), 0)
    assert mc.noise_profile(3, 5, {0: 7, 3: 0}, 9) == ((7, 5, 5, 0), 9)
    assert mc.check_noise_profile(2, [1, 2, np.uint16(3)], 4) == ((1, 2, 3), 4)
    assert mc.parse_noise_profile(3, "all:0x10,3:5,depol:1024") == ((16, 16, 16, 5), 1024)
    assert mc.parse_noise_profile(3, "0:0x8000") == ((0x8000, 0, 0, 0), 0)
    assert mc.parse_noise_profile(3, "2:7, all:1") == ((1, 1, 7, 1), 0)  # a row overrides all wherever it stands
    assert mc.parse_noise_profile(3, "") == ((0, 0, 0, 0), 0)
    assert mc.parse_noise_profile(3, ((1, 2, 3, 4), 5)) == ((1, 2, 3, 4), 5)
    p = mc.parse_noise_profile(7, "all:16,3:5,depol:0x400")
    assert mc.format_noise_profile(p) == "all:0x10,3:0x5,depol:0x400"
    assert mc.parse_noise_profile(7, mc.format_noise_profile(p)) == p
    for rates, depol, field in (([0] * 3, 0, "3 rows"), ([0] * 5, 0, "5 rows"), ([0, 0, 65536, 0], 0, "row 2"),
                                ([-1, 0, 0, 0], 0, "row 0"), ([0, 0.5, 0, 0], 0, "row 1"), ([0, 0, 0, True], 0, "row 3"),
                                ([0, 0, 0, "1"], 0, "row 3"), ([0] * 4, 65536, "depol_q16"), ([0] * 4, -1, "depol_q16"),
                                ([0] * 4, 1.0, "depol_q16"), (7, 0, "sequence")):
        with pytest.raises(E, match=field):
            mc.check_noise_profile(3, rates, depol)
        with pytest.raises(E, match=field):
            mc.run_host(3, 4, 1, 1, 0, HostEngine(), noise=(rates, depol))
        with pytest.raises(E, match=field):
            sub("engine").Engine._check_noise(3, (rates, depol))
    for kw, field in (({"rows": {4: 1}}, "row 4"), ({"rows": {-1: 1}}, "row -1"), ({"all": 65536}, "row 0"),
                      ({"rows": {2: 70000}}, "row 2"), ({"depol_q16": 65536}, "depol_q16")):
        with pytest.raises(E, match=field):
            mc.noise_profile(3, **kw)
    for text, field in (("al:1", "'al'"), ("4:1", "row 4"), ("1:1,1:2", "row 1 given twice"), ("all:1,all:2", "all"),
                        ("depol:1,depol:1", "depol given twice"), ("1", "KEY:K"), ("1:x", "1: K"),
                        ("depol:65536", "depol_q16"), ("2:65536", "row 2"), ("-1:1", "-1")):
        with pytest.raises(E, match=field):
            mc.parse_noise_profile(3, text)
    rates, n_rates, depol = sub("engine").Engine._check_noise(3, None)
    assert list(rates) == [0] * 4 and n_rates == 4 and depol == 0


def test_refusals_come_before_the_engine_is_touched():
    mc = sub("montecarlo")
    prof = mc.noise_profile(3, 0x1000)
    msg = "noise profile"
    for path in ("tables", "tables_noisy"):
        with pytest.raises(ValueError, match="path=.*" + msg):
            mc.run(3, 8, 1, 4, 0, None, path=path, noise=prof)
    for f, size in ((lambda **kw: mc.run(3, 8, 1, 4, 0, None, path="fused", **kw), 8),
                    (lambda **kw: mc.curve(3, [8], 1, 4, 0, None, **kw), 8)):
        with pytest.raises(ValueError, match="flip_q16=9.*" + msg):
            f(noise=prof, flip_q16=9)
        with pytest.raises(ValueError, match="coalition.*" + msg):
            f(noise=prof, coalition=0x1)
        with pytest.raises(ValueError, match="lossy network.*" + msg):
            f(noise=prof, net=0x2000)
        with pytest.raises(ValueError, match="explain.*" + msg):
            f(noise=prof, explain=4, failures=4)
        with pytest.raises(mc.QbaError, match="row 1"):
            f(noise=([0, -1, 0, 0], 0))
    with pytest.raises(ValueError, match="a sweep.*" + msg):
        mc.sweep(3, [8], [(1, 0xF)], 4, 0, None, noise=prof)
    with pytest.raises(ValueError, match="a grid.*" + msg):
        mc.grid(3, [8], [(1, 0xF, 0)], 4, 0, None, noise=prof)
    with pytest.raises(ValueError, match="replay.*" + msg):
        mc.replay(3, 8, 1, [0], 0, None, noise=prof)
    for kw, what in (({"flip_q16": 9}, "flip_q16=9"), ({"coalition": 1}, "coalition"), ({"net": 0x2000}, "lossy")):
        with pytest.raises(ValueError, match=what + ".*" + msg):
            mc.run_host(3, 8, 1, 1, 0, HostEngine(), noise=prof, **kw)
        with pytest.raises(ValueError, match=what + ".*" + msg):
            mc.curve_host(3, [8], 1, 1, 0, HostEngine(), noise=prof, **kw)
    # zero words beside a profile are no refusal, and noise=None calls what was called
    want = mc.run_host(3, 8, 1, 6, KEY, HostEngine())
    assert np.array_equal(mc.run_host(3, 8, 1, 6, KEY, HostEngine(), noise=None, net=0, coalition=0), want)
    assert np.array_equal(mc.run_host(3, 8, 1, 6, KEY, HostEngine(), noise=mc.noise_profile(3), net=0), want)
    assert np.array_equal(mc.run_host(3, 8, 1, 6, KEY, HostEngine(), noise=prof),
                          mc.run_host(3, 8, 1, 6, KEY, HostEngine(), flip_q16=0x1000))


def test_cli_takes_noise_and_refuses_it_where_it_is_not_built():
    tfg, mc = sub("tfg"), sub("montecarlo")
    a = tfg._args(["8", "2", "--parties", "7", "--runs", "16", "--noise", "all:16,0:0x8000,depol:0x400", "--curve",
                   "3,8", "--adversary", "strip", "--tally", "--failures", "2"])
    assert a.noise == ((0x8000,) + (16,) * 7, 0x400) and a.fused and a.curve == [3, 8]
    assert mc.format_noise_profile(a.noise) == "all:0x10,0:0x8000,depol:0x400"
    assert tfg._args(["8", "2", "--runs", "16"]).noise is None
    base = ["--runs", "4", "--noise", "all:1"]
    for bad in (["--noise", "all:1"], ["--runs", "4", "--noise", "4:1"], ["--runs", "4", "--noise", "al:1"],
                ["--runs", "4", "--noise", "1:1,1:1"], ["--runs", "4", "--noise", "depol:65536"],
                base + ["--flip", "9"], base + ["--collude", "late"], base + ["--drop", "1"], base + ["--sweep", "1,2"],
                base + ["--grid", "1@0"], base + ["--explain", "2"], base + ["--tables"],
                ["--noise", "all:1", "--replay", "3", "--seed", "1"]):
        with pytest.raises(SystemExit):
            tfg._args(["8", "1"] + bad)


def test_cli_refusals_name_the_flag(capsys):
    tfg = sub("tfg")
    for extra, flag in ((["--flip", "9"], "--flip"), (["--collude", "late"], "--collude"), (["--drop", "1"], "--drop"),
                        (["--sweep", "1,2"], "--sweep"), (["--grid", "1@0"], "--grid"), (["--explain", "2"], "--explain"),
                        (["--tables"], "--tables")):
        with pytest.raises(SystemExit):
            tfg._args(["8", "1", "--runs", "4", "--noise", "all:1"] + extra)
        assert f"--noise: not with {flag}" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tfg._args(["8", "1", "--noise", "all:1", "--replay", "3", "--seed", "1"])
    assert "--noise: not with --replay" in capsys.readouterr().err


def _calls(lib):
    counts = (C.c_uint32 * 2)(5, 60)
    return {
        "qba_montecarlo_curve_sampled_nprof":
            lambda a, r, nr, d, cs=counts, n=7, nd=2: lib.qba_montecarlo_curve_sampled_nprof(
                None, n, nd, 0, 4, cs, 2, None, None, a, r, nr, d),
        "qba_montecarlo_curve_lists_nprof":
            lambda a, r, nr, d, cs=counts, n=7, nd=2: lib.qba_montecarlo_curve_lists_nprof(
                None, n, nd, 0, 4, cs, 2, None, 64, 8 * 64, None, None, a, r, nr, d),
    }


def test_symbols_are_exported_and_the_profile_is_checked_after_adv_and_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    u32, p, u64, i64, pu16 = C.c_uint32, C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(C.c_uint16)
    head = [p, C.c_int, C.c_int, u64, i64, C.POINTER(u32), C.c_int]
    want = {"qba_montecarlo_curve_sampled_nprof": head + [p, p, u32, pu16, C.c_int, u32],
            "qba_montecarlo_curve_lists_nprof": head + [p, u64, u64, p, p, u32, pu16, C.c_int, u32],
            "qba_noise_profile_apply": [p, C.c_int, u64, i64, u64, pu16, C.c_int, u32, p, u64, u64, p]}
    for name, sig in want.items():
        assert hasattr(lib, name) and lib_mod.SIGNATURES[name] == sig
        assert list(getattr(lib, name).argtypes) == sig
    adv_sig = lib_mod.SIGNATURES["qba_montecarlo_curve_sampled_adv"]  # the _adv call's without flip_q16, then the profile
    assert want["qba_montecarlo_curve_sampled_nprof"][:-3] == adv_sig[:7] + adv_sig[8:]
    assert want["qba_montecarlo_curve_lists_nprof"][:-3] == lib_mod.SIGNATURES["qba_montecarlo_curve_lists_adv"]
    header = (Path(__file__).resolve().parent.parent / "include" / "qba.h").read_text()
    assert all(f"QBA_API int {name}(" in header for name in want)
    err = lambda: lib.qba_last_error().decode()  # noqa: E731
    rates = (C.c_uint16 * 8)(*([0x1000] * 8))
    for name, f in _calls(lib).items():
        for nr in (0, 7, 9, -1):
            assert f(0xF, rates, nr, 0) == lib_mod.QBA_EINVAL and name + ": n_rates" in err(), (name, nr, err())
        assert f(0xF, None, 8, 0) == lib_mod.QBA_EINVAL and name + ": rates_host is NULL" in err(), (name, err())
        for d in (65536, 1 << 31):
            assert f(0xF, rates, 8, d) == lib_mod.QBA_EINVAL and name + ": depol_q16" in err(), (name, d, err())
        for d in (0, 1, 65535):  # only the device is missing: a NULL ctx is reported after a good profile
            assert f(0xF, rates, 8, d) == lib_mod.QBA_EINVAL and "ctx is NULL" in err(), (name, d, err())
        for bad_adv in BAD_WORDS:  # adv is looked at first
            assert f(bad_adv, None, 0, 65536) == lib_mod.QBA_EINVAL and ": adv" in err(), (name, err())
        # the rejection order of the other arguments is that of the _adv curve calls
        down = (C.c_uint32 * 2)(60, 5)
        assert f(0, None, 0, 65536, down) == lib_mod.QBA_EINVAL and "counts" in err()
        assert f(0, None, 0, 65536, down, 16) == lib_mod.QBA_EINVAL and "n_parties" in err()
        assert f(0, None, 0, 65536, down, 7, 8) == lib_mod.QBA_EINVAL and "n_dishonest" in err()
    name = "qba_noise_profile_apply"
    apply = lambda r, nr, d, n=7: lib.qba_noise_profile_apply(None, n, 0, 4, 60, r, nr, d, None, 64, 512, None)  # noqa: E731
    assert apply(rates, 7, 0) == lib_mod.QBA_EINVAL and name + ": n_rates" in err()
    assert apply(None, 8, 0) == lib_mod.QBA_EINVAL and name + ": rates_host is NULL" in err()
    assert apply(rates, 8, 65536) == lib_mod.QBA_EINVAL and name + ": depol_q16" in err()
    assert apply(rates, 8, 65535) == lib_mod.QBA_EINVAL and "ctx is NULL" in err()
    assert apply(rates, 17, 0, 16) != 0 and "ctx is NULL" in err()  # n_parties is qba_noise_apply_batched's refusal


def test_noise_profile_kernels_keep_the_curve_shapes_resident_waves():
    """One lists kernel, one apply kernel and per n the sampled kernels of the
    _adv curve kernels' samplers and wave counts; no scratch, no static LDS;
    VGPRs within what the resident waves of qba_montecarlo_curve_shape leave a
    wave (512 per SIMD lane, granule 8), at most 128; no older name pattern."""
    lib = sub("_lib").lib()
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    new = {k: v for k, v in kds.items() if "qba_k_nprof_" in k}
    assert sum("17qba_k_nprof_listsE" in k for k in new) == 1
    assert sum("17qba_k_nprof_applyE" in k for k in new) == 1
    for n in range(1, 16):
        kernel = f"_Z19qba_k_nprof_sampledILi{n}E"
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
        adv = {k[len("_Z26qba_k_mc_curve_sampled_adv"):].split("EEvPK")[0] for k in kds
               if k.startswith(f"_Z26qba_k_mc_curve_sampled_advILi{n}E")}
        assert {k[len("_Z19qba_k_nprof_sampled"):].split("EEvPK")[0] for k in mine} == adv, n
    assert len(new) == 2 + 11 * 3 + 4 * 2  # only curve forms
    for k, v in new.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= 128, (k, v)
        assert not any(s in k for s in ("qba_k_mc_", "qba_k_trace_", "qba_k_protocol", "qba_k_grid_", "_adv", "_noisy",
                                        "qba_k_nettrace_", "coal"))


def test_the_grid_rotation_gives_every_profile_to_every_large_n():
    """Each of the 20 profiles meets every n >= 7, and more than one policy."""
    for n in (7, 11, 15):
        assert {pi for gi, pi in CASES if GRID[gi][0] == n} == set(range(len(PROFILES))), n
    for pi in range(len(PROFILES)):
        assert len({policy_at(gi, p) for gi, p in CASES if p == pi}) >= 2, pi
    assert len(PROFILES) == 20 and len(CASES) == 5 * len(GRID)


# ---------------------------------------------------------------------------
# reach, on the host model alone
# ---------------------------------------------------------------------------
def _reach(mc, name):
    n, nd, sizeL, adv, what, _ = REACH[name]
    eng, w = HostEngine(), 1 << int(n).bit_length()
    ev = dict.fromkeys(EVENTS, 0)
    plain = mc.run_host(n, sizeL, nd, REACH_KEYS, REACH_BASE, eng, adversary=adv)
    assert not plain[:, 3].any()
    if what == "traitors":
        vi = 5 + 5 * np.arange(2, n + 1)
        for i in range(REACH_KEYS):
            key, dis = REACH_BASE + i, int(plain[i, 1])
            lieu = [r for r in range(2, n + 1) if (dis >> r) & 1]
            if not lieu:
                continue
            prof = mc.noise_profile(n, 0, {r: 0x8000 for r in lieu})
            seen = {}
            row = mc.run_host(n, sizeL, nd, 1, key, eng, adversary=adv, noise=prof, party_cls=observing(mc, seen))[0]
            assert np.array_equal(row, mc.run_host(n, sizeL, nd, 1, key, eng, adversary=adv, noise=prof)[0])
            assert row[3] == 0 and row[1] == dis  # the traitor draw does not depend on the lists
            tab = seen["tables"][key]
            honest = [r for r in range(1, n + 1) if not (dis >> r) & 1]
            theirs = {tab.desc(g, u) for g in lieu for u in range(w)} - {()}
            # a traitor checks too, with its own tuple in L, and what it then relays reaches the honest ones
            looked = set().union(*[seen["consulted"].get((key, r), set()) for r in range(2, n + 1)])
            same = all(row[5 + 5 * h] == plain[i, 5 + 5 * h] for h in honest if h >= 2)
            clean = np.asarray(eng.sample(n, key, 0, sizeL))[:, :sizeL]
            if not theirs & looked:
                assert same, (name, key, row.tolist(), plain[i].tolist())
                ev["traitor_rows_unseen"] += int(not np.array_equal(seen["lists"][key], clean))  # the noise did flip bits
            elif not same:
                ev["traitor_rows_seen"] += 1
        assert vi.size
        return ev
    rates, depol = what
    seen = {}
    rows = mc.run_host(n, sizeL, nd, REACH_KEYS, REACH_BASE, eng, adversary=adv, noise=what,
                       party_cls=observing(mc, seen))
    assert np.array_equal(rows, mc.run_host(n, sizeL, nd, REACH_KEYS, REACH_BASE, eng, adversary=adv, noise=what))
    assert not rows[:, 3].any()  # noise never raises a status bit
    if depol:
        for i in range(REACH_KEYS):
            key = REACH_BASE + i
            clean = np.asarray(eng.sample(n, key, 0, sizeL))[:, :sizeL]
            noisy = seen["lists"][key]
            assert np.array_equal(noisy, mc.noisy_lists_profile(n, key, clean, rates, depol))
            for e, c in q_events(n, clean, noisy, depol_hits(mc, key, sizeL, depol)).items():
                ev[e] += c
    else:
        cmd = mc.run_host(n, sizeL, nd, REACH_KEYS, REACH_BASE, eng, adversary=adv,
                          noise=(commander_only(n, MEAN), 0))
        ev["uniform_ok_cmd_fails"] = int(((rows[:, 0] == 1) & (cmd[:, 0] == 0)).sum())
        ev["cmd_ok_uniform_fails"] = int(((rows[:, 0] == 0) & (cmd[:, 0] == 1)).sum())
    return ev


@pytest.fixture(scope="module")
def reached():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = _reach(sub("montecarlo"), name)
        return memo[name]
    return get


@pytest.mark.parametrize("name", list(REACH))
def test_reach_sets_show_the_events_they_were_chosen_for(reached, name):
    ev = reached(name)
    print(name, ev)
    for event in REACH[name][5]:
        assert ev[event] > 0, (name, event, ev)


def test_every_listed_event_is_reached_by_some_set(reached):
    total = {e: sum(reached(name)[e] for name in REACH) for e in EVENTS}
    print(total)
    for event in EVENTS:
        assert total[event] > 0, event
