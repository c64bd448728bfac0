"""The sizeL-curve Monte-Carlo calls without a GPU: the three entry points'
envelope, the launch shape with the accumulator area, the static resources of
the curve kernels, the host specification (curve_host) with the prefix
property it rests on, and the CLI's argument errors."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT, sub
from kd_util import kernel_descriptors
from oracle_engine import OracleEngine

CU_LDS = 160 * 1024
CURVE_MAX = 32
U32 = C.c_uint32


def _arr(counts):
    return None if counts is None else (U32 * max(len(counts), 1))(*counts)


def _sampled(n, nd, counts, n_counts=None, n_inst=1, ctx=None, out=None):
    lib_mod = sub("_lib")
    k = len(counts) if n_counts is None else n_counts
    rc = lib_mod.lib().qba_montecarlo_curve_sampled(ctx, n, nd, 0, n_inst, _arr(counts), k, out, None)
    return rc, lib_mod.lib().qba_last_error().decode()


def _lists(n, nd, counts, n_counts=None, n_inst=1, ctx=None, out=None):
    lib_mod = sub("_lib")
    k = len(counts) if n_counts is None else n_counts
    ld = counts[-1] if counts else 0
    rc = lib_mod.lib().qba_montecarlo_curve_lists(ctx, n, nd, 0, n_inst, _arr(counts), k, None, ld, (n + 1) * ld,
                                                  out, None)
    return rc, lib_mod.lib().qba_last_error().decode()


def test_symbols_are_exported_and_bound():
    lib_mod = sub("_lib")
    for name in ("qba_montecarlo_curve_sampled", "qba_montecarlo_curve_lists", "qba_montecarlo_curve_shape"):
        assert hasattr(lib_mod.lib(), name) and name in lib_mod.SIGNATURES
    eng = sub("engine").Engine
    assert callable(eng.montecarlo_curve_sampled) and callable(eng.montecarlo_curve_lists)
    assert callable(eng.montecarlo_curve_shape)
    mc = sub("montecarlo")
    assert callable(mc.curve) and callable(mc.curve_host)
    assert lib_mod.lib().qba_build_flags() == 0


@pytest.mark.parametrize("call", [_sampled, _lists], ids=["sampled", "lists"])
def test_envelope_is_checked_before_ctx(call):
    lib_mod = sub("_lib")
    EINVAL = lib_mod.QBA_EINVAL
    for n in (0, -1, 16, 1000):
        rc, msg = call(n, 0, [10])
        assert rc == EINVAL and "n_parties" in msg
    for n, nd in ((1, 2), (7, 8), (15, 16), (7, -1)):
        rc, msg = call(n, nd, [10])
        assert rc == EINVAL and "n_dishonest" in msg
    # the checkpoint list: after n_parties and n_dishonest, before ctx
    rc, msg = call(16, 0, None, n_counts=1)
    assert rc == EINVAL and "n_parties" in msg
    rc, msg = call(7, 8, None, n_counts=1)
    assert rc == EINVAL and "n_dishonest" in msg
    rc, msg = call(7, 2, None, n_counts=1)
    assert rc == EINVAL and "counts is NULL" in msg
    for k in (0, -1, CURVE_MAX + 1, 1000):
        rc, msg = call(7, 2, list(range(CURVE_MAX + 1)), n_counts=k)
        assert rc == EINVAL and "n_counts" in msg, k
    for counts in ([5, 5], [0, 0], [1, 2, 2], [3, 2], [0, 10, 9, 20], list(range(31)) + [29]):
        rc, msg = call(7, 2, counts)
        assert rc == EINVAL and "increasing" in msg, counts
    for counts in ([1 << 31], [0, 1 << 31], [5, (1 << 32) - 1], list(range(31)) + [(1 << 31) + 7]):
        rc, msg = call(7, 2, counts)
        assert rc == EINVAL and "2^31" in msg, counts
    # only the device is missing
    for n, nd, counts in ((1, 0, [0]), (1, 1, [5]), (7, 2, [0, (1 << 31) - 1]), (15, 15, list(range(0, 64, 2))),
                          (3, 1, [0, 1, 5, 60])):
        assert len(counts) <= CURVE_MAX
        rc, msg = call(n, nd, counts)
        assert rc == EINVAL and "ctx is NULL" in msg, counts


def test_engine_validation_mirrors_the_single_count_calls():
    Engine, QbaError = sub("engine").Engine, sub("_lib").QbaError
    ok = Engine._check_curve(7, 2, 4, np.array([0, 1, 5]))
    assert ok == [0, 1, 5] and all(type(c) is int for c in ok)
    for n, nd, inst, counts in ((7, 8, 1, [1]), (7, -1, 1, [1]), (7, 2, -1, [1]), (7, 2, 1, []),
                                (7, 2, 1, list(range(33))), (7, 2, 1, [2, 2]), (7, 2, 1, [3, 1]),
                                (7, 2, 1, [-1, 4]), (7, 2, 1, [1 << 31]), (7, 2, 1, 5)):
        with pytest.raises(QbaError):
            Engine._check_curve(n, nd, inst, counts)


def _shape(fn, n):
    waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
    assert fn(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
    return waves.value, lds.value, wgs.value


def _design_rows():
    """The LDS table of DESIGN.md section 13.2: n -> (waves, LDS bytes,
    workgroups per CU, resident waves, accumulator bytes, waves of 13.1)."""
    text = (ROOT / "DESIGN.md").read_text()
    rows = {}
    cell = r" *([\d,]+) *\|"
    for m in re.finditer(r"^\|" + cell * 7 + "$", text, re.M):
        v = [int(x.replace(",", "")) for x in m.groups()]
        rows[v[0]] = tuple(v[1:])
    return rows


@pytest.fixture(scope="module")
def kds():
    return kernel_descriptors(Path(sub("_lib").LIB_PATH))


def test_shape_adds_the_accumulator_area_and_matches_design():
    lib = sub("_lib").lib()
    rows = _design_rows()
    assert sorted(rows) == list(range(1, 16))
    fewer = []
    for n in range(1, 16):
        waves0, lds0, _ = _shape(lib.qba_montecarlo_shape, n)
        waves, lds, wgs = _shape(lib.qba_montecarlo_curve_shape, n)
        assert 1 <= waves <= 16 and wgs >= 1 and wgs * lds <= CU_LDS and waves * wgs <= 16
        g, w = n + 1, 1 << n.bit_length()
        per_wave = 2064 + (2 * g * (g * w + 1) + 3) // 4 * 16   # ProtoShared + the mailbox (section 13.1)
        acc = (2 * w * g + 2 + 3) // 4 * 16                     # 2 w G + 2 words, rounded to 16 bytes
        assert acc <= 2064
        tables = lds0 - waves0 * per_wave                       # the staged tables are those of section 13.1
        assert tables >= 0 and lds - tables == waves * (per_wave + acc), n
        assert waves <= waves0
        # no other wave count keeps more waves resident
        for nw in range(1, 17):
            need = tables + nw * (per_wave + acc)
            if need <= CU_LDS:
                assert min(CU_LDS // need, max(16 // nw, 1)) * nw <= waves * wgs, (n, nw)
        if waves < waves0:
            fewer.append(n)
        assert rows[n] == (waves, lds, wgs, waves * wgs, acc, waves0), n
    assert fewer, "the accumulator area costs a wave at some n"
    assert lib.qba_montecarlo_curve_shape(16, None, None, None) == sub("_lib").QBA_EINVAL
    assert lib.qba_montecarlo_curve_shape(0, None, None, None) == sub("_lib").QBA_EINVAL
    assert sub("engine").Engine.montecarlo_curve_shape(7) == _shape(lib.qba_montecarlo_curve_shape, 7)


def test_curve_kernels_use_no_scratch_no_static_lds_and_at_most_128_vgprs(kds):
    new = {k: v for k, v in kds.items() if "qba_k_mc_curve_" in k}
    assert sum("qba_k_mc_curve_lists" in k for k in new) == 1
    for n in range(1, 16):  # a sampling kernel for every n, the closed form's up to 11
        assert any(k.startswith(f"_Z22qba_k_mc_curve_sampledILi{n}E") for k in new), n
    for n in range(1, 12):
        assert any(k.startswith(f"_Z22qba_k_mc_curve_sampledILi{n}ELi2E") for k in new), n
    for k, v in new.items():
        assert v["scratch"] == 0, k
        assert v["vgprs"] <= 128, (k, v["vgprs"])
        assert v["lds"] == 0, k
    # the wave count a kernel is compiled for is the reported shape's
    lib = sub("_lib").lib()
    for n in range(1, 16):
        waves = _shape(lib.qba_montecarlo_curve_shape, n)[0]
        samp = 2 if n <= 11 else 1
        assert any(k.startswith(f"_Z22qba_k_mc_curve_sampledILi{n}ELi{samp}ELi{waves}E") for k in new), n


COUNTS = [0, 1, 5, 60]


@pytest.mark.parametrize("n,nd,base", [(3, 1, 1000), (7, 2, 3000)])
def test_curve_host_is_the_stack_of_run_host_and_lists_are_prefixes(n, nd, base):
    import oracle_lib
    mc = sub("montecarlo")
    inst = 6
    eng = OracleEngine()
    got = mc.curve_host(n, COUNTS, nd, inst, base, eng)
    assert got.shape == (len(COUNTS), inst, mc.out_words(n)) and got.dtype == np.int32
    # the c_max lists, sampled once; their first c columns are the lists at c
    dummy = {"nfac": 0, "desc": np.zeros((0, 6), np.int32), "pat": np.zeros(1, np.uint64),
             "apat": np.zeros(1, np.uint64), "thr": np.zeros(1, np.uint64)}
    full = np.stack([oracle_lib.sample(n, base + i, 0, COUNTS[-1], dummy, dummy, True) for i in range(inst)])
    assert full.shape == (inst, n + 1, COUNTS[-1])
    for j, c in enumerate(COUNTS):
        want = mc.run_host(n, c, nd, inst, base, eng)
        assert np.array_equal(got[j], want), c
        if c:
            short = np.stack([oracle_lib.sample(n, base + i, 0, c, dummy, dummy, True) for i in range(inst)])
            assert np.array_equal(short, full[:, :, :c]), c
        assert np.array_equal(mc.run_host(n, c, nd, inst, base, eng, lists=full[:, :, :c]), want), c
    assert np.array_equal(mc.curve_host(n, COUNTS, nd, inst, base, eng, lists=full), got)
    assert not got[:, :, 3].any()
    assert any(not np.array_equal(got[0], got[j]) for j in range(1, len(COUNTS)))


def test_curve_batches_and_rejects_like_run():
    mc = sub("montecarlo")
    with pytest.raises(ValueError):
        mc.curve(3, [1, 2], 1, -1, 0, engine=None)
    with pytest.raises(ValueError):
        mc.curve(3, [1, 2], 1, 4, 0, engine=None, batch=0)
    with pytest.raises(ValueError):                 # run itself is unchanged
        mc.run(3, 10, 1, 4, 0, engine=None, path="other")

    class Fake:
        calls = []

        def montecarlo_curve_sampled(self, n, nd, key, b, counts, out=None):
            import torch
            self.calls.append((key, b, list(counts)))
            rows = torch.zeros((len(counts), b, mc.out_words(n)), dtype=torch.int32)
            rows[:, :, 0] = 1
            return rows

    fake = Fake()
    got = mc.curve(3, [4, 9], 1, 10, (1 << 64) - 2, fake, batch=4)
    assert fake.calls == [((1 << 64) - 2, 4, [4, 9]), (2, 4, [4, 9]), (6, 2, [4, 9])]
    assert list(got) == [4, 9] and all(s["runs"] == 10 and s["successes"] == 10 for s in got.values())
    assert mc.curve(3, [4, 9], 1, 0, 0, fake) == {c: mc.summarize(3, np.zeros((0, 24), np.int32)) for c in (4, 9)}


def _cli(*args):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "tfg---quantum-byzantine-agreement_amd.tfg", *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=str(ROOT))


def test_cli_rejects_curve_without_runs_and_too_many_checkpoints():
    out = _cli("50", "2", "--parties", "7", "--curve", "16,64")
    assert out.returncode == 2 and "--curve needs --runs" in out.stderr
    many = ",".join(str(c) for c in range(1, 34))   # 33 checkpoints, the positional one among them
    out = _cli("33", "2", "--parties", "7", "--runs", "4", "--curve", many)
    assert out.returncode == 2 and "at most 32" in out.stderr
    out = _cli("50", "2", "--parties", "7", "--runs", "4", "--curve", ",".join(str(c) for c in range(1, 33)))
    assert out.returncode == 2 and "at most 32" in out.stderr   # 32 values and a 33rd positional
