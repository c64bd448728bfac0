"""The fused Monte-Carlo path without a GPU: the two entry points' envelope,
the host restatement of what the kernels distil (masks_from_lists ==
masks_from_tables of the counted tables) and the static resources of the new
kernels."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, sub
from kd_util import kernel_descriptors
from montecarlo_cases import HOSTILE, HOSTILE_IDS, SWEEP, SWEEP_IDS, hostile_lists
from oracle_engine import OracleEngine

GOLDEN_CASES = json.loads((GOLDEN / "protocol.json").read_text())
GOLDEN_LISTS = np.load(GOLDEN / "protocol_lists.npz")
CU_LDS = 160 * 1024


def _sampled(n, nd, count, n_inst=1, ctx=None, out=None):
    lib_mod = sub("_lib")
    rc = lib_mod.lib().qba_montecarlo_sampled(ctx, n, nd, 0, n_inst, count, out, None)
    return rc, lib_mod.lib().qba_last_error().decode()


def _lists(n, nd, count, n_inst=1, ctx=None, out=None):
    lib_mod = sub("_lib")
    rc = lib_mod.lib().qba_montecarlo_lists(ctx, n, nd, 0, n_inst, count, None, count, (n + 1) * count, out, None)
    return rc, lib_mod.lib().qba_last_error().decode()


def test_symbols_are_exported_and_bound():
    lib_mod = sub("_lib")
    for name in ("qba_montecarlo_sampled", "qba_montecarlo_lists", "qba_montecarlo_shape"):
        assert hasattr(lib_mod.lib(), name) and name in lib_mod.SIGNATURES
    eng = sub("engine").Engine
    assert callable(eng.montecarlo_sampled) and callable(eng.montecarlo_lists)
    assert sub("montecarlo").ST_RANGE == 4


@pytest.mark.parametrize("call", [_sampled, _lists], ids=["sampled", "lists"])
def test_envelope_is_checked_before_ctx(call):
    lib_mod = sub("_lib")
    for n in (0, -1, 16, 1000):
        rc, msg = call(n, 0, 10)
        assert rc == lib_mod.QBA_EINVAL and "n_parties" in msg
    for n, nd in ((1, 2), (7, 8), (15, 16), (7, -1)):
        rc, msg = call(n, nd, 10)
        assert rc == lib_mod.QBA_EINVAL and "n_dishonest" in msg
    for count in (1 << 31, (1 << 31) + 5, 1 << 40, (1 << 64) - 1):
        rc, msg = call(7, 2, count)
        assert rc == lib_mod.QBA_EINVAL and "count" in msg
    for n, nd, count in ((1, 0, 0), (1, 1, 5), (7, 2, (1 << 31) - 1), (15, 15, 100)):  # only the device is missing
        rc, msg = call(n, nd, count)
        assert rc == lib_mod.QBA_EINVAL and "ctx is NULL" in msg


def _same(n, lists, sizeL):
    mc = sub("montecarlo")
    a = mc.masks_from_lists(n, lists)
    b = mc.masks_from_tables(n, OracleEngine().count_tables(n, sizeL, lists=lists))
    assert set(a) == set(b) == {"pnz", "hmask", "czero", "rep"}
    assert a["pnz"] == b["pnz"]
    for k in ("hmask", "czero", "rep"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    return a


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_masks_of_hostile_lists_equal_the_tables(case):
    li = hostile_lists(case)
    for i in range(1 if li.strides[0] == 0 else case["keys"]):
        _same(case["n"], np.array(li[i]), case["sizeL"])


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c["name"] for c in GOLDEN_CASES])
def test_masks_of_golden_lists_equal_the_tables(case):
    _same(case["n"], GOLDEN_LISTS[case["name"]], case["sizeL"])


@pytest.mark.parametrize("n", [3, 7, 11])
@pytest.mark.parametrize("sizeL", [0, 1, 5, 64, 300])
def test_masks_of_sampled_lists_equal_the_tables(n, sizeL):
    import oracle_lib
    dummy = {"nfac": 0, "desc": np.zeros((0, 6), np.int32), "pat": np.zeros(1, np.uint64),
             "apat": np.zeros(1, np.uint64), "thr": np.zeros(1, np.uint64)}
    for seed in (1, 77):
        li = oracle_lib.sample(n, seed, 0, sizeL, dummy, dummy, True) if sizeL else np.zeros((n + 1, 0), np.uint8)
        m = _same(n, li, sizeL)
        if sizeL == 0:
            w = 1 << n.bit_length()
            assert m["pnz"] == 0 and not m["hmask"].any() and not m["rep"].any()
            assert np.all(m["czero"] == (1 << (n + 1)) - 1) and m["rep"].shape == (w, n + 1)


def test_masks_reject_out_of_range_values_at_q_positions_only():
    mc = sub("montecarlo")
    li = np.array([[0, 1, 2], [1, 1, 3], [2, 3, 0], [3, 2, 1]], np.uint8)  # n = 3, w = 4; entry 1 is not Q
    ok = mc.masks_from_lists(3, li)
    off = li.copy()
    off[2, 1] = 4
    got = mc.masks_from_lists(3, off)
    assert got["pnz"] == ok["pnz"] and all(np.array_equal(got[k], ok[k]) for k in ("hmask", "czero", "rep"))
    bad = li.copy()
    bad[2, 0] = 4
    with pytest.raises(ValueError):
        mc.masks_from_lists(3, bad)


@pytest.fixture(scope="module")
def kds():
    return kernel_descriptors(Path(sub("_lib").LIB_PATH))


def test_new_kernels_use_no_scratch_and_keep_the_protocol_kernel_findable(kds):
    new = {k: v for k, v in kds.items() if "qba_k_mc_" in k}
    assert any("qba_k_mc_lists" in k for k in new)
    for n in range(1, 16):  # a sampling kernel for every n, the closed form's up to 11
        assert any(k.startswith(f"_Z16qba_k_mc_sampledILi{n}E") for k in new), n
    for n in range(1, 12):
        assert any(k.startswith(f"_Z16qba_k_mc_sampledILi{n}ELi2E") for k in new), n
    for k, v in new.items():
        assert v["scratch"] == 0, k
        assert "qba_k_protocol" not in k
        # the shapes count on 4 waves per SIMD (16 per CU): 512 VGPRs / 4
        assert v["vgprs"] <= 128, (k, v["vgprs"])


def _shape(n):
    lib = sub("_lib").lib()
    waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
    assert lib.qba_montecarlo_shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
    return waves.value, lds.value, wgs.value


def _design_rows():
    """The LDS budget table of DESIGN.md section 13: n -> (waves, LDS bytes, workgroups per CU)."""
    text = (ROOT / "DESIGN.md").read_text()
    rows = {}
    for m in re.finditer(r"^\| *(\d+) *\| *(\d+) *\| *([\d,]+) *\| *(\d+) *\| *(\d+) *\|$", text, re.M):
        rows[int(m.group(1))] = (int(m.group(2)), int(m.group(3).replace(",", "")), int(m.group(4)),
                                 int(m.group(5)))
    return rows


def test_lds_per_n_fits_the_workgroups_per_cu_design_states(kds):
    rows = _design_rows()
    assert sorted(rows) == list(range(1, 16))
    for n in range(1, 16):
        waves, lds, wgs = _shape(n)
        assert (waves, lds, wgs) == rows[n][:3], n
        assert rows[n][3] == waves * wgs            # resident waves per CU
        assert 1 <= waves <= 16 and wgs >= 1 and wgs * lds <= CU_LDS and waves * wgs <= 16
        g, w = n + 1, 1 << n.bit_length()
        per_wave = 2064 + (2 * g * (g * w + 1) + 3) // 4 * 16  # ProtoShared + the mailbox
        assert lds >= waves * per_wave and (lds - waves * per_wave) % 16 == 0
        # all of it is dynamic: the static segment of the sampling kernels is empty
        mine = [v for k, v in kds.items() if k.startswith(f"_Z16qba_k_mc_sampledILi{n}E")]
        assert mine and all(v["lds"] == 0 for v in mine)
    rc = sub("_lib").lib().qba_montecarlo_shape(16, None, None, None)
    assert rc == sub("_lib").QBA_EINVAL


def test_run_rejects_an_unknown_path():
    with pytest.raises(ValueError):
        sub("montecarlo").run(3, 10, 1, 4, 0, engine=None, path="other")
