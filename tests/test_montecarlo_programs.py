"""The non-shipped test programs (tests/montecarlo_programs.py) without a GPU:
the shape query's exports and envelope, the compiled programs of the golden file, and the
host specification on a general program's lists -- masks_from_lists ==
masks_from_tables, and curve_host == the stack of run_host."""
import ctypes as C

import numpy as np
import pytest

from conftest import sub
from montecarlo_programs import LARGER_TABLES, PROGRAMS, host_info, twin_lists
from oracle_engine import OracleEngine

BASE = 0xA11CE


@pytest.fixture(scope="module")
def general3():
    info = host_info("general3")
    return info, twin_lists(info, BASE, 16, 130)


def test_program_shape_is_exported_bound_and_checks_its_envelope():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    assert hasattr(lib, "qba_montecarlo_program_shape") and "qba_montecarlo_program_shape" in lib_mod.SIGNATURES
    assert callable(sub("engine").Engine.montecarlo_program_shape)
    out = [C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int()]
    refs = [C.byref(x) for x in out]
    for n in (0, -1, 16):
        assert lib.qba_montecarlo_program_shape(None, n, 0, *refs) == lib_mod.QBA_EINVAL
        assert b"n_parties" in lib.qba_last_error()
    assert lib.qba_montecarlo_program_shape(None, 7, 0, None, *refs[1:]) == lib_mod.QBA_EINVAL
    for curve in (0, 1):  # only the context is missing
        assert lib.qba_montecarlo_program_shape(None, 7, curve, *refs) == lib_mod.QBA_EINVAL
        assert b"ctx is NULL" in lib.qba_last_error()


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_golden_programs_and_their_lists(name):
    """Uniform factors of distinct patterns, more entries than the canonical
    program only where the list says so, a GHZ Q program, and lists with every
    value below w whose not-Q entries keep L0 == L1 where group 0 copies group 1."""
    n = PROGRAMS[name][0]
    info = host_info(name)
    nq, w = info["nq"], 1 << info["nq"]
    canonical = 256 * ((n * nq + 7) // 8 - 1) + (1 << (n * nq - 8 * ((n * nq + 7) // 8 - 1)))
    entries = len(info["notq"]["pat"])
    assert (entries > canonical) == (name in LARGER_TABLES) and (entries == canonical) == info["canonical"]
    assert entries == sum(1 << bits for bits, *_ in info["notq"]["desc"].tolist())
    for bits, uniform, off, *_ in info["notq"]["desc"].tolist():
        assert uniform == 1 and len(set(info["notq"]["pat"][off:off + (1 << bits)].tolist())) == 1 << bits
    assert info["q"]["nfac"] == 1 and len(info["q"]["pat"]) == w
    N = (n + 1) * nq
    assert set(info["q"]["pat"].tolist()) == {sum(r << (N - (g + 1) * nq) for g in range(n + 1)) for r in range(w)}
    li = twin_lists(info, 1, 4, 200)
    assert li.shape == (4, n + 1, 200) and li.max() < w
    q = li[:, 0] != li[:, 1]
    assert q.any() and not q.all()
    if name in ("tables7", "big15"):  # group 0 is no copy of group 1: most not-Q entries look Q-correlated
        assert q.mean() > 0.9
        return
    for i in range(4):
        qi = li[i][:, q[i]].astype(np.int64)
        assert (np.diff(np.sort(qi, axis=0), axis=0) != 0).all()  # Q entries: n + 1 distinct values


def test_masks_of_a_general_programs_lists_equal_the_tables(general3):
    mc = sub("montecarlo")
    _, lists = general3
    for i in range(len(lists)):
        for sizeL in (0, 1, 5, 64, 130):
            li = np.array(lists[i, :, :sizeL])
            a = mc.masks_from_lists(3, li)
            b = mc.masks_from_tables(3, OracleEngine().count_tables(3, sizeL, lists=li))
            assert a["pnz"] == b["pnz"]
            for k in ("hmask", "czero", "rep"):
                assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (i, sizeL, k)
    # group 3 copies group 2 at the not-Q entries, which the masks never see
    nq_entries = lists[:, 0] == lists[:, 1]
    assert np.array_equal(lists[:, 3][nq_entries], lists[:, 2][nq_entries])


@pytest.mark.parametrize("nd", [0, 1, 2])
def test_curve_host_is_the_stack_of_run_host_on_a_general_programs_lists(general3, nd):
    mc = sub("montecarlo")
    _, lists = general3
    counts = [0, 1, 2, 3, 5, 63, 64, 65, 127, 130]
    got = mc.curve_host(3, counts, nd, len(lists), BASE, OracleEngine(), lists=lists)
    assert got.shape == (len(counts), len(lists), mc.out_words(3)) and got.dtype == np.int32
    for j, c in enumerate(counts):
        want = mc.run_host(3, c, nd, len(lists), BASE, OracleEngine(), lists=lists[:, :, :c])
        assert np.array_equal(got[j], want), (nd, c)
    assert not got[:, :, 3].any()
    if nd == 1:  # both outcomes, and the checkpoints tell apart
        assert 0 < got[:, :, 0].sum() < got[:, :, 0].size and len({s.tobytes() for s in got}) >= 2
