"""The tally of Monte-Carlo result rows on the CPU: montecarlo.tally_host (the
numpy specification of qba_montecarlo_tally) against a row-by-row loop,
summary_from_tally against summarize on the host reference's rows, and the C
ABI's envelope and the kernel's resources without a device."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from conftest import sub
from kd_util import kernel_descriptors
from montecarlo_cases import HOSTILE, hostile_lists
from montecarlo_tally_cases import synthetic_rows, tally_loop
from oracle_engine import OracleEngine

mc = sub("montecarlo")

# (n, dishonest, sizeL) -> (successes, dishonest commanders) of 67 instances from key 0xA11CE
SAMPLED = {(3, 1, 2): (46, 24), (4, 2, 4): (47, 35), (7, 2, 8): (51, 23), (11, 3, 12): (53, 16)}
SAMPLED_INST, SAMPLED_BASE = 67, 0xA11CE
# hostile set -> empty-V_i rows of its 8
HOSTILE_EMPTY = {"n7-d4-L60-dup_cmd": 5, "n8-d7-L64-dup_cmd": 5, "n12-d6-L80-dup_cmd": 1, "n15-d8-L96-dup_cmd": 1}
SHARED = ("runs", "successes", "rate", "empty_vi_runs", "decisions")


@pytest.fixture(scope="module")
def host_rows():
    """run_host's rows of every set, computed once, read-only: {name: (n, rows)}."""
    sets = {}
    for (n, nd, size_l) in SAMPLED:
        sets[f"n{n}-d{nd}-L{size_l}"] = (n, mc.run_host(n, size_l, nd, SAMPLED_INST, SAMPLED_BASE, OracleEngine()))
    for case in HOSTILE:
        if case["name"] in HOSTILE_EMPTY:
            sets[case["name"]] = (case["n"], mc.run_host(case["n"], case["sizeL"], case["nDishonest"], case["keys"],
                                                         case["base"], OracleEngine(), lists=hostile_lists(case)))
    for _, rows in sets.values():
        rows.setflags(write=False)
    assert len(sets) == len(SAMPLED) + len(HOSTILE_EMPTY)
    return sets


# ---------------------------------------------------------------------------
# C ABI without a device
# ---------------------------------------------------------------------------
def _call(n=7, rows=True, n_inst=4, k=1, tally=True, select=0, capture=False, cap=0):
    lib = sub("_lib").lib()
    buf = (C.c_int64 * 64)()  # never read: every call here fails before ctx is used
    at = C.cast(buf, C.c_void_p)
    rc = lib.qba_montecarlo_tally(None, n, at if rows else None, n_inst, k, 0, at if tally else None, select,
                                  at if capture else None, cap, None)
    return rc, lib.qba_last_error().decode()


def test_tally_is_exported_and_checks_its_envelope():
    lib_mod = sub("_lib")
    assert hasattr(lib_mod.lib(), "qba_montecarlo_tally") and "qba_montecarlo_tally" in lib_mod.SIGNATURES
    assert (mc.TALLY_WORDS, mc.SEL_FAILED, mc.SEL_EMPTY_VI, mc.SEL_STATUS) == (32, 1, 2, 4)
    refused = [(dict(n=0), "n_parties"), (dict(n=16), "n_parties"), (dict(n=-1), "n_parties"),
               (dict(k=0), "n_slices"), (dict(k=33), "n_slices"), (dict(n_inst=-1), "n_instances"),
               (dict(select=-1), "select"), (dict(select=8), "select"), (dict(cap=-1), "capture_cap"),
               (dict(tally=False), "tally_dev"), (dict(rows=False), "rows_dev"),
               (dict(select=1, cap=4), "capture_dev"), (dict(select=7, cap=1), "capture_dev")]
    for kw, word in refused:
        rc, msg = _call(**kw)
        assert rc == lib_mod.QBA_EINVAL and word in msg and "ctx is NULL" not in msg, (kw, msg)
    inside = [dict(), dict(n=1), dict(n=15, k=32), dict(n_inst=0, rows=False), dict(select=7, cap=0),
              dict(select=0, cap=9), dict(select=3, cap=9, capture=True)]
    for kw in inside:  # only the device is missing
        rc, msg = _call(**kw)
        assert rc == lib_mod.QBA_EINVAL and "ctx is NULL" in msg, (kw, msg)


def test_tally_kernel_resources():
    """One wavefront per workgroup, a tile of 64 rows in dynamic LDS, the
    partial tallies in registers: no scratch and no static LDS."""
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    hits = [v for k, v in kds.items() if "qba_k_mc_tally" in k]
    assert len(hits) == 1
    assert hits[0]["scratch"] == 0 and hits[0]["lds"] == 0
    assert 64 * ((4 + 5 * 16) | 1) * 4 <= 64 * 1024  # the dynamic request at n = 15


# ---------------------------------------------------------------------------
# summary_from_tally against summarize on the host reference's rows
# ---------------------------------------------------------------------------
def test_summary_from_tally_equals_summarize_on_host_rows(host_rows):
    for name, (n, rows) in host_rows.items():
        tally, matches = mc.tally_host(n, rows)
        assert tally.shape == (1, mc.TALLY_WORDS) and tally.dtype == np.int64 and matches == [[]]
        got, want = mc.summary_from_tally(n, tally[0]), mc.summarize(n, rows)
        assert {k: got[k] for k in SHARED} == want, name
        assert set(got) == set(SHARED) | {"cmd_dishonest_runs", "cmd_dishonest_successes", "accept", "reject", "sent"}
        per = rows[:, 4 + 5:].reshape(len(rows), n, 5).astype(np.int64)
        assert (got["accept"], got["reject"], got["sent"]) == tuple(int(per[:, :, f].sum()) for f in (2, 3, 4))
        assert tally[0].tolist() == tally_loop(n, rows)[0], name
    for (n, nd, size_l), (ok, cmd) in SAMPLED.items():
        s = mc.summary_from_tally(n, mc.tally_host(n, host_rows[f"n{n}-d{nd}-L{size_l}"][1])[0][0])
        assert (s["runs"], s["successes"], s["cmd_dishonest_runs"]) == (SAMPLED_INST, ok, cmd), (n, s)
    for name, empty in HOSTILE_EMPTY.items():
        n, rows = host_rows[name]
        s = mc.summary_from_tally(n, mc.tally_host(n, rows)[0][0])
        assert (s["runs"], s["empty_vi_runs"]) == (8, empty), (name, s)


def test_host_rows_hold_what_every_tally_word_needs(host_rows):
    """About the inputs: successes and failures, empty-V_i rows and -1
    decisions, a dishonest commander with a success and with a failure."""
    total = np.zeros(mc.TALLY_WORDS, np.int64)
    for n, rows in host_rows.values():
        total += mc.tally_host(n, rows)[0][0]
    T = total.tolist()
    assert 0 < T[mc.T_SUCCESSES] < T[mc.T_RUNS]
    assert T[mc.T_EMPTY_VI] > 0 and T[mc.T_DEC_NEG] > 0
    assert 0 < T[mc.T_CMD_DISHONEST_OK] < T[mc.T_CMD_DISHONEST]
    assert T[mc.T_STATUS_ROWS] == 0 and T[mc.T_STATUS_OR] == 0 and T[mc.T_CAPTURE] == 0
    assert T[mc.T_ACCEPT] > 0 and T[mc.T_REJECT] > 0 and T[mc.T_SENT] > 0
    assert sum(1 for v in T[mc.T_DEC0:]) == 16 and sum(1 for v in T[mc.T_DEC0:] if v) >= 4


def test_selected_matches_on_host_rows(host_rows):
    for name, (n, rows) in host_rows.items():
        for sel in range(8):
            tally, matches = mc.tally_host(n, rows, inst_base=1000, select=sel)
            want, want_m = tally_loop(n, rows, 1000, sel)
            assert tally[0].tolist() == want and matches == [want_m], (name, sel)
        fails = [1000 + i for i in np.nonzero(rows[:, 0] == 0)[0]]
        assert mc.tally_host(n, rows, 1000, mc.SEL_FAILED)[1] == [fails]


# ---------------------------------------------------------------------------
# synthetic rows: statuses whose other fields are not zero, 64-bit sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 7, 11, 15])
def test_tally_host_equals_a_row_by_row_loop_on_synthetic_rows(n):
    rows = synthetic_rows(n, 301, seed=n)
    st = rows[:, 3]
    assert set(st.tolist()) == {0, 1, 2, 4}
    assert np.all(rows[st != 0][:, 11] != 0)   # status rows keep their other fields
    assert rows[:, 4 + 5 + 2::5].min() > (1 << 31) - 1 - 1000
    for sel in (0, 1, 2, 4, 7):
        tally, matches = mc.tally_host(n, rows, inst_base=(1 << 40) + 5, select=sel)
        want, want_m = tally_loop(n, rows, (1 << 40) + 5, sel)
        assert tally[0].tolist() == want and matches == [want_m], sel
    t = mc.tally_host(n, rows)[0][0]
    assert t[mc.T_STATUS_ROWS] == 43 and t[mc.T_STATUS_OR] == 7 and t[mc.T_ACCEPT] > 1 << 32
    assert t[11:15].tolist() == [0, 0, 0, 0]
    # a tally that did not skip the status rows would differ
    as_normal = rows.copy()
    as_normal[:, 3] = 0
    assert not np.array_equal(mc.tally_host(n, as_normal)[0][0][5:10], t[5:10])
    # two halves add to the whole; inst_base shifts the matches
    a, ma = mc.tally_host(n, rows[:150], inst_base=10, select=7)
    b, mb = mc.tally_host(n, rows[150:], inst_base=160, select=7)
    whole, mw = mc.tally_host(n, rows, inst_base=10, select=7)
    both = a + b
    both[0, mc.T_STATUS_OR] = a[0, mc.T_STATUS_OR] | b[0, mc.T_STATUS_OR]
    assert np.array_equal(both, whole) and ma[0] + mb[0] == mw[0]
    assert [i + 90 for i in mw[0]] == mc.tally_host(n, rows, inst_base=100, select=7)[1][0]
    # slices are independent
    stack = np.stack([rows, as_normal, rows[::-1]])
    ts, ms = mc.tally_host(n, stack, select=1)
    for j in range(3):
        tj, mj = mc.tally_host(n, stack[j], select=1)
        assert np.array_equal(ts[j], tj[0]) and ms[j] == mj[0]


def test_summary_from_tally_refuses_status_rows():
    QbaError = sub("_lib").QbaError
    rows = synthetic_rows(3, 50, seed=1, statuses=(2, 4))
    tally = mc.tally_host(3, rows)[0][0]
    with pytest.raises(QbaError) as e:
        mc.summary_from_tally(3, tally)
    assert f"{int(tally[mc.T_STATUS_ROWS])} instance(s)" in str(e.value) and "statuses: 6" in str(e.value)
    with pytest.raises(ValueError):
        mc.tally_host(3, rows[:, :-1])
    with pytest.raises(ValueError):
        mc.tally_host(3, rows, select=8)
    empty = mc.summary_from_tally(3, mc.tally_host(3, rows[:0])[0][0])
    assert empty["runs"] == 0 and empty["rate"] == 0.0 and empty["decisions"] == {}
