"""Two edges under the resource compiler that no other test reaches.

Truncation: the compaction kernels (qba_k_compact_emit, qba_k_compact_small)
guard every emit with pos < cap, and simulate_register relies on the guard
whenever a register's support exceeds its buffer.  Here cap < total, with 64
canary slots behind cap: nothing past cap is written, the count is the full
total, the first cap outputs are numpy's.

Second trip: the statevector kernels run grid-stride loops under a cap of
65,536 workgroups (2^24 threads).  One state of 28 qubits (2 GiB) gives the
product pass, hset with K <= 3, xmask and xmulti more threads than that; each
form runs on amplitudes above index 2^25 and is checked on the device against
the tableau.  hset with K = 4, 5 takes its second trip only from 29 qubits
(4 GiB) and 30 (8 GiB): left out."""
import ctypes as C

import numpy as np
import pytest

import stabilizer as st
from conftest import sub

pytestmark = pytest.mark.gpu

CANARY_SLOTS, CANARY = 64, -0x0123456789ABCDEF


def _lists(count, seed):
    rng = np.random.default_rng(seed)
    l0 = rng.integers(0, 4, count, dtype=np.uint8)
    l1 = np.where(rng.random(count) < 0.4, l0 ^ 1, l0).astype(np.uint8)
    return l0, l1, np.nonzero(l0 != l1)[0]


def test_isq_indices_device_form_writes_nothing_past_cap(engine):
    import torch
    call = sub("_lib").call
    count = 40_000
    l0, l1, want = _lists(count, 1)
    d0, d1 = engine.to_device(l0), engine.to_device(l1)
    total = len(want)
    assert total > 4096
    for cap in (0, total - 1, total):
        out = torch.full((cap + CANARY_SLOTS,), CANARY, dtype=torch.int64, device=engine.device)
        found = C.c_int64(-1)
        call("qba_isq_indices", engine.ctx, C.c_void_p(d0.data_ptr()), C.c_void_p(d1.data_ptr()), count,
             C.c_void_p(out.data_ptr()), cap, C.byref(found), engine.stream())
        got = out.cpu().numpy()
        assert found.value == total, cap
        assert np.array_equal(got[:cap], want[:cap]) and np.all(got[cap:] == CANARY), cap


@pytest.mark.parametrize("count", [9_000, 40_000], ids=["one-workgroup", "device-compaction"])
def test_isq_indices_host_form_writes_nothing_past_cap(engine, count):
    call = sub("_lib").call
    l0, l1, want = _lists(count, count)
    d0, d1 = engine.to_device(l0), engine.to_device(l1)
    total = len(want)
    for cap in (1, total // 2 + 1, total - 1):
        out = np.full(cap + CANARY_SLOTS, CANARY, np.int64)
        found = C.c_int64(-1)
        call("qba_isq_indices_host", engine.ctx, C.c_void_p(d0.data_ptr()), C.c_void_p(d1.data_ptr()), count,
             out.ctypes.data, cap, C.byref(found), engine.stream())
        assert found.value == total and cap < total, cap
        assert np.array_equal(out[:cap], want[:cap]) and np.all(out[cap:] == CANARY), cap
    assert np.array_equal(engine.isq_indices(d0, d1), want)  # and the context is as before


def test_support_writes_nothing_past_cap(engine):
    import torch
    call = sub("_lib").call
    q, cap = 17, 1000
    sv = engine.statevector(q, np.array([(0, t, -1) for t in range(q)], np.int32))
    idx = torch.full((cap + CANARY_SLOTS,), CANARY, dtype=torch.int64, device=engine.device)
    prob = torch.full((cap + CANARY_SLOTS,), -7.0, dtype=torch.float64, device=engine.device)
    found = C.c_int64(-1)
    call("qba_sv_support", engine.ctx, C.c_void_p(sv.data_ptr()), q, 1e-24, C.c_void_p(idx.data_ptr()),
         C.c_void_p(prob.data_ptr()), cap, C.byref(found), engine.stream())
    gi, gp = idx.cpu().numpy(), prob.cpu().numpy()
    assert found.value == 1 << q
    assert np.array_equal(gi[:cap], np.arange(cap)) and np.all(gi[cap:] == CANARY)
    assert np.all(np.abs(gp[:cap] - 2.0 ** -q) <= 1e-18) and np.all(gp[cap:] == -7.0)
    with pytest.raises(sub("_lib").QbaError):
        engine.support(sv, q, cap=cap)  # the wrapper reports the overflow


# ---------------------------------------------------------------------------
# second trip of the grid-stride loops
# ---------------------------------------------------------------------------
Q = 28
H, X = "H", "X"
# A product state with amplitudes on both sides of index 2^25 (qubits 0, 1, 2 are
# bits 27, 26, 25), then the gates of one kernel form through qba_sv_apply, which
# folds nothing into the product pass.  Form -> (prefix folded by qba_sv_prepare,
# gates of the form); the comments give the launch the form's gates fuse into.
SPREAD = [(H, 0, -1), (H, 1, -1), (H, 2, -1), (X, 9, -1), (H, 9, -1), (X, 20, -1)]
FORMS = {
    "product":            (SPREAD + [(H, t, -1) for t in (5, 11, 12, 17, 26, 27)] + [(X, 27, -1), (X, 3, -1)], []),
    "hset-k1":            (SPREAD, [(H, 5, -1)]),
    "hset-k1-v":          (SPREAD, [(H, 27, -1)]),
    "hset-k2":            (SPREAD, [(H, 1, -1), (H, 6, -1)]),                   # H on qubit 1 interferes
    "hset-k2-v":          (SPREAD, [(H, 5, -1), (H, 27, -1)]),
    "hset-k3":            (SPREAD, [(H, 3, -1), (H, 9, -1), (H, 6, -1)]),       # |-> back to |1>
    "hset-k3-v":          (SPREAD, [(H, 0, -1), (H, 5, -1), (H, 27, -1)]),
    "xmask":              (SPREAD, [(X, 4, -1)]),                               # vec, M without bit 0
    "xmask-bit0":         (SPREAD, [(X, 27, -1), (X, 4, -1)]),                  # vec, the partner's halves swapped
    "xmask-scalar":       (SPREAD, [(X, 27, -1)]),                              # brep = 0
    "xmask-ctl":          (SPREAD, [(X, 4, 1)]),
    "xmask-ctl-bit0":     (SPREAD, [(X, 4, 1), (X, 27, 1)]),
    "xmask-ctl-scalar":   (SPREAD, [(X, 27, 1)]),                               # brep = 0 under a control
    "xmask-ctl0-scalar":  (SPREAD + [(H, 27, -1)], [(X, 4, 27), (X, 0, 27)]),   # the control is bit 0
    "xmulti":             (SPREAD, [(X, 4, 0), (X, 5, 1), (X, 6, 1)]),
    "xmulti-bit0":        (SPREAD, [(X, 4, 0), (X, 27, 1), (X, 3, -1)]),
    "xmulti-scalar":      (SPREAD + [(H, 27, -1)], [(X, 4, 27), (X, 5, 1)]),    # a control on bit 0
}


@pytest.fixture(scope="module")
def state(engine):
    import torch
    sv = torch.empty(1 << Q, dtype=torch.float64, device=engine.device)
    yield sv
    del sv
    torch.cuda.empty_cache()


def _triples(gates):
    return np.array([(0 if g == H else 1, t, c) for g, t, c in gates], np.int32).reshape(-1, 3)


@pytest.mark.parametrize("form", list(FORMS))
def test_statevector_kernels_second_trip_equals_the_tableau(engine, state, form):
    import torch
    prefix, gates = FORMS[form]
    base, basis = st.distribution(prefix + gates, Q)
    k = len(basis)
    assert k <= 20
    engine.statevector(Q, _triples(prefix), out=state)
    if gates:
        engine.apply_gates(state, Q, _triples(gates))
    idx = torch.nonzero(state).flatten()
    assert idx.numel() == 1 << k, (form, idx.numel(), k)
    amp = state[idx]
    assert float(((amp * amp) - 2.0 ** -k).abs().max()) <= 1e-12
    assert int((idx > 1 << 25).sum()) >= 1 << (k - 1)
    r = idx ^ base
    for b in basis:  # reduce by the echelon basis: members of the subspace end at 0
        r = torch.where((r >> (b.bit_length() - 1)) & 1 == 1, r ^ b, r)
    assert int(torch.count_nonzero(r)) == 0, form
