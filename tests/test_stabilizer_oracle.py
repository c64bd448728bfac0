"""oracle/stabilizer.py (the tableau reference of the resource compiler) held
to the dense numpy statevector, then the golden programs of
tests/golden/montecarlo_programs.npz and the generated circuit pairs of
tests/resource_circuits.py held to it.  No device.

The golden file was written by the GPU compile and the GPU tests hold the
compiler to the file; here each of its programs is compared with the tableau
distribution of the circuit it was compiled from, which shares no code with
the compiler."""
import json

import numpy as np
import pytest

import statevector as sv_oracle
import stabilizer as st
from conftest import GOLDEN
from montecarlo_programs import PROGRAMS, host_info
from resource_circuits import (FACTORS15, NS, PAIRS_PER_N, Q_WIDE_N, SAMPLED, WORDS3, chained_h, misplaced_x, n_qubits,
                               pair, perm_mask, program_subspace, register_dims)


def _dense_check(gates, nq, what=""):
    """Support set exactly the dense run's, every nonzero probability 2^-k within 1e-12."""
    base, basis = st.distribution(gates, nq)
    probs = sv_oracle.probabilities(sv_oracle.run(gates, nq))
    idx = np.nonzero(probs > 1e-20)[0]
    want = st.points((base, basis))
    assert len(want) == 1 << len(basis)
    assert idx.tolist() == want, (what, gates)
    assert np.all(np.abs(probs[idx] - 2.0 ** -len(basis)) <= 1e-12), (what, gates)
    assert abs(probs.sum() - 1.0) <= 1e-12
    assert all(st.contains((base, basis), int(i)) for i in idx[:64])
    return base, basis


def _random_gates(rng, nq, length):
    gates = []
    for _ in range(length):
        kind = rng.integers(4)
        t = int(rng.integers(nq))
        if kind == 0 or nq == 1 and kind >= 2:
            gates.append(("H", t, -1))
        elif kind == 1:
            gates.append(("X", t, -1))
        else:
            c = int(rng.integers(nq - 1))
            gates.append(("X", t, c + (c >= t)))
    return gates


def test_random_circuits_equal_the_dense_statevector():
    rng = np.random.default_rng(0x7AB1EA0)
    seen_dims = set()
    for trial in range(320):
        nq = 1 + trial % 12
        gates = _random_gates(rng, nq, int(rng.integers(0, 4 * nq + 2)))
        _, basis = _dense_check(gates, nq, f"trial {trial}")
        seen_dims.add((nq, len(basis)))
    assert any(2 * k >= nq for nq, k in seen_dims if nq >= 6) and any(k == 0 for _, k in seen_dims)
    assert any(0 < k < nq for nq, k in seen_dims)


STRUCTURED = {
    "nothing": (3, []),
    "h_twice": (2, [("H", 0, -1), ("H", 0, -1)]),
    "h_thrice_and_x": (2, [("H", 1, -1), ("H", 1, -1), ("X", 0, -1), ("H", 1, -1)]),
    "minus_state_h": (1, [("X", 0, -1), ("H", 0, -1), ("H", 0, -1)]),       # H|-> = |1>
    "bell_then_h_on_the_target": (2, [("H", 0, -1), ("X", 1, 0), ("H", 1, -1)]),
    "bell_then_h_on_the_control": (2, [("H", 0, -1), ("X", 1, 0), ("H", 0, -1)]),
    "bell_then_h_on_both": (2, [("H", 0, -1), ("X", 1, 0), ("H", 0, -1), ("H", 1, -1)]),  # back to 00 + 11
    "ghz_then_h": (4, [("H", 0, -1)] + [("X", t, 0) for t in (1, 2, 3)] + [("H", 2, -1)]),
    # H . CX . H on the target is a controlled Z: the sign shows after one more H
    "cz_on_plus_plus": (2, [("H", 0, -1), ("H", 1, -1), ("H", 1, -1), ("X", 1, 0), ("H", 1, -1), ("H", 1, -1)]),
    "cz_on_plus_plus_then_h0": (2, [("H", 0, -1), ("H", 1, -1), ("H", 1, -1), ("X", 1, 0), ("H", 1, -1), ("H", 0, -1)]),
    "cz_on_one_plus": (2, [("X", 0, -1), ("H", 1, -1), ("H", 1, -1), ("X", 1, 0), ("H", 1, -1), ("H", 1, -1)]),
    "cz_on_minus_minus": (2, [("X", 0, -1), ("X", 1, -1), ("H", 0, -1), ("H", 1, -1), ("H", 1, -1), ("X", 1, 0),
                              ("H", 1, -1), ("H", 0, -1), ("H", 1, -1)]),
    "cx_reversed_by_h": (2, [("X", 1, -1), ("H", 0, -1), ("H", 1, -1), ("X", 1, 0), ("H", 0, -1), ("H", 1, -1)]),
    "shared_control_run": (6, [("H", 2, -1)] + [("X", t, 2) for t in (0, 1, 3, 4, 5)]),
    "shared_control_run_twice": (5, [("H", 0, -1), ("H", 3, -1)] + [("X", t, 0) for t in (1, 2, 4)]
                                 + [("X", t, 3) for t in (1, 4)] + [("X", 1, 0)]),
    "shared_control_then_h_on_it": (4, [("H", 1, -1), ("X", 0, 1), ("X", 2, 1), ("X", 3, 1), ("H", 1, -1), ("X", 0, 1)]),
    "chain": (7, [("H", 0, -1), ("X", 6, -1)] + [("X", t + 1, t) for t in range(6)]),
    "x_between_cx": (3, [("H", 0, -1), ("X", 1, 0), ("X", 1, -1), ("X", 2, 1), ("X", 0, -1)]),
}


@pytest.mark.parametrize("name", list(STRUCTURED))
def test_structured_circuits_equal_the_dense_statevector(name):
    nq, gates = STRUCTURED[name]
    _dense_check(gates, nq, name)


def test_known_answers():
    assert st.distribution([("H", 0, -1), ("X", 1, 0)], 2) == (0, (3,))
    assert st.distribution([("X", 0, -1), ("H", 0, -1), ("H", 0, -1)], 1) == (1, ())
    assert st.distribution([("X", 2, -1)], 3) == (1, ())                       # qubit 0 is the MSB
    assert st.distribution([("H", 0, -1), ("X", 1, 0), ("X", 1, -1)], 2) == (1, (3,))
    assert st.distribution([("H", q, -1) for q in range(64)], 64)[1] == tuple(1 << b for b in range(63, -1, -1))


def test_subspace_helpers():
    a = st.subspace(0b1011, [0b0110, 0b0011, 0b0101])
    assert a[1] == (0b0101, 0b0011) and st.rank([0b0110, 0b0011, 0b0101, 0]) == 2 and st.dimension(a) == 2
    assert st.contains(a, 0b1011 ^ 0b0110) and not st.contains(a, 0b0011)
    assert st.same_subspace(a, (0b1011 ^ 0b0101, (0b0110, 0b0011))) and not st.same_subspace(a, (0, a[1]))
    assert not st.same_subspace(a, (a[0], a[1][:1])) and st.shifted(a, 0b0110) == a and st.shifted(a, 1) != a
    assert st.points(a) == sorted({0b1011, 0b1011 ^ 0b0110, 0b1011 ^ 0b0011, 0b1011 ^ 0b0101})
    assert st.reduce_basis([]) == () and st.subspace(5, []) == (5, ())


def test_shipped_circuits_equal_their_dense_probabilities():
    gates = json.loads((GOLDEN / "gates.json").read_text())
    checked = 0
    for n_s, g in gates.items():
        if g["size"] > 21:  # 2^21 amplitudes: the largest dense run worth its time here
            continue
        n, nq, big = int(n_s), g["nq"], g["size"]
        _, basis = _dense_check([tuple(o) for o in g["notq"]], big, f"not-Q n={n}")
        assert len(basis) == n * nq
        for case in g["q"]:
            base, basis = _dense_check([tuple(o) for o in case["ops"]], big, f"Q n={n}")
            assert len(basis) == nq and base == st.reduce_point(perm_mask(n, case["perm"]), basis)
        checked += 1
    assert checked >= 5


# ---------------------------------------------------------------------------
# the golden programs against the tableau of their circuits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_golden_program_is_its_circuits_distribution(name):
    n, make, _, _ = PROGRAMS[name]
    big = (n + 1) * n_qubits(n)
    notq, q = make()
    info = host_info(name)
    assert program_subspace(info["notq"]) == st.distribution(notq.ops, big), (name, "notq")
    got = st.shifted(program_subspace(info["q"]), perm_mask(n, q.perm))
    assert got == st.distribution(q.ops, big), (name, "q")


def test_program_subspace_refuses_what_is_not_a_uniform_subspace():
    good = host_info("big15")["notq"]  # 8 factors of 8 bits, four to a column word
    assert st.dimension(program_subspace(good)) > 0

    def broken(**kw):
        p = {k: np.array(v) for k, v in good.items() if k != "nfac"}
        p["nfac"] = good["nfac"]
        for k, (i, v) in kw.items():
            p[k].reshape(-1)[i] = v
        return p
    bits0 = int(good["desc"][0][0])
    assert bits0 >= 2
    for bad in (broken(pat=(1, good["pat"][0])),                       # a repeated pattern
                broken(pat=(3, int(good["pat"][3]) ^ (1 << 62))),       # leaves the coset
                broken(thr=(0, 1 << 31)), broken(desc=(1, 0)),          # not uniform
                broken(desc=(4, int(good["desc"][0][4]) + 1))):         # column fields overlap / leave the word
        with pytest.raises(AssertionError):
            program_subspace(bad)


# ---------------------------------------------------------------------------
# the generated pairs stay inside the compiler's envelope (about the inputs)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_generated_pairs_are_inside_the_envelope_and_varied(n):
    nq = n_qubits(n)
    big = (n + 1) * nq
    kinds, widths, interleaved, dims_q, bare_x = set(), set(), 0, [], 0
    for i in range(PAIRS_PER_N):
        notq, q, kind = pair(n, i)
        kinds.add(kind)
        assert pair(n, i)[0].ops == notq.ops and pair(n, i)[1].ops == q.ops  # seeded
        for gate in (notq, q):
            regs = register_dims(gate.ops, big)
            assert all(1 <= len(qs) <= 16 and d <= 8 for qs, d in regs), (n, i)
            assert sum(d for _, d in regs) == st.dimension(st.distribution(gate.ops, big))
        regs = register_dims(notq.ops, big)
        widths |= {d for _, d in regs}
        interleaved += sum(1 for qs, _ in regs if len({qb // nq for qb in qs}) > 1)
        dims_q.append(sum(d for _, d in register_dims(q.ops, big)))
        assert sorted(q.perm.tolist()) == list(range(1, n + 1))
        assert any(c >= 0 for _, _, c in notq.ops)
        bare_x += any(g == "X" and c < 0 for g, _, c in notq.ops)
    assert kinds == {"ghz", "extended"} and interleaved >= PAIRS_PER_N and 2 * bare_x >= PAIRS_PER_N
    assert {0, 1} <= widths and max(widths) >= min(8, big // 2)
    assert max(dims_q) > nq


def test_the_named_pairs_have_the_shapes_they_are_named_for():
    big = 64
    for i, want in ((SAMPLED["factors15"][1], FACTORS15), (SAMPLED["words3"][1], WORDS3)):
        regs = register_dims(pair(15, i)[0].ops, big)
        assert [d for _, d in regs[:len(want)]] == want and all(d == 0 for _, d in regs[len(want):])
        assert [qs[0] for qs, _ in regs[:len(want)]] == list(range(len(want)))
    n, i = SAMPLED["q_wide"]
    assert n == Q_WIDE_N
    regs = register_dims(pair(n, i)[1].ops, (n + 1) * n_qubits(n))
    assert [d for _, d in regs[:4]] == [8, 8, 8, 1] and sorted(d for _, d in regs[4:]) == [8, 8]
    rng = np.random.default_rng(5)
    for m in (9, 17):
        (qs, d), = [r for r in register_dims(chained_h(7, m, rng).ops, 24) if len(r[0]) > 1]
        assert len(qs) == m and d == m
    bad = misplaced_x(7, rng, list(range(1, 8)))
    assert st.distribution(bad.ops, 24)[0] != st.reduce_point(perm_mask(7, bad.perm), st.distribution(bad.ops, 24)[1])
