"""Circuit pairs that are not the shipped ones, for the Monte-Carlo kernels'
paths the shipped programs never take (tests/test_gpu_montecarlo_programs.py,
tests/test_montecarlo_programs.py).  TEST INFRASTRUCTURE ONLY.

Every pair keeps the shipped Q circuit (identity permutation) and replaces the
not-Q circuit by one from H and controlled X gates.  In `general3` and the
`narrow` programs group 0 is still a copy of group 1, so L0 == L1 at the not-Q
entries and the rounds never consult them; in `tables7` and `big15` it is not,
and the protocol reads most not-Q entries as Q-correlated ones with repeated
values.  None is the closed form's distribution, and all but `tables7`
(canonical tables at an n where the shipped program is closed) run the general
alias-table sampler.

Which wave count a program runs is decided by qba_mc_shape from the bytes of
its tables, against the canonical program's the kernels are built for.  That
program randomises n * nQ bits (group 0 copies group 1).  A register of H / X /
CX gates has a uniform support of at most 256 patterns and costs one H qubit
per pattern bit, so the largest tables the API accepts randomise all
(n + 1) * nQ qubits: (n + 1) * nQ / 8 factors of 256 entries.

  larger tables   `big15`, H on all 64 qubits: 2,064 entries against the
                  canonical 1,824, and the curve kernel runs 3 of its 4 waves.
                  No other n gets there: at n = 11 the same circuit reaches
                  1,552 entries against 1,312, and all 7 (6) waves still fit.
  smaller tables  the `narrow` programs: several small workgroups keep more
                  wavefronts resident on a CU than one workgroup of the
                  compiled wave count does, and the launcher picks them.

The entries of PROGRAMS say which kernel of which program runs fewer waves;
the GPU tests assert it through Engine.montecarlo_program_shape, never from
here.  The compiled programs (what Engine.compile returns: the C twin samples
from them) are kept in tests/golden/montecarlo_programs.npz, written by
tests/golden/gen_montecarlo_programs.py on a GPU, so that the CPU tests have
them; the GPU tests hold the compiler to the file, and
tests/test_stabilizer_oracle.py holds the file to the tableau distribution of
each circuit (oracle/stabilizer.py), which shares nothing with the compiler.
"""
from pathlib import Path

import numpy as np

import oracle_lib
from conftest import sub

SAMPLER_GENERAL, SAMPLER_TABLES = 0, 1  # as qba_montecarlo_program_shape reports them


def general_pair(n):
    """Group 0 = copy of group 1 and group 3 = copy of group 2 in the not-Q
    circuit, groups 1 and 2 uniform (general alias-table sampler)."""
    resource = sub("resource")
    nq = resource.n_qubits(n)
    notq = resource.Gate((n + 1) * nq)
    for qb in range(nq, 3 * nq):
        notq.add_operation("H", targets=qb)
    for j in range(nq):
        notq.add_operation("X", targets=j, controls=nq + j)
        notq.add_operation("X", targets=3 * nq + j, controls=2 * nq + j)
    return notq, resource.qCorrelated(n, nq, perm=[1, 2, 3])


def narrow_pair(n, bits):
    """A not-Q circuit of `bits` random bits: H on the first `bits` qubits from
    group 1 on, group 0 a copy of group 1, every other qubit 0.  Its alias
    tables hold 256 entries per 8 bits (and 2^(bits % 8) for the rest)."""
    resource = sub("resource")
    nq = resource.n_qubits(n)
    assert nq <= bits <= n * nq
    notq = resource.Gate((n + 1) * nq)
    for qb in range(nq, nq + bits):
        notq.add_operation("H", targets=qb)
    for j in range(nq):
        notq.add_operation("X", targets=j, controls=nq + j)
    return notq, resource.qCorrelated(n, nq, perm=list(range(1, n + 1)))


def shifted_copy_pair(n):
    """The shipped not-Q circuit with group 0 a copy of group 2 instead of
    group 1: the canonical table layout, so the canonical-table sampler, but
    not the closed form's distribution -- the one way to that sampler's
    kernels at n <= 11.  L0 != L1 at most of its not-Q entries, which the
    protocol then reads as Q-correlated entries with repeated values."""
    resource = sub("resource")
    nq = resource.n_qubits(n)
    notq = resource.Gate((n + 1) * nq)
    for qb in range(nq, (n + 1) * nq):
        notq.add_operation("H", targets=qb)
    for j in range(nq):
        notq.add_operation("X", targets=j, controls=2 * nq + j)
    return notq, resource.qCorrelated(n, nq, perm=list(range(1, n + 1)))


def all_h_pair(n):
    """H on every qubit: (n + 1) * nQ random bits, the largest tables a circuit
    of the API's gate set compiles to, and L0 independent of L1."""
    resource = sub("resource")
    nq = resource.n_qubits(n)
    notq = resource.Gate((n + 1) * nq)
    for qb in range((n + 1) * nq):
        notq.add_operation("H", targets=qb)
    return notq, resource.qCorrelated(n, nq, perm=list(range(1, n + 1)))


# name -> (n, circuit pair, kernels that must run fewer waves than compiled:
# "single" = montecarlo_sampled, "curve" = montecarlo_curve_sampled; sampler)
PROGRAMS = {
    "general3": (3, lambda: general_pair(3), (), SAMPLER_GENERAL),
    "tables7": (7, lambda: shifted_copy_pair(7), (), SAMPLER_TABLES),
    "narrow10": (10, lambda: narrow_pair(10, 7), ("single",), SAMPLER_GENERAL),
    "narrow11": (11, lambda: narrow_pair(11, 7), ("curve",), SAMPLER_GENERAL),
    "narrow12": (12, lambda: narrow_pair(12, 9), ("curve",), SAMPLER_GENERAL),
    "narrow14": (14, lambda: narrow_pair(14, 7), ("single",), SAMPLER_GENERAL),
    "big15": (15, lambda: all_h_pair(15), ("curve",), SAMPLER_GENERAL),
}
LARGER_TABLES = ["big15"]  # more table entries than the canonical program of their n
REDUCED = [name for name, (_, _, kernels, _) in PROGRAMS.items() if kernels]


GOLDEN_PROGRAMS = Path(__file__).resolve().parent / "golden" / "montecarlo_programs.npz"
_KEYS = ("desc", "pat", "apat", "thr")


def host_info(name):
    """Program info of PROGRAMS[name] as Engine.compile returns it, from the
    golden file (no device)."""
    n, _, _, sampler = PROGRAMS[name]
    with np.load(GOLDEN_PROGRAMS) as z:
        prog = {kind: {k: z[f"{name}.{kind}.{k}"] for k in _KEYS} for kind in ("notq", "q")}
    for p in prog.values():
        p["nfac"] = len(p["desc"])
    return {"n": n, "nq": int(n).bit_length(), "notq": prog["notq"], "q": prog["q"],
            "canonical": sampler == SAMPLER_TABLES, "closed": False}


def same_program(a, b):
    return a["nfac"] == b["nfac"] and all(np.array_equal(a[k], b[k]) for k in _KEYS)


def twin_lists(info, base, inst, count):
    """[inst, n+1, count] uint8 (read-only): instance i is the C twin's sample of
    entries [0, count) under key base + i (the closed-form schedule when the
    program info says so: a shipped program of n <= 11)."""
    n, closed = info["n"], bool(info.get("closed", False))
    with oracle_lib.single_thread():  # many tiny samples
        li = np.stack([oracle_lib.sample(n, (base + i) & ((1 << 64) - 1), 0, count, info["notq"], info["q"], closed)
                       for i in range(inst)]) if inst else np.zeros((0, n + 1, count), np.uint8)
    li = np.ascontiguousarray(li)
    li.setflags(write=False)
    return li
