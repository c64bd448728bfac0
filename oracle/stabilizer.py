"""Exact measurement distribution of an H / X / CX circuit on up to 64 qubits,
from a stabilizer tableau (Aaronson & Gottesman, Phys. Rev. A 70, 052328).

TEST INFRASTRUCTURE ONLY (see oracle/tfg_oracle.py header).  Written from the
gate definitions; it shares nothing with the product's compiler, with
resource.py or with the C twin, and never splits a circuit into registers.

Convention (the engine's and oracle/statevector.py's): qubit 0 is the most
significant bit of a basis index, so qubit q is bit N-1-q of an outcome.
Gates are (name, target, control) with control = -1 for none.

The state |0...0> after such a circuit is a stabilizer state.  Measured in
the computational basis it is uniform over an affine subspace of GF(2)^N:

    support = base ^ span(basis),   every outcome of it with probability 2^-k,

k = len(basis).  With the N stabilizer generators (-1)^r X^x Z^z brought to
a form in which k of them have linearly independent x parts and the other
N - k have x = 0, the span is that of the k x parts (a generator maps a basis
state b of the support to +-|b ^ x>), and the base solves z . b = r over the
N - k generators (-1)^r Z^z.

A subspace is the canonical pair (base, basis): basis in reduced echelon form
by leading bit, descending, base with every leading bit cleared -- two
subspaces are equal iff their pairs are.
"""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple

Subspace = Tuple[int, Tuple[int, ...]]


# ---------------------------------------------------------------------------
# GF(2) linear algebra on Python ints
# ---------------------------------------------------------------------------
def reduce_basis(vectors: Iterable[int]) -> Tuple[int, ...]:
    """Reduced echelon basis of span(vectors): distinct leading bits, no basis
    vector holds another's leading bit; descending."""
    basis: List[int] = []
    for v in vectors:
        v = int(v)
        for b in basis:
            v = min(v, v ^ b)
        if v:
            top = 1 << (v.bit_length() - 1)
            basis = [b ^ v if b & top else b for b in basis]
            basis.append(v)
            basis.sort(reverse=True)
    return tuple(basis)


def rank(vectors: Iterable[int]) -> int:
    return len(reduce_basis(vectors))


def reduce_point(point: int, basis: Sequence[int]) -> int:
    """The representative of point + span(basis) with every leading bit of the
    (reduced) basis cleared."""
    p = int(point)
    for b in basis:
        if p >> (b.bit_length() - 1) & 1:
            p ^= b
    return p


def subspace(base: int, vectors: Iterable[int]) -> Subspace:
    """Canonical pair of base ^ span(vectors)."""
    basis = reduce_basis(vectors)
    return reduce_point(base, basis), basis


def contains(sub: Subspace, point: int) -> bool:
    base, basis = sub
    return reduce_point(int(point) ^ base, basis) == 0


def same_subspace(a: Subspace, b: Subspace) -> bool:
    return subspace(*a) == subspace(*b)


def shifted(sub: Subspace, offset: int) -> Subspace:
    """{p ^ offset : p in sub}."""
    return subspace(sub[0] ^ int(offset), sub[1])


def dimension(sub: Subspace) -> int:
    return len(sub[1])


def points(sub: Subspace) -> List[int]:
    """Every point, ascending (2^k of them: small k only)."""
    out = [sub[0]]
    for b in sub[1]:
        out += [p ^ b for p in out]
    return sorted(out)


# ---------------------------------------------------------------------------
# tableau: the N stabilizer generators, row i = (-1)^r[i] X^x[i] Z^z[i]
# ---------------------------------------------------------------------------
def _g_sum(x1: int, z1: int, x2: int, z2: int) -> int:
    """Sum over the qubits of the exponent of i that multiplying the Pauli
    (x1, z1) onto (x2, z2) contributes (Aaronson-Gottesman's g)."""
    y1, xo1, zo1 = x1 & z1, x1 & ~z1, ~x1 & z1
    plus = (y1 & z2 & ~x2) | (xo1 & z2 & x2) | (zo1 & x2 & ~z2)
    minus = (y1 & x2 & ~z2) | (xo1 & z2 & ~x2) | (zo1 & x2 & z2)
    return bin(plus).count("1") - bin(minus).count("1")


class Tableau:
    def __init__(self, nqubits: int):
        if not 1 <= nqubits <= 64:
            raise ValueError("1 <= nqubits <= 64")
        self.n = nqubits
        self.x = [0] * nqubits
        self.z = [1 << (nqubits - 1 - q) for q in range(nqubits)]  # |0...0>: Z_q
        self.r = [0] * nqubits

    def _bit(self, q: int) -> int:
        if not 0 <= q < self.n:
            raise ValueError(f"qubit {q} outside [0, {self.n})")
        return self.n - 1 - q

    def h(self, a: int) -> None:
        s = self._bit(a)
        for i in range(self.n):
            xa, za = self.x[i] >> s & 1, self.z[i] >> s & 1
            self.r[i] ^= xa & za
            if xa != za:
                self.x[i] ^= 1 << s
                self.z[i] ^= 1 << s

    def x_gate(self, a: int) -> None:
        s = self._bit(a)
        for i in range(self.n):
            self.r[i] ^= self.z[i] >> s & 1  # X anticommutes with Z and Y

    def cx(self, control: int, target: int) -> None:
        if control == target:
            raise ValueError("control == target")
        a, b = self._bit(control), self._bit(target)
        for i in range(self.n):
            xa, za = self.x[i] >> a & 1, self.z[i] >> a & 1
            xb, zb = self.x[i] >> b & 1, self.z[i] >> b & 1
            self.r[i] ^= xa & zb & (xb ^ za ^ 1)
            self.x[i] ^= xa << b
            self.z[i] ^= zb << a

    def apply(self, gates: Iterable[Tuple[str, int, int]]) -> "Tableau":
        for name, tgt, ctl in gates:
            if name == "H" and ctl < 0:
                self.h(tgt)
            elif name == "X":
                self.x_gate(tgt) if ctl < 0 else self.cx(ctl, tgt)
            else:
                raise ValueError(f"gate {name!r} (control {ctl}) is outside H, X, CX")
        return self

    def _mul(self, h: int, i: int) -> None:
        """row h <- row i * row h"""
        e = 2 * self.r[h] + 2 * self.r[i] + _g_sum(self.x[i], self.z[i], self.x[h], self.z[h])
        if e % 2:
            raise AssertionError("generators do not commute")
        self.r[h] = e % 4 // 2
        self.x[h] ^= self.x[i]
        self.z[h] ^= self.z[i]

    def distribution(self) -> Subspace:
        """The support of a computational-basis measurement (the tableau is
        consumed: its rows are row-reduced in place)."""
        n, lead = self.n, 0
        for s in range(n - 1, -1, -1):  # eliminate on the x parts
            piv = next((i for i in range(lead, n) if self.x[i] >> s & 1), None)
            if piv is None:
                continue
            for a in (self.x, self.z, self.r):
                a[lead], a[piv] = a[piv], a[lead]
            for i in range(n):
                if i != lead and self.x[i] >> s & 1:
                    self._mul(i, lead)
            lead += 1
        basis = self.x[:lead]
        # rows lead.. are (-1)^r Z^z: solve z . b = r, free bits 0
        rows = [(self.z[i], self.r[i]) for i in range(lead, n)]
        solved = []  # (pivot bit, z, r) with the pivot bit in no other row
        for z, r in rows:
            for s, zz, rr in solved:
                if z >> s & 1:
                    z, r = z ^ zz, r ^ rr
            if not z:
                if r:
                    raise AssertionError("inconsistent Z stabilizers")
                continue
            s = z.bit_length() - 1
            solved = [(t, zz ^ z, rr ^ r) if zz >> s & 1 else (t, zz, rr) for t, zz, rr in solved]
            solved.append((s, z, r))
        if len(solved) != n - lead:
            raise AssertionError("Z stabilizers are not independent")
        base = 0
        for s, _, r in solved:
            base |= r << s
        return subspace(base, basis)


def distribution(gates: Iterable[Tuple[str, int, int]], nqubits: int) -> Subspace:
    """Support of measuring |0...0> after `gates`: canonical (base, basis);
    every outcome base ^ (subset XOR of basis) has probability 2^-len(basis)."""
    return Tableau(nqubits).apply(gates).distribution()
