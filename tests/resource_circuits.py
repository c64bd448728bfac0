"""Seeded circuit pairs the resource compiler has never been held to, and the
reading of a compiled program as an affine subspace
(tests/test_stabilizer_oracle.py, tests/test_gpu_resource_compile.py).
TEST INFRASTRUCTURE ONLY.

The reference for every pair is oracle/stabilizer.py's tableau on the whole
gate list.  Nothing here asks the compiler, resource.py's circuits or the C
twin what the answer is; the register bookkeeping below only keeps the
generated circuits inside the compiler's envelope (a register's support at
most 256 outcomes) and is itself checked against the tableau (`register_dims`).

What the envelope allows (worked out from qba_plan_program's layout rules; the
GPU tests assert each on the compiled programs):

  factors   adjacent factors merge while the product of their supports stays
            <= 256, so two neighbours that stay apart carry >= 9 bits, and a
            bit costs a qubit: f factors need 9 * (f // 2) + (f % 2) qubits.
            N <= 64 gives at most 15 factors (widths 1, 8, 1, ..., 8, 1 on 64
            qubits, `FACTORS15`); 16 would need 72.  The compiler's "more than
            16 alias tables" refusal cannot be reached through
            qba_resource_compile; csrc/sanitize/plan_check.cpp drives
            qba_plan_program with 16 and 17 factors directly.
  words     a factor opens the next column word when it does not fit the 32
            bits of the current one, so a word is left with >= 25 bits used
            and the factor that leaves it makes 33: a third word needs
            25 + 33 = 58 qubits (n >= 14), a fourth 25 + 25 + 33 = 83.  A
            not-Q program therefore never leaves Philox block 0 (words x1, x2,
            x3; `WORDS3` uses all three).  A Q program has x1 alone in block
            0 and leaves it from 33 column bits on (`Q_WIDE`).
  Q         the shipped GHZ layer puts every qubit into one of nQ <= 4
            registers: at most 4 factors of 8 bits, exactly one word.  More
            column bits need qubits outside the GHZ registers, so the extended
            Q circuits drop the GHZ CX of some (group, bit) qubits and build
            further registers on them, in front of the permutation's X layer.
"""
import numpy as np

from conftest import sub
from stabilizer import distribution, rank, subspace

NS = (3, 7, 11, 12, 15)
PAIRS_PER_N = 12


def n_qubits(n):
    return int(n).bit_length()


# ---------------------------------------------------------------------------
# a compiled program as an affine subspace
# ---------------------------------------------------------------------------
def program_subspace(prog):
    """The distribution a program (Engine.compile's info["notq"] / ["q"]) samples,
    as oracle/stabilizer.py's canonical (base, basis) -- after asserting that it
    is uniform over it: every factor uniform, its 2^bits patterns distinct and a
    coset of a `bits`-dimensional space, the factors' column fields disjoint and
    inside their 32-bit words, their spaces independent."""
    desc = np.asarray(prog["desc"], dtype=np.int64).reshape(-1, 6)
    pat, thr = prog["pat"], prog["thr"]
    assert len(desc) == prog["nfac"] >= 1
    base, dirs, total, used, end = 0, [], 0, {}, 0
    for f, (bits, uniform, off, cw, cs, uw) in enumerate(desc.tolist()):
        k = 1 << bits
        assert 0 <= bits <= 8 and off == end and off + k <= len(pat), (f, bits, off)
        end = off + k
        assert uniform == 1 and uw == -1, f"factor {f} is not uniform"
        assert all(int(t) == 1 << 32 for t in thr[off:off + k]), f"factor {f}: thresholds of a uniform factor"
        pats = [int(p) for p in pat[off:off + k]]
        assert len(set(pats)) == k, f"factor {f}: repeated patterns"
        d = [p ^ pats[0] for p in pats[1:]]
        assert rank(d) == bits, f"factor {f}: {k} patterns are no coset of a {bits}-dimensional space"
        field = ((1 << bits) - 1) << cs
        assert cw >= 0 and cs >= 0 and cs + bits <= 32 and not used.get(cw, 0) & field, f"factor {f}: column field"
        used[cw] = used.get(cw, 0) | field
        base ^= pats[0]
        dirs += d
        total += bits
    assert end == len(pat), "table entries outside every factor"
    assert rank(dirs) == total, "the factors' spaces are not independent"
    return subspace(base, dirs)


def perm_mask(n, perm):
    """Field g = perm[g - 1] of an outcome (the Q circuit's classical X mask)."""
    nq = n_qubits(n)
    big = (n + 1) * nq
    m = 0
    for g in range(1, n + 1):
        m |= int(perm[g - 1]) << (big - (g + 1) * nq)
    return m


def column_bits(prog):
    return int(np.asarray(prog["desc"]).reshape(-1, 6)[:, 0].sum())


def column_words(prog):
    return int(np.asarray(prog["desc"]).reshape(-1, 6)[:, 3].max()) + 1


# ---------------------------------------------------------------------------
# registers
# ---------------------------------------------------------------------------
def _components(gates, big):
    par = list(range(big))

    def find(a):
        while par[a] != a:
            par[a] = par[par[a]]
            a = par[a]
        return a
    for _, t, c in gates:
        if c >= 0:
            par[find(t)] = find(c)
    regs = {}
    for qb in range(big):
        regs.setdefault(find(qb), []).append(qb)
    return sorted(regs.values())


def register_dims(gates, big):
    """[(qubits, support dimension)] of the CX-connected components, ascending
    smallest qubit; each dimension from the tableau on the component alone."""
    out = []
    for qs in _components(gates, big):
        pos = {qb: i for i, qb in enumerate(qs)}
        local = [(g, pos[t], pos[c] if c >= 0 else -1) for g, t, c in gates if t in pos]
        out.append((qs, len(distribution(local, len(qs))[1])))
    return out


STYLES = ("chain", "fanout", "tree")


def register_gates(rng, qubits, style=None, bare_x=True, all_h=False):
    """Gates of one CX-connected register on `qubits` (any order) with a support
    of at most 256 outcomes.  Single qubits: |0>, |1>, |+> or |->.  Larger ones:
    X on some qubits, H on up to 8, then a CX chain, a CX fan-out from one
    control or a random CX tree, and (half of the time) an H on a qubit the CX
    gates have entangled, followed by one more CX: interference.
    bare_x = False (Q circuits, whose classical X gates must be exactly the
    permutation's): an X is always followed by an H on its qubit."""
    qs = [int(qb) for qb in qubits]
    m = len(qs)
    if m == 1:
        kind = "plus" if all_h else ("zero", "one", "plus", "plus", "minus")[rng.integers(5)]
        if kind == "one" and not bare_x:
            kind = "minus"
        return {"zero": [], "one": [("X", qs[0], -1)], "plus": [("H", qs[0], -1)],
                "minus": [("X", qs[0], -1), ("H", qs[0], -1)]}[kind]
    style = style or STYLES[rng.integers(len(STYLES))]
    for _ in range(50):
        order = [qs[i] for i in rng.permutation(m)]
        h = min(m, 8) if all_h else int(rng.integers(1, min(m, 8) + 1))
        gates = []
        for i, qb in enumerate(order):
            flip = not all_h and rng.integers(4) == 0
            if flip and (bare_x or i < h):
                gates.append(("X", qb, -1))
            if i < h:
                gates.append(("H", qb, -1))
        if style == "chain":
            gates += [("X", order[i + 1], order[i]) for i in range(m - 1)]
        elif style == "fanout":
            gates += [("X", order[i], order[0]) for i in range(1, m)]
        else:
            for i in range(1, m):
                a, b = order[i], order[int(rng.integers(i))]
                gates.append(("X", a, b) if rng.integers(2) else ("X", b, a))
        if not all_h and rng.integers(2):
            a, b = (order[i] for i in rng.choice(m, 2, replace=False))
            gates += [("H", a, -1), ("X", b, a) if rng.integers(2) else ("X", a, b)]
            if bare_x and rng.integers(2):
                gates.append(("X", b, -1))
        pos = {qb: i for i, qb in enumerate(qs)}
        local = [(g, pos[t], pos[c] if c >= 0 else -1) for g, t, c in gates]
        if len(distribution(local, m)[1]) <= 8:
            return gates
    raise AssertionError("no register within the envelope in 50 draws")


def interleave(rng, lists):
    """One gate list holding every list's gates in their own order, the lists
    shuffled into each other."""
    left = [list(g) for g in lists if g]
    out = []
    while left:
        i = int(rng.integers(len(left)))
        out.append(left[i].pop(0))
        if not left[i]:
            left.pop(i)
    return out


def _gate(big, ops, perm=None):
    g = sub("resource").Gate(big)
    for name, t, c in ops:
        g.add_operation(name, targets=t, controls=None if c < 0 else c)
    if perm is not None:
        g.perm = np.asarray(perm, dtype=np.int64)
    return g


SIZES = (1, 1, 1, 2, 2, 3, 3, 4, 5, 6, 8, 10, 14)


def _split(rng, qubits, sizes=SIZES):
    qs = [qubits[i] for i in rng.permutation(len(qubits))]
    out = []
    while qs:
        m = min(len(qs), int(sizes[rng.integers(len(sizes))]))
        out.append(qs[:m])
        qs = qs[m:]
    return out


def random_notq(n, rng):
    """Registers of 1..14 qubits drawn from a shuffle of all (n+1)*nQ qubits (so
    a register's qubits lie in several groups), their gates interleaved."""
    big = (n + 1) * n_qubits(n)
    return _gate(big, interleave(rng, [register_gates(rng, qs) for qs in _split(rng, list(range(big)))]))


def notq_from_widths(n, rng, widths):
    """Register i has smallest qubit i and a support of 2^widths[i]: H on all its
    widths[i] qubits (the others drawn from the qubits past len(widths)), joined
    by CX gates.  Qubits left over are |0> or |1>."""
    big = (n + 1) * n_qubits(n)
    rest = [int(x) for x in rng.permutation(np.arange(len(widths), big))]
    regs = []
    for i, w in enumerate(widths):
        regs.append([i] + rest[:w - 1])
        rest = rest[w - 1:]
    ops = [register_gates(rng, qs, all_h=True) for qs in regs]
    ops += [[("X", qb, -1)] for qb in rest[::2]]
    return _gate(big, interleave(rng, ops))


def shipped_q(n, perm):
    return sub("resource").qCorrelated(n, n_qubits(n), perm=list(perm))


def shipped_notq(n):
    return sub("resource").notQCorrelated(n, n_qubits(n))


def extended_q(n, rng, perm, pre_h=None, extras=None):
    """The shipped Q circuit with (a) the GHZ CX of some (group, bit) qubits
    dropped and further registers built on those qubits, and (b) an H on some
    GHZ targets, all in front of the permutation's X layer: the X gates stay
    classical (only CX gates target their qubits afterwards) and the mask is
    still field g = perm(g).
    pre_h[j]: GHZ targets of bit j that get an H (register j: 1 + pre_h[j] bits);
    extras: [(qubits, all_h)] sizes of the further registers.  None: random."""
    nq = n_qubits(n)
    big = (n + 1) * nq
    targets = {j: [g * nq + j for g in range(1, n + 1)] for j in range(nq)}
    if extras is None:
        free = [t for j in range(nq) for t in targets[j] if rng.integers(3) == 0]
        extras = [(len(qs), False) for qs in _split(rng, free, (1, 1, 2, 3, 4, 6, 8))] if free else []
    n_free = sum(m for m, _ in extras)
    pool, left = [], [n] * nq  # a bit keeps the GHZ targets its pre_h asks for
    for t in (int(x) for x in rng.permutation(np.arange(nq, big))):
        if len(pool) < n_free and left[t % nq] > (0 if pre_h is None else pre_h[t % nq]):
            pool.append(t)
            left[t % nq] -= 1
    assert len(pool) == n_free
    free = set(pool)
    head = [("H", j, -1) for j in range(nq)]
    for j in range(nq):
        mine = [t for t in targets[j] if t not in free]
        k = min(len(mine), 7, int(rng.integers(0, 8)) if pre_h is None else pre_h[j])
        head += [("H", int(t), -1) for t in rng.permutation(mine)[:k]]
    regs = []
    for m, all_h in extras:
        regs.append(register_gates(rng, pool[:m], bare_x=False, all_h=all_h))
        pool = pool[m:]
    ops = interleave(rng, [head] + regs)
    for g in range(1, n + 1):
        ops += [("X", g * nq + j, -1) for j in range(nq) if int(perm[g - 1]) >> (nq - 1 - j) & 1]
    ops += [("X", t, t % nq) for t in range(nq, big) if t not in free]
    return _gate(big, ops, perm)


def misplaced_x(n, rng, perm):
    """The shipped Q circuit with one bit of the permutation's X layer flipped:
    an X too many or one too few on a qubit of groups 1..n."""
    nq = n_qubits(n)
    q = shipped_q(n, perm)
    t = int(rng.integers(nq, (n + 1) * nq))
    ops = [op for op in q.ops if op != ("X", t, -1)]
    if len(ops) == len(q.ops):
        at = next(i for i, (_, _, c) in enumerate(ops) if c >= 0)
        ops.insert(at, ("X", t, -1))
    return _gate(q.size, ops, perm)


# ---------------------------------------------------------------------------
# the pairs
# ---------------------------------------------------------------------------
FACTORS15 = [1, 8] * 7 + [1]                  # n = 15: 15 factors (the most 64 qubits allow), 3 column words
WORDS3 = [8, 8, 8, 1, 8, 8, 8, 1, 8]          # n = 15: 9 factors in words 0, 1, 2
Q_WIDE_N = 11                                 # Q program of 25 + 16 column bits: two words


def pair(n, i):
    """Pair i of n: (not-Q gate, Q gate, kind of the Q circuit: "ghz" = the
    shipped circuit under a random permutation, "extended" otherwise)."""
    rng = np.random.default_rng([0x57AB, n, i])
    perm = rng.permutation(n) + 1
    notq = random_notq(n, rng)
    if n == 15 and i == 1:
        notq = notq_from_widths(n, rng, FACTORS15)
    if n == 15 and i == 2:
        notq = notq_from_widths(n, rng, WORDS3)
    if n == Q_WIDE_N and i == 1:
        return notq, extended_q(n, rng, perm, pre_h=[7, 7, 7, 0], extras=[(8, True), (8, True)]), "extended"
    if i % 2 == 0:
        return notq, shipped_q(n, perm), "ghz"
    return notq, extended_q(n, rng, perm), "extended"


SAMPLED = {"q_wide": (Q_WIDE_N, 1), "factors15": (15, 1), "words3": (15, 2), "n15": (15, 3)}


def chained_h(n, m, rng):
    """H on m qubits spread over the groups, joined by a CX chain: one register
    of support 2^m."""
    big = (n + 1) * n_qubits(n)
    qs = [int(x) for x in rng.permutation(big)[:m]]
    return _gate(big, [("H", qb, -1) for qb in qs] + [("X", qs[i + 1], qs[i]) for i in range(m - 1)])
