"""Python restatements of the samplers' rank draws, shared by
tests/test_closed_form.py, tests/test_sampler_rare.py, the GPU tests of the rare
branches and tests/golden/gen_sampler_rare.py.  TEST INFRASTRUCTURE ONLY.

Written from the header comment of csrc/qba_lists_sample.h, the schedule in
csrc/qba_internal.h and DESIGN.md section 4, not from the C twin; only Philox
itself is the twin's (oracle_lib.philox, pinned by the Random123 known-answer
vectors in tests/test_oracle_golden.py).

Each `*_classify` names the branch a Q-correlated entry takes:

  closed form   "w1"          the rank word is w1
                "w0"          w1 rejected, w0 & ~31 accepted (27-bit test)
                "retry1"      both rejected, word 0 of retry block 1 accepted
                "retry_late"  both rejected, a later retry word accepted
  64-bit        "first"       F = x2 | x3 << 32 accepted
                "retry64"     rejected: F of retry blocks 1, 2, ...

and returns what the rare-branch fixture records: the accepted rank word,
where it was found, the entry's n + 1 values and `naive`, the values the entry
would get had the first candidate been taken without its test.
"""
import math

import numpy as np

import oracle_lib

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def fy_decode(n, R):
    """Forward Fisher-Yates: digit of position i has radix n-i+1, first most significant."""
    perm = list(range(16))
    div = math.factorial(n)
    for i in range(1, n):
        div //= n - i + 1
        d, R = divmod(R, div)
        perm[i], perm[i + d] = perm[i + d], perm[i]
    return perm[: n + 1]


def _block(c0, c1, c2, c3, seed):
    return [int(v) for v in oracle_lib.philox(np.array([c0 & M32, c1 & M32, c2, c3], np.uint32), seed)[0]]


def closed_classify(n, seed, e):
    """(kind, word, where, values, naive) of entry e of the closed-form schedule;
    kind "notq" (word, where and naive None) for a not-Q-correlated entry.
    where = 4 * (a - 1) + i for word i of retry block a, 0 otherwise."""
    nq = oracle_lib.n_qubits(n)
    W = 1 << nq
    p, h = e >> 1, e & 1
    x = _block(p, p >> 32, 0, 0, seed)
    w0, w1 = x[2 * h], x[2 * h + 1]
    if not w0 & 1:
        # group g >= 1: nibble g of the word pair (w1 low nibbles, w1 high
        # nibbles, w0 high nibbles, byte order); group 0 = group 1
        vals = [(w1 >> s) & (W - 1) for s in (8, 16, 24, 4, 12, 20, 28)] + \
               [(w0 >> s) & (W - 1) for s in (4, 12, 20, 28)]
        return "notq", None, None, [vals[0]] + vals[: n], None
    nf = math.factorial(n)
    t32, t27 = (1 << 32) % nf, ((1 << 27) % nf) << 5
    ok = lambda F, t: (F * nf) & M32 >= t  # noqa: E731
    where = 0
    if ok(w1, t32):
        kind, F = "w1", w1
    elif ok(w0 & ~31 & M32, t27):
        kind, F = "w0", w0 & ~31 & M32
    else:
        a, F = 0, None
        while F is None:
            a += 1
            ys = _block(p, p >> 32, 0x80000000 + a, h, seed)
            i = next((i for i, y in enumerate(ys) if ok(y, t32)), None)
            if i is not None:
                F, where = ys[i], 4 * (a - 1) + i
        kind = "retry1" if where == 0 else "retry_late"
    r = (w0 >> 1) & (W - 1)
    values = [r ^ q for q in fy_decode(n, (F * nf) >> 32)]
    naive = [r ^ q for q in fy_decode(n, (w1 * nf) >> 32)]
    return kind, F, where, values, naive


def closed_entry_py(n, seed, e):
    """Python restatement of the closed-form schedule for one entry."""
    return closed_classify(n, seed, e)[3]


def perm64_digits(n, F):
    """The 64-bit permutation draw: for i = n .. 2 the digit floor(F * i / 2^64)
    swaps positions i and 1 + digit, F keeps the fraction F * i mod 2^64.
    Returns (pi as a list with pi[0] = 0, the final fraction)."""
    perm = list(range(n + 1))
    for i in range(n, 1, -1):
        d, F = (F * i) >> 64, (F * i) & M64
        perm[i], perm[1 + d] = perm[1 + d], perm[i]
    return perm, F


def perm64_classify(n, seed, e, q):
    """(kind, word, where, values, naive) of entry e under the table samplers'
    schedule with Q program `q` (uniform factors; the shipped one is the GHZ
    table: one factor, pattern r in every field); kind "notq" (everything else
    None: a not-Q entry is its program's, which is not restated here).  word is
    the accepted 64-bit F, where the number of retry blocks."""
    nq = oracle_lib.n_qubits(n)
    x = _block(e, e >> 32, 0, 0, seed)
    if not x[0] & 1:
        return "notq", None, None, None, None
    t = (1 << 64) % math.factorial(n)
    first = x[2] | x[3] << 32
    F, a = first, 0
    while perm64_digits(n, F)[1] < t:  # the final fraction is F * n! mod 2^64
        a += 1
        y = _block(e, e >> 32, 0x80000000 + a, 0, seed)
        F = y[0] | y[1] << 32
    # the Q program's table words: x1, then the words of blocks 1, 2, ...
    words = {}

    def word(k):
        if k not in words:
            words[k] = x[1] if k == 0 else _block(e, e >> 32, 1 + (k - 1) // 4, 0, seed)[(k - 1) % 4]
        return words[k]

    out = 0
    for bits, uniform, off, cw, cs, _ in np.asarray(q["desc"]).tolist():
        assert uniform == 1
        out ^= int(q["pat"][off + ((word(cw) >> cs) & ((1 << bits) - 1))])
    N = (n + 1) * nq
    field = lambda g: (out >> (N - (g + 1) * nq)) & ((1 << nq) - 1)  # noqa: E731
    values = [field(g) ^ pg for g, pg in enumerate(perm64_digits(n, F)[0])]
    naive = [field(g) ^ pg for g, pg in enumerate(perm64_digits(n, first)[0])]
    return ("retry64" if a else "first"), F, a, values, naive


NO_PROGRAM = {"nfac": 0, "desc": np.zeros((0, 6), np.int32), "pat": np.zeros(1, np.uint64),
              "apat": np.zeros(1, np.uint64), "thr": np.zeros(1, np.uint64)}
