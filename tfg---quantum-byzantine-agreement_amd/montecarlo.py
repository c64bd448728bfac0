"""Monte-Carlo runs of the count-mode protocol: many independent instances,
their rounds and decisions computed on the device.

The reference answers "how often does agreement succeed at this sizeL with
this many traitors?" by running tfg.py again and again (its ``Success:``
line, tfg.py:362-363).  Here the lists of a batch of instances are sampled and
counted by ``Engine.sample_check_batched`` and their protocol rounds decided
by ``Engine.protocol_batched`` (qba_protocol_batched, csrc/qba_proto.hip); only
the small result rows come to the host.

Both sides draw from one counter-based stream (:class:`ProtocolRng`; layout in
csrc/qba_internal.h), so :func:`run_host` -- the existing CountParty under
``protocol.run_local`` on that stream -- is the kernel's specification: the
two agree in every field of every instance.

Result row of one instance (int32, ``out_words(n)`` = 4 + 5*(n+1) words):
``{success, dishonest-rank bitmask, empty-V_i rank bitmask, status}`` then per
rank r = 0..n ``{decision (-1 on an empty V_i), V_r bitmask, accept, reject,
sent}`` (rank 0: zeros; the commander keeps no V).  status bit 0 = mailbox
overflow (device only), bit 1 = an RNG retry cap was hit, bit 2 = a list value
>= w at a Q-correlated position (``Engine.montecarlo_lists`` only); with a
nonzero status every other field is 0.

The fused path (``run(path="fused")``, ``Engine.montecarlo_sampled`` /
``montecarlo_lists``) goes from lists to rows in one kernel.  It rests on the
fact that the rounds consult only bitwise reductions over an instance's
Q-correlated entries, restated on the host by :func:`masks_from_lists` and
:func:`masks_from_tables`.

A whole sizeL curve (:func:`curve`, ``Engine.montecarlo_curve_sampled`` /
``montecarlo_curve_lists``) decides the same instances at several sizeL in one
pass: the lists at sizeL = c are the first c columns of the lists at any larger
sizeL, and those reductions are monotone.  :func:`curve_host` is its
specification.

Qubit-flip noise (``flip_q16=k`` on the calls below; DESIGN.md sections 13.5
and 13.6): every measured bit of an entry flips independently with probability
k / 65536 before anything looks at the entry.  :func:`noise_masks` is the
definition; the fused kernels draw the same flips inside
(``Engine.montecarlo_sampled(..., flip_q16=k)``), so does the batched sampler
(``Engine.sample_check_batched(..., flip_q16=k)``, ``run(path="tables_noisy")``:
the noisy lists and their count tables stay on the device for the caller), and
``Engine.noise_apply`` XORs them into device lists.

Adversary policies (``adversary=word`` on the calls below; DESIGN.md section
13.7): what a dishonest lieutenant does to a packet per destination and how a
dishonest commander splits the lieutenants, as a 32-bit word built by
:func:`adversary` (presets in :data:`ADVERSARIES`).  :class:`AdversaryParty`
is the definition; ``0xF`` is the reference's rule, and ``None`` (the default
everywhere) calls exactly what was called before policies existed.

A sweep (:func:`sweep`, ``Engine.montecarlo_sweep_sampled`` /
``montecarlo_sweep_lists``) decides the instances of a
curve under a whole grid of scenarios ``(n_dishonest, word)`` in the same one
pass: the lists do not depend on either.  :func:`sweep_host` is its
specification.

Colluding traitors (``coalition=word`` on :func:`run`, :func:`curve` and their
host forms): a second word, built by
:func:`coalition` (presets in :data:`COALITIONS`), under which the dishonest
lieutenants withhold accepted packets from the honest ones and inject them in a
late round, padded with each other's tuples.  :class:`CoalitionParty` is the
definition; ``None`` and ``0`` are "no coalition".

Lossy links (``net=word`` on :func:`run`, :func:`curve` and their host forms;
DESIGN.md section 13.11): a word built by :func:`net` under which a packet in
flight is lost with probability ``drop_q16 / 65536``, decided per packet by
the pure function :func:`net_lost`.  :class:`NetParty` is the definition;
``None`` and ``0`` are the perfect network.

A grid (:func:`grid`, ``Engine.montecarlo_grid_sampled`` /
``montecarlo_grid_lists``) is the sweep with a
network word in every scenario, ``(n_dishonest, word, net)``: one pass, and
along ``drop_q16`` the loss decisions are nested.  :func:`grid_host` is its
specification.

Noise profiles (``noise=(rates, depol_q16)`` on :func:`run`, :func:`curve` and
their host forms): a flip rate per list row and a
probability that a whole entry is depolarised, in place of the one
``flip_q16``; built by :func:`noise_profile` or :func:`parse_noise_profile`.
:func:`noise_masks_profile` is the definition; ``None`` is "no profile".
"""
from __future__ import annotations

import copy
from typing import Callable, Dict, Optional

import numpy as np

from . import protocol
from ._lib import QbaError
from .countmode import CountParty

MASK64 = (1 << 64) - 1
CTR_TAG = 0x51424150  # word 3 of every protocol counter; the sampler's is 0 or 1
NOISE_TAG = 0x4E4F4953  # word 3 of every noise counter
RNG_CAP = 64          # words one randint may draw
ST_MAILBOX, ST_RNG, ST_RANGE = 1, 2, 4

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32(ctr, key: int):
    """Philox4x32-10 (Salmon et al., SC'11): the 4 output words of counter
    ``ctr`` under the 64-bit ``key`` taken as (lo, hi)."""
    c0, c1, c2, c3 = (int(x) & _U32 for x in ctr)
    k0, k1 = key & _U32, (key >> 32) & _U32
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _U32, (p0 >> 32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0, c1, c2, c3


def _philox4x32_entries(e: np.ndarray, c2: int, c3: int, key: int):
    """:func:`philox4x32` of the counters ``(e_lo, e_hi, c2, c3)`` for a uint64
    array ``e`` at once: four uint64 arrays of 32-bit words."""
    u32 = np.uint64(_U32)
    c0, c1 = e & u32, e >> np.uint64(32)
    c2, c3 = np.full_like(e, c2), np.full_like(e, c3)
    k0, k1 = key & _U32, (key >> 32) & _U32
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & u32, \
            (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & u32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0, c1, c2, c3


def out_words(n: int) -> int:
    return 4 + 5 * (n + 1)


class ProtocolRng:
    """The stream of rank ``rank`` of the instance keyed ``key``: word t is
    output word t % 4 of Philox4x32-10 with counter {t / 4, rank, 0, CTR_TAG}.
    Offers exactly what Party calls: ``randint`` and ``choice``."""

    def __init__(self, key: int, rank: int):
        self.key, self.rank = int(key) & MASK64, int(rank)
        self.t = 0
        self.capped = False
        self._blk, self._words = -1, None

    def word(self) -> int:
        blk = self.t >> 2
        if blk != self._blk:
            self._words = philox4x32((blk, self.rank, 0, CTR_TAG), self.key)
            self._blk = blk
        x = self._words[self.t & 3]
        self.t += 1
        return x

    def randint(self, k: int) -> int:
        """Uniform in [0, k), 1 <= k <= 2^16, by Lemire's method: m = x * k,
        accept m >> 32 when (uint32)m >= 2^32 mod k.  After RNG_CAP rejected
        words ``capped`` is set and the last candidate returned."""
        k = int(k)
        if not 1 <= k <= 1 << 16:
            raise ValueError("randint(k) needs 1 <= k <= 2^16")
        thr = (1 << 32) % k
        r = 0
        for _ in range(RNG_CAP):
            m = self.word() * k
            r = m >> 32
            if (m & _U32) >= thr:
                return r
        self.capped = True
        return r

    def choice(self, a, m: int, replace: bool = False) -> np.ndarray:
        """``m`` distinct elements of ``a``: partial Fisher-Yates, a[j] swapped
        with a[j + randint(len(a) - j)] for j < m; the result is a[:m]."""
        if replace:
            raise ValueError("only choice(..., replace=False) is defined")
        a = np.array(a, copy=True)
        if not 0 <= m <= len(a):
            raise ValueError("cannot take more elements than there are")
        for j in range(m):
            s = j + self.randint(len(a) - j)
            a[j], a[s] = a[s], a[j]
        return a[:m]


def _recording(cls, sink: Dict[int, protocol.Party]):
    class Recorded(cls):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            sink[self.rank] = self
    return Recorded


def _mask(values) -> int:
    m = 0
    for v in values:
        m |= 1 << int(v)
    return m


def _check_flip(flip_q16: int) -> int:
    k = int(flip_q16)
    if not 0 <= k <= 65535:
        raise ValueError("flip_q16 must be in [0, 65535]")
    return k


def noise_masks(n: int, key: int, count: int, flip_q16: int) -> np.ndarray:
    """The flips of the entries [0, count) of the instance keyed ``key`` at flip
    probability k / 65536, k = ``flip_q16``: uint8 [n+1, count], the value XORed
    into group g of entry e.  With word(t) = output word t % 4 of
    ``philox4x32((e_lo, e_hi, t / 4, NOISE_TAG), key)`` and j0 the lowest set
    bit of k, 64 bits r start at 0 and take, for s = 0 .. 15 - j0,
    ``x = word(2s) | word(2s+1) << 32; r = r | x if bit j0 + s of k else r & x``
    (one step maps a bit's probability q to (bit + q) / 2, so every bit of r is
    1 with probability exactly k / 65536); the mask of group g is
    ``(r >> 4g) & (w - 1)``.  k = 0 draws nothing."""
    k = _check_flip(flip_q16)
    g, w = n + 1, 1 << _nq(n)
    out = np.zeros((g, int(count)), np.uint8)
    if k == 0:
        return out
    j0 = (k & -k).bit_length() - 1
    e = np.arange(int(count), dtype=np.uint64)
    r = np.zeros(int(count), np.uint64)
    blk = None
    for s in range(16 - j0):
        if s % 2 == 0:
            blk = _philox4x32_entries(e, s // 2, NOISE_TAG, int(key) & MASK64)
        x = blk[2 * (s % 2)] | blk[2 * (s % 2) + 1] << np.uint64(32)
        r = r | x if (k >> (j0 + s)) & 1 else r & x
    for i in range(g):
        out[i] = (r >> np.uint64(4 * i)) & np.uint64(w - 1)
    return out


def noisy_lists(n: int, key: int, lists, flip_q16: int) -> np.ndarray:
    """``lists`` [n+1, count] with :func:`noise_masks` XORed in (a new uint8 array)."""
    L = np.array(lists, dtype=np.uint8).reshape(n + 1, -1)
    return L ^ noise_masks(n, key, L.shape[1], flip_q16)


# ---------------------------------------------------------------------------
# Noise profiles
# ---------------------------------------------------------------------------
DEPOL_CTR = 8  # word 2 of the depolarisation counter; the ladder's are 0..7


def _q16(value, what: str) -> int:
    """``value`` as an int in [0, 65535]; QbaError naming ``what`` otherwise
    (bools and non-integers included)."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise QbaError(f"noise profile: {what} must be an integer, not {value!r}")
    if not 0 <= int(value) <= 65535:
        raise QbaError(f"noise profile: {what}={int(value)} outside [0, 65535]")
    return int(value)


def check_noise_profile(n: int, rates, depol_q16=0):
    """``(rates, depol_q16)`` as a tuple of n + 1 ints and an int when they are a
    valid profile of ``n`` parties: one integer rate in [0, 65535] per list row
    (row 0 the commander's list, row 1 Lc, row g >= 2 lieutenant g) and
    ``depol_q16`` in [0, 65535].  QbaError naming the row or ``depol_q16``
    otherwise."""
    try:
        rs = list(rates)
    except TypeError:
        raise QbaError(f"noise profile: rates must be a sequence of {n + 1} integers, not {rates!r}") from None
    if len(rs) != n + 1:
        raise QbaError(f"noise profile: rates has {len(rs)} rows, n={n} needs {n + 1}")
    return tuple(_q16(r, f"row {g}") for g, r in enumerate(rs)), _q16(depol_q16, "depol_q16")


def noise_profile(n: int, all=0, rows=None, depol_q16=0):  # noqa: A002 (the CLI's word)
    """The profile ``(rates, depol_q16)`` of ``n`` parties: every row at rate
    ``all``, then ``rows`` ({row: rate}) over it."""
    rates = [all] * (n + 1)
    for g, k in (rows or {}).items():
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) <= n:
            raise QbaError(f"noise profile: row {g!r} outside [0, {n}]")
        rates[int(g)] = k
    return check_noise_profile(n, rates, depol_q16)


def parse_noise_profile(n: int, text):
    """``all:K,G:K,...,depol:K`` (K decimal or ``0x`` hex, G a row index; any
    order, every item optional, a row overrides ``all``) as a checked profile.
    An unknown key, a row > n or a repeated key is a QbaError naming it."""
    if not isinstance(text, str):
        return check_noise_profile(n, *text)
    seen, rows, every, depol = set(), {}, 0, 0
    for item in filter(None, (t.strip() for t in text.split(","))):
        key, sep, val = item.partition(":")
        key = key.strip()
        if not sep:
            raise QbaError(f"noise profile {text!r}: item {item!r} is not KEY:K")
        try:
            k = int(val, 0)
        except ValueError:
            raise QbaError(f"noise profile {text!r}: {key}: K is a number (0x... or decimal), not {val!r}") from None
        if key in ("all", "depol"):
            name = key
        else:
            try:
                name = int(key, 10)
            except ValueError:
                raise QbaError(f"noise profile {text!r}: unknown key {key!r} (all, depol or a row index)") from None
            if not 0 <= name <= n:
                raise QbaError(f"noise profile {text!r}: row {name} outside [0, {n}]")
        if name in seen:
            raise QbaError(f"noise profile {text!r}: {'row ' if isinstance(name, int) else ''}{name} given twice")
        seen.add(name)
        if name == "all":
            every = k
        elif name == "depol":
            depol = k
        else:
            rows[name] = k
    return noise_profile(n, every, rows, depol)


def format_noise_profile(profile) -> str:
    """A profile in the normal form of :func:`parse_noise_profile`: ``all:K``
    (the most common rate, the smaller one on a tie), the rows that differ in
    ascending order, then ``depol:K``; every K in hex."""
    rates, depol = profile
    every = max(sorted(set(rates)), key=list(rates).count)
    items = [f"all:{every:#x}"] + [f"{g}:{k:#x}" for g, k in enumerate(rates) if k != every]
    return ",".join(items + [f"depol:{depol:#x}"])


def noise_masks_profile(n: int, key: int, count: int, rates, depol_q16=0) -> np.ndarray:
    """:func:`noise_masks` under a profile: uint8 [n+1, count], the value XORed
    into group g of entry e.  With word(t) as there and j0 the lowest set bit
    of any rate, 64 bits r start at 0 and take, for s = 0 .. 15 - j0,
    ``x = word(2s) | word(2s+1) << 32; r = ((r | x) & M_s) | ((r & x) & ~M_s)``
    where nibble g of M_s is 0xF when bit j0 + s of ``rates[g]`` is set: nibble
    g goes through the ladder of its own rate (ANDs into 0 below its lowest
    bit), so each of its bits is 1 with probability exactly ``rates[g] /
    65536``, and with equal rates r is :func:`noise_masks`'s.  Then, when
    ``depol_q16`` is not 0, ``d = philox4x32((e_lo, e_hi, DEPOL_CTR,
    NOISE_TAG), key)`` and the entries with ``(d[0] & 0xFFFF) < depol_q16`` are
    depolarised: ``r ^= d[2] | d[3] << 32``, a uniform value below w into every
    group at once.  The mask of group g is ``(r >> 4g) & (w - 1)``.  The
    all-zero profile draws nothing."""
    rates, depol = check_noise_profile(n, rates, depol_q16)
    g, w = n + 1, 1 << _nq(n)
    count = int(count)
    out = np.zeros((g, count), np.uint8)
    anyr = 0
    for k in rates:
        anyr |= k
    if not (anyr or depol):
        return out
    e = np.arange(count, dtype=np.uint64)
    r = np.zeros(count, np.uint64)
    key = int(key) & MASK64
    if anyr:
        j0 = (anyr & -anyr).bit_length() - 1
        blk = None
        for s in range(16 - j0):
            if s % 2 == 0:
                blk = _philox4x32_entries(e, s // 2, NOISE_TAG, key)
            x = blk[2 * (s % 2)] | blk[2 * (s % 2) + 1] << np.uint64(32)
            m = np.uint64(sum(0xF << (4 * i) for i, k in enumerate(rates) if (k >> (j0 + s)) & 1))
            r = ((r | x) & m) | ((r & x) & ~m)
    if depol:
        d = _philox4x32_entries(e, DEPOL_CTR, NOISE_TAG, key)
        hit = (d[0] & np.uint64(0xFFFF)) < np.uint64(depol)
        r = np.where(hit, r ^ (d[2] | d[3] << np.uint64(32)), r)
    for i in range(g):
        out[i] = (r >> np.uint64(4 * i)) & np.uint64(w - 1)
    return out


def noisy_lists_profile(n: int, key: int, lists, rates, depol_q16=0) -> np.ndarray:
    """``lists`` [n+1, count] with :func:`noise_masks_profile` XORed in (a new uint8 array)."""
    L = np.array(lists, dtype=np.uint8).reshape(n + 1, -1)
    return L ^ noise_masks_profile(n, key, L.shape[1], rates, depol_q16)


def _no_profile(noise, what: str) -> None:
    """ValueError when ``noise`` is a profile (not None): ``what`` is not built for one."""
    if noise is not None:
        raise ValueError(f"{what} is not built for a noise profile (noise=)")


def _profile_alone(flip: int, coal: int, lossy: int, explain: int = 0) -> None:
    """ValueError naming what a noise profile was combined with: a profile
    replaces ``flip_q16``, and the coalition, lossy-network and trace kernels
    take none."""
    if flip:
        raise ValueError(f"flip_q16={flip} with a noise profile (noise=): the profile holds the rates")
    if coal:
        _no_profile(True, f"a coalition (coalition={coal:#x})")
    if lossy:
        _no_profile(True, f"a lossy network (net={lossy:#x})")
    if explain:
        _no_profile(True, "explain (the trace kernels)")


# ---------------------------------------------------------------------------
# Adversary policies
# ---------------------------------------------------------------------------
ACT_MUTE, ACT_REORDER, ACT_CLEAR_P, ACT_CLEAR_L, ACT_RELAY = range(5)
ORDER_REFERENCE, ORDER_LOW, ORDER_W = range(3)
ADV_REFERENCE = 0xF
_ADV_VALID = 0x0001131F


def check_adversary(word) -> int:
    """``word`` as an int when it is a valid policy word; QbaError otherwise
    (a reserved bit, no allowed action, or order 3)."""
    try:
        a = int(word)
    except (TypeError, ValueError):
        raise QbaError(f"adversary must be an integer policy word, not {word!r}") from None
    if a < 0 or a & ~_ADV_VALID:
        raise QbaError(f"adversary word {a:#x} sets a reserved bit")
    if not a & 0x1F:
        raise QbaError(f"adversary word {a:#x} allows no action (acts == 0)")
    if (a >> 8) & 3 > 2:
        raise QbaError(f"adversary word {a:#x}: the order field must be <= 2")
    return a


def adversary(acts=(ACT_MUTE, ACT_REORDER, ACT_CLEAR_P, ACT_CLEAR_L), order: int = ORDER_REFERENCE,
              fresh: bool = False, comm: bool = False) -> int:
    """The policy word of a dishonest party.

    ``acts``   the actions a dishonest lieutenant draws from, uniformly, per
               destination (a set of 0..4, or their bit mask): 0 maybe do not
               send, 1 replace the order, 2 clear P, 3 clear L (the reference's
               four), 4 relay unchanged.
    ``order``  what action 1 writes: 0 ``randint(n + 1)`` (the reference), 1 the
               smallest order in [0, w) other than the packet's current v
               (0, or 1 when v is 0; no draw), 2 ``randint(w)``.
    ``fresh``  False: a mutation stays for the later destinations of the same
               broadcast (the reference).  True: every destination starts from
               the packet as it was handed to the broadcast.
    ``comm``   the dishonest commander's split: False ``dest <= (n + 1) / 2``
               gets v1 (the reference), True even ``dest`` gets v1.

    The defaults give ``0xF``, the reference's traitor."""
    if isinstance(acts, int):
        mask = acts
    else:
        mask = 0
        for a in acts:
            if not 0 <= int(a) <= 4:
                raise QbaError(f"action {a!r} outside 0..4")
            mask |= 1 << int(a)
    if not 0 <= mask < 32:
        raise QbaError(f"acts {mask:#x} outside the five action bits")
    if order not in (0, 1, 2):
        raise QbaError("order is 0 (randint(n + 1)), 1 (low) or 2 (randint(w))")
    return check_adversary(mask | int(order) << 8 | (1 << 12 if fresh else 0) | (1 << 16 if comm else 0))


ADVERSARIES = {
    "reference": ADV_REFERENCE,
    "relay": adversary([ACT_RELAY]),
    "reorder_low": adversary([ACT_REORDER], order=ORDER_LOW, fresh=True, comm=True),
    "mute": adversary([ACT_MUTE]),
    "strip": adversary([ACT_CLEAR_P, ACT_CLEAR_L], fresh=True),
}


def parse_adversary(text) -> int:
    """A preset name of :data:`ADVERSARIES` or a number (``0x...`` or decimal)
    as a checked policy word."""
    if isinstance(text, str):
        if text in ADVERSARIES:
            return ADVERSARIES[text]
        try:
            text = int(text, 0)
        except ValueError:
            raise QbaError(f"adversary {text!r} is neither a number nor one of {sorted(ADVERSARIES)}") from None
    return check_adversary(text)


class AdversaryParty(CountParty):
    """CountParty whose dishonest behaviour is read from the policy word
    ``adv`` (a class attribute: :func:`adversary_party` makes the subclass of a
    word).  The specification of the ``_adv`` kernels.

    Per destination a dishonest lieutenant draws ``a = randint(popcount(acts))``
    -- always, also when one action is allowed -- and takes the a-th set bit of
    ``acts`` in ascending order as its action; action 0 then draws
    ``randint(2)``, action 1 what ``order`` says, the others nothing.  With
    ``0xF`` this is Party.lieu_broadcast / comm_broadcast draw for draw."""

    adv = ADV_REFERENCE

    def comm_broadcast(self):
        if self.rank != 1 or not self.dishonest or not (self.adv >> 16) & 1:
            return super().comm_broadcast()
        v1 = self.rng.randint(self.w)
        v2 = self.rng.randint(self.w)
        while v2 == v1:
            v2 = self.rng.randint(self.w)
        for dest in range(2, self.n + 1):
            v = v1 if dest % 2 == 0 else v2
            self.send(dest, self.p_for(v), v, set())

    def lieu_broadcast(self, P, v, L):
        acts = [a for a in range(5) if (self.adv >> a) & 1]
        order, fresh = (self.adv >> 8) & 3, (self.adv >> 12) & 1
        P0, v0, L0 = P, v, L
        for dest in range(2, self.n + 1):
            if dest == self.rank:
                continue
            go = 1
            if self.dishonest:
                if fresh:  # P.clear() and L.clear() mutate in place: a copy per destination
                    P, v, L = copy.copy(P0), v0, set(L0)
                action = acts[self.rng.randint(len(acts))]
                if action == ACT_MUTE:
                    go = self.rng.randint(2)
                elif action == ACT_REORDER:
                    if order == ORDER_LOW:
                        v = 1 if int(v) == 0 else 0
                    else:
                        v = self.rng.randint(self.n + 1 if order == ORDER_REFERENCE else self.w)
                elif action == ACT_CLEAR_P:
                    P.clear()
                elif action == ACT_CLEAR_L:
                    L.clear()
            if go:
                self.send(dest, P, v, L)


def adversary_party(word: int, base=None):
    """The :class:`AdversaryParty` subclass of the policy ``word``, for the
    ``party_cls`` seam of :func:`run_host`; ``base`` (a CountParty subclass, for
    instance an observing one) is mixed in behind it."""
    word = check_adversary(word)
    bases = (AdversaryParty,) if base in (None, CountParty, AdversaryParty) else (AdversaryParty, base)
    return type(f"AdversaryParty_{word:x}", bases, {"adv": word})


# ---------------------------------------------------------------------------
# Colluding traitors
# ---------------------------------------------------------------------------
WHEN_LAST, WHEN_RELAYED = 0, 1
TARGETS_ALL, TARGETS_EVEN, TARGETS_LOWEST = 0, 1, 2
_COAL_VALID = 0x1331


def check_coalition(word) -> int:
    """``word`` as an int when it is a valid coalition word (0: no coalition);
    QbaError otherwise (a reserved bit, when > 1, targets > 2, or a field set
    without ``on``)."""
    try:
        c = int(word)
    except (TypeError, ValueError):
        raise QbaError(f"coalition must be an integer word, not {word!r}") from None
    if c < 0 or c & ~_COAL_VALID:
        raise QbaError(f"coalition word {c:#x} sets a reserved bit")
    if (c >> 4) & 3 > 1:
        raise QbaError(f"coalition word {c:#x}: the when field must be <= 1")
    if (c >> 8) & 3 > 2:
        raise QbaError(f"coalition word {c:#x}: the targets field must be <= 2")
    if not c & 1:
        for name, field in (("when", (c >> 4) & 3), ("targets", (c >> 8) & 3), ("starve", (c >> 12) & 1)):
            if field:
                raise QbaError(f"coalition word {c:#x} sets the {name} field without on")
    return c


def coalition(when: int = WHEN_LAST, targets: int = TARGETS_ALL, starve: bool = False) -> int:
    """The word of a coalition of all dishonest parties (bit 0, ``on``, set).

    ``when``     the round R in which the receivers process the held packets:
                 0 ``n_dishonest + 1`` (the last round: an acceptance there is
                 never relayed), 1 ``max(1, n_dishonest)`` (the last round whose
                 acceptances are still relayed).
    ``targets``  the honest lieutenants that packets are withheld from and
                 injected to: 0 all, 1 those of even rank, 2 the lowest-ranked.
    ``starve``   a dishonest commander sends v1 to every honest lieutenant and
                 v2 to every dishonest one."""
    if when not in (0, 1):
        raise QbaError("when is 0 (the last round) or 1 (the last relayed round)")
    if targets not in (0, 1, 2):
        raise QbaError("targets is 0 (all honest lieutenants), 1 (even ranks) or 2 (the lowest-ranked)")
    return check_coalition(1 | int(when) << 4 | int(targets) << 8 | (1 << 12 if starve else 0))


COALITIONS = {
    "late": coalition(),
    "late_relayed": coalition(when=WHEN_RELAYED),
    "late_one": coalition(targets=TARGETS_LOWEST),
    "starve_late": coalition(targets=TARGETS_EVEN, starve=True),
}


def parse_coalition(text) -> int:
    """A preset name of :data:`COALITIONS` or a number (``0x...`` or decimal)
    as a checked coalition word."""
    if isinstance(text, str):
        if text in COALITIONS:
            return COALITIONS[text]
        try:
            text = int(text, 0)
        except ValueError:
            raise QbaError(f"coalition {text!r} is neither a number nor one of {sorted(COALITIONS)}") from None
    return check_coalition(text)


class CoalitionRun:
    """What the traitors of one run share: ``parties`` {rank: party}, filled as
    the parties are made.  The dishonest set is rank 0's draw; a lieutenant
    reads it only after the tables of rank 0 have reached it, which rank 0
    sends after the draw.  The traitors' descriptors under a P_u come from the
    count tables, which every rank holds."""

    def __init__(self):
        self.parties: Dict[int, protocol.Party] = {}

    def dishonest(self) -> frozenset:
        return frozenset(int(r) for r in self.parties[0].dishonest_ids)


class CoalitionParty(AdversaryParty):
    """AdversaryParty whose dishonest parties collude as the coalition word
    ``coal`` says (class attributes: :func:`coalition_party` makes the subclass
    of a pair of words; ``run_shared`` is the :class:`CoalitionRun` that
    :func:`run_host` hands over per instance, and without one -- the class
    used outside :func:`run_host` -- nobody colludes).  The specification of
    the ``_coal`` kernels; with ``coal == 0`` it is AdversaryParty.

    A dishonest lieutenant under ``on`` that accepts a packet in round r (0:
    the commander's epoch) serves its destinations in ascending order: a
    dishonest one gets the packet as it was handed over, with no draw; a target
    gets nothing while r < R - 1, and the handed packet goes once to the hold
    list; every other one is served as AdversaryParty serves it (a mutation
    that stays, stays for these destinations only).  In round R - 1, after its
    inbox, it sends the hold list in order to every target in ascending rank,
    each packet with a P and no empty tuple padded to R tuples from the pool:
    the dishonest lieutenants' tuples in ascending rank, then under a
    dishonest commander its tuple (row 0) and, when v != u, its extra list's
    (row 1, Lc: equal to u on all of P_u, so Cond2 lets it pass under another
    v only)."""

    coal = 0
    run_shared: Optional[CoalitionRun] = None

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._acc_rnd = 0      # the round of the packet being processed (0: the commander's epoch)
        self._seen_rounds = 0  # rounds whose inbox has been drained
        self._left = 0         # packets of the current round not yet processed
        self.hold = []
        if self.run_shared is not None:
            self.run_shared.parties[self.rank] = self

    # -- the word ------------------------------------------------------------
    @property
    def colluding(self) -> bool:
        return bool(self.coal & 1) and self.dishonest and self.run_shared is not None

    def delivery_round(self) -> int:
        return self.n_dis + 1 if (self.coal >> 4) & 3 == 0 else max(1, self.n_dis)

    def targets(self) -> list:
        if self.run_shared is None:
            return []
        dis = self.run_shared.dishonest()
        honest = [r for r in range(2, self.n + 1) if r not in dis]
        sel = (self.coal >> 8) & 3
        return honest if sel == 0 else [r for r in honest if r % 2 == 0] if sel == 1 else honest[:1]

    # -- the commander -------------------------------------------------------
    def comm_broadcast(self):
        if self.rank != 1 or not self.colluding or not (self.coal >> 12) & 1:
            return super().comm_broadcast()
        dis = self.run_shared.dishonest()
        v1 = self.rng.randint(self.w)
        v2 = self.rng.randint(self.w)
        while v2 == v1:
            v2 = self.rng.randint(self.w)
        for dest in range(2, self.n + 1):
            v = v2 if dest in dis else v1
            self.send(dest, self.p_for(v), v, set())

    # -- a lieutenant --------------------------------------------------------
    def lieu_receive(self, P, v, L, rnd, pre=None):
        self._acc_rnd = rnd
        super().lieu_receive(P, v, L, rnd, pre)
        self._left -= 1
        if self._left == 0 and self.colluding and rnd == self.delivery_round() - 1:
            self.deliver()

    def precheck(self, inbox):
        """Called once per round with the drained inbox: the point from which
        the end of the round's inbox walk is counted."""
        self._seen_rounds += 1
        self._left = len(inbox)
        if not inbox and self.colluding and self._seen_rounds == self.delivery_round() - 1:
            self.deliver()
        return super().precheck(inbox)

    def lieu_broadcast(self, P, v, L):
        if not self.colluding:
            return super().lieu_broadcast(P, v, L)
        acts = [a for a in range(5) if (self.adv >> a) & 1]
        order, fresh = (self.adv >> 8) & 3, (self.adv >> 12) & 1
        dis, targets = self.run_shared.dishonest(), self.targets()
        early = self._acc_rnd < self.delivery_round() - 1
        P0, v0, L0 = copy.copy(P), v, set(L)  # the packet as handed over; P and L below are working copies
        P, L = copy.copy(P0), set(L0)
        held = False
        for dest in range(2, self.n + 1):
            if dest == self.rank:
                continue
            if dest in dis:
                self.send(dest, P0, v0, L0)
                continue
            if early and dest in targets:
                if not held:
                    self.hold.append((copy.copy(P0), v0, set(L0)))
                    held = True
                continue
            go = 1
            if fresh:
                P, v, L = copy.copy(P0), v0, set(L0)
            action = acts[self.rng.randint(len(acts))]
            if action == ACT_MUTE:
                go = self.rng.randint(2)
            elif action == ACT_REORDER:
                if order == ORDER_LOW:
                    v = 1 if int(v) == 0 else 0
                else:
                    v = self.rng.randint(self.n + 1 if order == ORDER_REFERENCE else self.w)
            elif action == ACT_CLEAR_P:
                P.clear()
            elif action == ACT_CLEAR_L:
                L.clear()
            if go:
                self.send(dest, P, v, L)

    def pool(self, u: int, v: int) -> list:
        """The coalition's tuples under P_u, in the order they are offered."""
        dis = self.run_shared.dishonest()
        rows = [g for g in range(2, self.n + 1) if g in dis]
        if 1 in dis:  # row 0 is the commander's list, row 1 its extra list Lc: u on all of P_u
            rows.append(0)
            if int(v) != u:
                rows.append(1)
        return [(g, self.tables.desc(g, u)) for g in rows]

    def pad(self, P, v, L) -> None:
        """A held packet with a P and no empty tuple takes pool tuples it does
        not hold yet until it has R of them or the pool is exhausted."""
        if P.u is None or () in L:
            return
        R = self.delivery_round()
        for _, d in self.pool(P.u, v):
            if len(L) >= R:
                break
            L.add(d)  # a tuple that is there already (a duplicated row's, the sender's own) adds nothing

    def deliver(self):
        targets = self.targets()
        for P, v, L in self.hold:
            self.pad(P, v, L)
            for dest in targets:
                self.send(dest, P, v, L)
        self.hold = []


def coalition_party(adv: int, coal: int, base=None):
    """The :class:`CoalitionParty` subclass of a policy word and a coalition
    word, for the ``party_cls`` seam of :func:`run_host` (which sets
    ``run_shared`` per instance); ``base`` as in :func:`adversary_party`."""
    adv, coal = check_adversary(adv), check_coalition(coal)
    if base is not None and issubclass(base, CoalitionParty):  # an observing subclass: the words are set on it
        bases = (base,)
    else:
        bases = (CoalitionParty,) if base in (None, CountParty, AdversaryParty) else (CoalitionParty, base)
    return type(f"CoalitionParty_{adv:x}_{coal:x}", bases, {"adv": adv, "coal": coal})


# ---------------------------------------------------------------------------
# Lossy links
# ---------------------------------------------------------------------------
NET_TAG = 0x4E455457  # word 3 of every loss counter
NET_CMD = 1 << 16
_NET_VALID = 0x0001FFFF


def check_net(word) -> int:
    """``word`` as an int when it is a valid network word (0: the perfect
    network); QbaError otherwise (a reserved bit, or cmd with drop_q16 == 0)."""
    try:
        w = int(word)
    except (TypeError, ValueError):
        raise QbaError(f"net must be an integer network word, not {word!r}") from None
    if w < 0 or w & ~_NET_VALID:
        raise QbaError(f"network word {w:#x} sets a reserved bit")
    if w & NET_CMD and not w & 0xFFFF:
        raise QbaError(f"network word {w:#x} sets the cmd field with drop_q16 == 0")
    return w


def net(drop_q16: int, cmd: bool = False) -> int:
    """The network word: a packet on a lossy link is lost with probability
    ``drop_q16 / 65536``; the lieutenant-to-lieutenant links are lossy, and with
    ``cmd`` the commander's links of epoch 0 too."""
    k = int(drop_q16)
    if not 0 <= k <= 0xFFFF:
        raise QbaError("drop_q16 must be in [0, 65535]")
    return check_net(k | (NET_CMD if cmd else 0))


def parse_net(text) -> int:
    """``K`` or ``K:cmd`` (K decimal or ``0x`` hex) as a checked network word."""
    cmd = False
    if isinstance(text, str):
        head, sep, tail = text.partition(":")
        if sep and tail != "cmd":
            raise QbaError(f"net {text!r}: only ':cmd' may follow drop_q16")
        cmd = bool(sep)
        try:
            text = int(head, 0)
        except ValueError:
            raise QbaError(f"net {text!r}: drop_q16 is a number (0x... or decimal)") from None
    try:
        return net(text, cmd)
    except (TypeError, ValueError):
        raise QbaError(f"net {text!r}: drop_q16 is a number (0x... or decimal)") from None


def net_lost(key: int, epoch: int, src: int, dest: int, seq: int, drop_q16: int) -> bool:
    """Whether the packet ``seq`` that ``src`` hands to the link towards ``dest``
    in epoch ``epoch`` of the instance keyed ``key`` is lost: the low 16 bits of
    word ``seq & 3`` of ``philox4x32((epoch, src | dest << 8, seq >> 2, NET_TAG),
    key)`` are below ``drop_q16``.  A function of the packet alone."""
    x = philox4x32((epoch, src | dest << 8, seq >> 2, NET_TAG), int(key) & MASK64)[seq & 3]
    return (x & 0xFFFF) < int(drop_q16)


class NetLost:
    """What a lieutenant receives in place of a lost commander packet."""


class NetParty(AdversaryParty):
    """AdversaryParty on the network the word ``net`` describes (a class
    attribute: :func:`net_party` makes the subclass of a pair of words).  The
    specification of the ``_net`` kernels; with ``net == 0`` it is
    AdversaryParty.

    Every ``send`` counts, takes the next ``seq`` of its (epoch, dest) and is
    then handed over or, on a lossy link, lost as :func:`net_lost` says of
    ``(self.seed, epoch, rank, dest, seq)`` -- ``self.seed`` is the instance key
    under :func:`run_host`.  The epoch is 0 during comm_broadcast and ``rnd``
    while a packet of round ``rnd`` is processed.  In LocalWorld a lost
    commander packet travels as a marker (v = -1) that the lieutenant's ``recv``
    turns into :class:`NetLost`, so that nobody blocks; the lieutenant then
    skips step 3a.  A lost lieutenant packet is simply not sent."""

    net = 0
    _LOST_V = -1  # the marker's v; an order, also a traitor's, is >= 0

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._epoch = 0
        self._seq: Dict[tuple, int] = {}

    def lossy(self, dest: int) -> bool:
        """Whether this rank's link towards ``dest`` loses packets."""
        return bool(self.net & 0xFFFF) and (self.rank >= 2 or bool(self.net & NET_CMD))

    def send(self, dest, P, v, L):
        e = self._epoch
        seq = self._seq.get((e, dest), 0)
        self._seq[(e, dest)] = seq + 1
        if self.lossy(dest) and net_lost(self.seed, e, self.rank, dest, seq, self.net & 0xFFFF):
            self.stats.sent += 1  # the sender cannot tell
            return self.lose(dest, P, v, L, e, seq)
        super().send(dest, P, v, L)

    def lose(self, dest, P, v, L, epoch, seq):
        """The packet is lost (an observation seam).  Only a commander's loss
        leaves a trace: the marker its receiver is waiting for."""
        if self.rank == 1:
            head = np.array([-1, self._LOST_V, 0], dtype=np.int64)
            self.comm.Isend([head, protocol._dt(self.comm)], dest=dest, tag=1).Wait()
            self.comm.Isend([np.zeros(0, np.int64), protocol._dt(self.comm)], dest=dest, tag=2).Wait()

    def recv(self, src):
        P, v, L = super().recv(src)
        return (NetLost, v, L) if v == self._LOST_V else (P, v, L)

    def comm_broadcast(self):
        self._epoch = 0
        if self.rank <= 1 or not self.net & NET_CMD:
            return super().comm_broadcast()
        self.wire.clear()
        P, v, L = self.recv(1)
        if P is NetLost:
            return
        if self.add_own_and_check(P, v, L):
            self.Vi.add(v)
            self.lieu_broadcast(P, v, L)

    def lieu_receive(self, P, v, L, rnd, pre=None):
        self._epoch = rnd
        super().lieu_receive(P, v, L, rnd, pre)


def net_party(adv: int, net: int, base=None):
    """The :class:`NetParty` subclass of a policy word and a network word, for
    the ``party_cls`` seam of :func:`run_host`; ``base`` as in
    :func:`adversary_party`, or an observing :class:`NetParty` subclass."""
    adv, net = check_adversary(adv), check_net(net)
    if base is not None and issubclass(base, NetParty):
        bases = (base,)
    else:
        bases = (NetParty,) if base in (None, CountParty, AdversaryParty) else (NetParty, base)
    return type(f"NetParty_{adv:x}_{net:x}", bases, {"adv": adv, "net": net})


def _no_net(net, what: str) -> None:
    """ValueError when ``net`` is a non-zero network word: ``what`` is not built for one."""
    if net is not None and check_net(net):
        raise ValueError(f"{what} is not built for a lossy network (net={int(net):#x})")


def run_host(n: int, sizeL: int, n_dishonest: int, n_inst: int, seed_base: int, engine, lists=None,
             party_cls=None, rng_factory: Optional[Callable] = None, flip_q16: int = 0,
             adversary: Optional[int] = None, coalition: Optional[int] = None,
             net: Optional[int] = None, noise=None) -> np.ndarray:
    """The specification of qba_protocol_batched: CountParty under
    ``protocol.run_local`` (LocalWorld's barrier-epoch delivery: a round's inbox
    is everything sent in the previous epoch, in (source, sequence) order,
    drained before any packet is processed) for instance i with list seed
    ``seed_base + i`` and :class:`ProtocolRng` streams of the same key.

    ``engine`` needs only ``count_tables`` (the GPU Engine or the tests' numpy
    engine); ``lists`` injects [n_inst, n+1, sizeL] values instead of sampling.
    ``party_cls`` (a CountParty subclass) and ``rng_factory`` ((key, rank) ->
    rng) are observation seams for tests.  Returns int32 [n_inst, out_words(n)].

    ``flip_q16 > 0``: :func:`noisy_lists` of the lists the instance would have
    used (injected, or else sampled by ``engine.sample(n, key, 0, sizeL)``,
    which the engine must then offer), then the same.

    ``adversary=word``: the dishonest parties follow that policy
    (:func:`adversary_party` of ``party_cls``); ``None`` is the reference's
    rule, and ``0xF`` gives the same rows.

    ``coalition=word``: the dishonest parties collude (:class:`CoalitionParty`
    under ``adversary``, or the reference's rule); ``None`` and ``0`` are no
    coalition and call what is called without the argument; ``party_cls`` may
    then be an observing :class:`CoalitionParty` subclass.

    ``net=word``: packets are lost in flight (:class:`NetParty` under
    ``adversary``, or the reference's rule); ``None`` and ``0`` are the perfect
    network and call what is called without the argument; ``party_cls`` may
    then be an observing :class:`NetParty` subclass.  Not with a coalition.

    ``noise=(rates, depol_q16)``: a noise profile (:func:`noise_profile`) in
    place of ``flip_q16``: :func:`noisy_lists_profile` of the lists the instance
    would have used, then the same.  ``None`` calls what is called without the
    argument.  Not with a non-zero ``flip_q16``, a coalition or a lossy network.
    """
    flip = _check_flip(flip_q16)
    coal = 0 if coalition is None else check_coalition(coalition)
    lossy = 0 if net is None else check_net(net)
    prof = None if noise is None else check_noise_profile(n, *noise)
    if prof is not None:
        _profile_alone(flip, coal, lossy)
    if lossy:
        if coal:
            _no_net(lossy, "a coalition")
        party_cls = net_party(ADV_REFERENCE if adversary is None else adversary, lossy, party_cls)
    elif coal:
        party_cls = coalition_party(ADV_REFERENCE if adversary is None else adversary, coal, party_cls)
    elif adversary is not None:
        party_cls = adversary_party(adversary, party_cls)
    out = np.zeros((n_inst, out_words(n)), np.int32)
    make = rng_factory or ProtocolRng
    for i in range(n_inst):
        key = (int(seed_base) + i) & MASK64
        parties: Dict[int, protocol.Party] = {}
        rngs = []

        def factory(_seed, rank, key=key, rngs=rngs):
            rngs.append(make(key, rank))
            return rngs[-1]

        mine = None if lists is None else lists[i]
        if flip and sizeL > 0:
            clean = engine.sample(n, key, 0, sizeL) if mine is None else np.asarray(mine)[:, :sizeL]
            mine = noisy_lists(n, key, _host_lists(clean, sizeL), flip)
        elif prof is not None and sizeL > 0:
            clean = engine.sample(n, key, 0, sizeL) if mine is None else np.asarray(mine)[:, :sizeL]
            mine = noisy_lists_profile(n, key, _host_lists(clean, sizeL), *prof)
        cls = party_cls or CountParty
        if coal:  # what the traitors of this instance share
            cls = type(cls.__name__, (cls,), {"run_shared": CoalitionRun()})
        run = protocol.run_local(n, sizeL, n_dishonest, engine, lists=mine,
                                 list_seed=key, party_cls=_recording(cls, parties),
                                 rng_factory=factory)
        status = ST_RNG if any(getattr(r, "capped", False) for r in rngs) else 0
        row = out[i]
        row[3] = status
        if status:
            continue
        row[0] = int(run.result["success"])
        row[1] = _mask(run.result["dishonest"])
        row[2] = _mask(run.error_ranks)
        for r in range(1, n + 1):
            p = parties[r]
            row[4 + 5 * r:9 + 5 * r] = (run.result["decisions"][r - 1], _mask(p.Vi) if r > 1 else 0,
                                        p.stats.accept, p.stats.reject, p.stats.sent)
    return out


def _host_lists(lists, count: int) -> np.ndarray:
    """Sampled lists (a device tensor or an array, rows possibly padded) as a
    host array [n+1, count]."""
    if hasattr(lists, "cpu"):
        lists = lists.cpu().numpy()
    return np.asarray(lists)[:, :count]


def summarize(n: int, out: np.ndarray) -> dict:
    """Totals of result rows [runs, out_words(n)]: runs, successes, rate, the
    runs with an empty-V_i error, and the histogram of the honest ranks'
    decisions {value: count} (-1 = empty V_i).  QbaError on a nonzero status."""
    out = np.asarray(out).reshape(-1, out_words(n))
    bad = np.nonzero(out[:, 3])[0]
    if len(bad):
        raise QbaError(f"{len(bad)} instance(s) ended with a nonzero status "
                       f"(first: instance {int(bad[0])}, status {int(out[bad[0], 3])})")
    runs = len(out)
    ok = int(out[:, 0].sum())
    dec = out[:, 4 + 5:4 + 5 * (n + 1):5]                                # ranks 1..n
    honest = ((out[:, 1:2] >> np.arange(1, n + 1)) & 1) == 0
    vals, cnt = np.unique(dec[honest], return_counts=True)
    return {"runs": runs, "successes": ok, "rate": ok / runs if runs else 0.0,
            "empty_vi_runs": int(np.count_nonzero(out[:, 2])),
            "decisions": {int(v): int(c) for v, c in zip(vals, cnt)}}


# The tally of a block of rows (qba_montecarlo_tally, qba.h): int64 words per slice.
TALLY_WORDS = 32
(T_RUNS, T_SUCCESSES, T_EMPTY_VI, T_STATUS_ROWS, T_STATUS_OR, T_CMD_DISHONEST, T_CMD_DISHONEST_OK, T_ACCEPT, T_REJECT,
 T_SENT, T_CAPTURE) = range(11)
T_DEC_NEG, T_DEC0 = 15, 16     # honest decisions equal to -1; equal to v at T_DEC0 + v, 0 <= v < 16
SEL_FAILED, SEL_EMPTY_VI, SEL_STATUS = 1, 2, 4


def tally_host(n: int, rows, inst_base: int = 0, select: int = 0):
    """The specification of qba_montecarlo_tally in numpy: rows int32 [n_inst,
    out_words(n)] or [K, n_inst, out_words(n)].  Returns ``(tally, matches)``:
    the words the call adds to a zeroed tally, int64 [K, TALLY_WORDS], and per
    slice the sorted global indices ``inst_base + i`` of all rows that
    ``select`` matches (the device keeps at most its buffer's capacity of
    them).  A row with a nonzero status counts in T_RUNS, T_STATUS_ROWS and
    T_STATUS_OR only, whatever its other fields hold."""
    rows = np.asarray(rows)
    if rows.ndim == 2:
        rows = rows[None]
    if rows.ndim != 3 or rows.shape[2] != out_words(n) or rows.dtype != np.int32:
        raise ValueError(f"rows must be int32 [n_inst, {out_words(n)}] or [K, n_inst, {out_words(n)}]")
    if not 0 <= select <= 7:
        raise ValueError("select is an or of SEL_FAILED, SEL_EMPTY_VI and SEL_STATUS")
    tally = np.zeros((rows.shape[0], TALLY_WORDS), np.int64)
    matches = []
    for out, t in zip(rows, tally):
        st = out[:, 3]
        live = out[st == 0]
        ok, dis = live[:, 0] != 0, live[:, 1]
        cmd = ((dis >> 1) & 1) != 0
        per_rank = live[:, 4 + 5:].reshape(len(live), n, 5).astype(np.int64)   # ranks 1..n
        t[T_RUNS], t[T_SUCCESSES], t[T_EMPTY_VI] = len(out), ok.sum(), np.count_nonzero(live[:, 2])
        t[T_STATUS_ROWS] = np.count_nonzero(st)
        t[T_STATUS_OR] = np.bitwise_or.reduce(st.astype(np.int64) & _U32) if len(st) else 0
        t[T_CMD_DISHONEST], t[T_CMD_DISHONEST_OK] = cmd.sum(), (cmd & ok).sum()
        t[T_ACCEPT], t[T_REJECT], t[T_SENT] = (per_rank[:, :, f].sum() for f in (2, 3, 4))
        honest = ((dis[:, None] >> np.arange(1, n + 1)) & 1) == 0
        dec = per_rank[:, :, 0][honest]
        t[T_DEC_NEG] = np.count_nonzero(dec == -1)
        t[T_DEC0:T_DEC0 + 16] = np.bincount(dec[(dec >= 0) & (dec < 16)], minlength=16)
        hit = np.zeros(len(out), bool)
        if select & SEL_FAILED:
            hit |= (st == 0) & (out[:, 0] == 0)
        if select & SEL_EMPTY_VI:
            hit |= (st == 0) & (out[:, 2] != 0)
        if select & SEL_STATUS:
            hit |= st != 0
        t[T_CAPTURE] = np.count_nonzero(hit)
        matches.append([int(inst_base) + int(i) for i in np.nonzero(hit)[0]])
    return tally, matches


def summary_from_tally(n: int, tally_row) -> dict:
    """:func:`summarize` from one slice of a tally: the same five keys with the
    same values, then ``cmd_dishonest_runs``, ``cmd_dishonest_successes`` and
    the sums ``accept``, ``reject``, ``sent`` over ranks 1..n.  QbaError when
    rows ended with a nonzero status."""
    t = [int(x) for x in np.asarray(tally_row).reshape(TALLY_WORDS)]
    if t[T_STATUS_ROWS]:
        raise QbaError(f"{t[T_STATUS_ROWS]} instance(s) ended with a nonzero status "
                       f"(the or of their statuses: {t[T_STATUS_OR]})")
    runs, ok = t[T_RUNS], t[T_SUCCESSES]
    dec = {v - T_DEC0: t[v] for v in range(T_DEC_NEG, T_DEC0 + 16) if t[v]}
    return {"runs": runs, "successes": ok, "rate": ok / runs if runs else 0.0, "empty_vi_runs": t[T_EMPTY_VI],
            "decisions": dec, "cmd_dishonest_runs": t[T_CMD_DISHONEST],
            "cmd_dishonest_successes": t[T_CMD_DISHONEST_OK], "accept": t[T_ACCEPT], "reject": t[T_REJECT],
            "sent": t[T_SENT]}


def _batches(n: int, k: int, runs: int, batch: int, seed: int, engine, decide, tally: bool, failures: int,
             explain=None) -> list:
    """The summaries of the ``k`` slices of ``runs`` instances decided ``batch``
    at a time, the batch at offset ``off`` under key ``seed + off``:
    ``decide(key, b)`` returns the rows of the b instances from ``key`` on,
    [k, b, words] (or [b, words] when k == 1); ``decide(key, b, out=buffer)``
    writes them to ``buffer``, always [k, b, words].

    Without ``tally`` and ``failures`` the batches' rows (each call's own
    buffer) are joined on the host and go through :func:`summarize`.  Otherwise
    they are tallied on the device: one row buffer of ``batch`` instances
    serves every batch, and only the [k, 32] tally (and the [k, failures]
    captured indices) come to the host, for :func:`summary_from_tally`.

    ``explain`` (with ``failures``): ``(slices, flip_q16, cap)``, ``slices[j]``
    the ``(sizeL, n_dishonest, word)`` of slice j.  After the last batch one
    montecarlo_trace_sampled call per slice re-runs that slice's captured
    failures, fed by its capture row and match count as they lie on the device;
    the tally, the indices and the transcripts then come to the host together,
    and every summary gets ``trace`` = (rows, counts, events) in the order of
    ``failed_runs``."""
    import torch
    if runs < 0 or batch < 1:
        raise ValueError("runs >= 0 and batch >= 1")
    words = out_words(n)
    steps = [(off, min(batch, runs - off), (int(seed) + off) & MASK64) for off in range(0, runs, batch)]
    if not (tally or failures):
        outs = [decide(key, b).view(k, b, words) for _, b, key in steps]
        rows = torch.cat(outs, dim=1).cpu().numpy() if outs else np.zeros((k, 0, words), np.int32)
        return [summarize(n, r) for r in rows]
    if failures < 0:
        raise ValueError("failures >= 0")
    dev = engine.device
    tal = torch.zeros((k, TALLY_WORDS), dtype=torch.int64, device=dev)
    capture = torch.zeros((k, failures), dtype=torch.int64, device=dev) if failures else None
    buf = torch.empty(k * min(batch, runs) * words, dtype=torch.int32, device=dev)
    for off, b, key in steps:
        out = buf[:k * b * words].view(k, b, words)
        decide(key, b, out=out)
        engine.montecarlo_tally(n, out, tal, inst_base=off, select=SEL_FAILED if failures else 0, capture=capture)
    traces = []
    if explain and failures:
        slices, flip, ev_cap = explain
        for j, (c, kd, word) in enumerate(slices):
            traces.append(engine.montecarlo_trace_sampled(n, kd, seed, capture[j], c, cap=ev_cap, flip_q16=flip,
                                                          adversary=word, n_match=tal[j, T_CAPTURE:T_CAPTURE + 1]))
    host = tal.cpu().numpy()  # the one synchronisation: every launch above is done when it returns
    res = [summary_from_tally(n, row) for row in host]
    if failures:
        cap = capture.cpu().numpy()
        for j, s in enumerate(res):
            s["failed_total"] = int(host[j, T_CAPTURE])
            got = cap[j, :min(failures, s["failed_total"])]
            s["failed_runs"] = sorted(int(i) for i in got)
            if traces:
                order = np.argsort(got, kind="stable")
                s["trace"] = tuple(t.cpu().numpy()[order] for t in traces[j])
    return res


def _nq(n: int) -> int:
    return int(n).bit_length()  # ceil(log2(n + 1)), tfg.py:317


def masks_from_tables(n: int, flat) -> dict:
    """What the protocol keeps of an instance's count tables ``flat`` = [H | C
    | P] (``count_tables``), as qba_k_protocol's prologue distils it:

    ``pnz``   int, bit u: P[u] != 0
    ``hmask`` [w, n+1], bit x: H[u][g][x] != 0
    ``czero`` [w, n+1], bit h: C[u][g][h] == 0
    ``rep``   [w, n+1], min h with C[u][g][h] == P[u]
    """
    g, w = n + 1, 1 << _nq(n)
    flat = np.asarray(flat)
    h, c = w * g * w, w * g * g
    H, C, P = flat[:h].reshape(w, g, w), flat[h:h + c].reshape(w, g, g), flat[h + c:h + c + w]
    bits_w, bits_g = 1 << np.arange(w, dtype=np.int64), 1 << np.arange(g, dtype=np.int64)
    return {"pnz": int(((P != 0) * bits_w).sum()),
            "hmask": ((H != 0) * bits_w).sum(axis=2),
            "czero": ((C == 0) * bits_g).sum(axis=2),
            "rep": np.argmax(C == P[:, None, None], axis=2)}  # the diagonal is |P_u|: a hit always exists


def masks_from_lists(n: int, lists) -> dict:
    """The same four, straight from the lists [n+1, sizeL] with no counter: each
    is a bitwise reduction over the Q-correlated entries (L0 != L1) of P_u,
    u = L1.  With E(g) = the entry's equal-pair mask {h : L_h == L_g}:

    =================================  =========================================
    the tables give                    over the entries of P_u it is
    =================================  =========================================
    P[u] != 0                          OR of "an entry with this u exists"
    x with H[u][g][x] != 0             OR of 1 << L_g
    h with C[u][g][h] == 0             complement of OR of E(g)
    rep(u, g)                          lowest bit of AND of E(g) (all ones for
                                       an empty P_u: rep = 0)
    =================================  =========================================

    This is what the fused kernels compute in LDS (csrc/qba_proto_rounds.h).
    Values >= w at a Q-correlated position are an error (ST_RANGE there,
    ValueError here), as in ``Engine.count_tables``."""
    g, w = n + 1, 1 << _nq(n)
    L = np.asarray(lists, dtype=np.int64).reshape(g, -1)
    q = L[:, L[0] != L[1]]
    if q.size and q.max() >= w:
        raise ValueError("lists hold values >= w at Q-correlated positions")
    pnz = 0
    hmask = np.zeros((w, g), np.int64)
    eq_or = np.zeros((w, g), np.int64)
    eq_and = np.full((w, g), -1, np.int64)
    bits_g = 1 << np.arange(g, dtype=np.int64)
    for k in range(q.shape[1]):
        e = q[:, k]
        u = int(e[1])
        E = ((e[:, None] == e[None, :]) * bits_g).sum(axis=1)  # E(g), bit h
        pnz |= 1 << u
        hmask[u] |= 1 << e
        eq_or[u] |= E
        eq_and[u] &= E
    return {"pnz": pnz, "hmask": hmask, "czero": ~eq_or & ((1 << g) - 1),
            "rep": np.array([[(int(a) & -int(a)).bit_length() - 1 for a in row] for row in eq_and])}


def run(n: int, sizeL: int, n_dishonest: int, runs: int, seed: int, engine, packed: bool = True,
        batch: int = 4096, path: str = "tables", tally: bool = False, failures: int = 0, flip_q16: int = 0,
        adversary: Optional[int] = None, explain: int = 0, coalition: Optional[int] = None,
        net: Optional[int] = None, noise=None) -> dict:
    """``runs`` independent instances on the device, ``batch`` at a time, batch
    at offset ``off`` under key ``seed + off``; only the result rows are copied
    to the host.  Returns :func:`summarize` of all rows.

    ``path="tables"`` (the default): sample_check_batched then
    protocol_batched; the list buffer is reused across batches.
    ``path="fused"``: one montecarlo_sampled call per batch -- the same
    instances and rows, with no list buffer and no count tables (``packed``
    has nothing to apply to).

    ``tally=True`` (implied by ``failures > 0``): the rows stay on the device,
    in one buffer of ``batch`` instances, and montecarlo_tally reduces each
    batch there; the result is :func:`summary_from_tally`, whose memory does
    not grow with ``runs``.  ``failures=F`` adds ``failed_runs``, the sorted
    indices of up to F runs without success (run i has key ``seed + i``), and
    ``failed_total``, how many there were.

    ``flip_q16=k > 0`` (``path="fused"`` or ``path="tables_noisy"``): every
    measured bit flips with probability k / 65536.  ``"tables_noisy"`` is the
    tables path through the noisy batched sampler
    (``sample_check_batched(..., flip_q16=k)``): the same rows as ``"fused"``;
    with ``flip_q16=0`` it is ``"tables"``.

    ``adversary=word`` (any path): the dishonest parties follow that policy
    (:func:`adversary`); the decisions go through the ``_adv`` kernels.

    ``explain=cap > 0`` (with ``failures``): adds ``trace``, the device
    transcripts ``(rows, counts, events)`` of ``failed_runs`` with at most
    ``cap`` stored events per rank (``Engine.montecarlo_trace_sampled``, fed
    from the capture buffer on the device; :func:`format_trace` renders one).
    Every path's rows are equal, so the fused trace explains them all.

    ``coalition=word`` (``path="fused"`` only, without ``explain``): the
    dishonest parties collude (:func:`coalition`); the decisions go through the
    coalition kernel as a curve of the one checkpoint ``sizeL``.  ``None`` and
    ``0`` call what is called without the argument.

    ``net=word`` (``path="fused"`` only, without ``explain`` or ``coalition``):
    packets are lost in flight (:func:`net`); the decisions go through the
    lossy-network kernel as a curve of the one checkpoint ``sizeL``.  ``None``
    and ``0`` call what is called without the argument.

    ``noise=(rates, depol_q16)`` (``path="fused"`` only; not with ``flip_q16``,
    ``coalition``, a non-zero ``net`` or ``explain``): a noise profile
    (:func:`noise_profile`); the decisions go through the noise-profile kernel
    as a curve of the one checkpoint ``sizeL``.  ``None`` calls what is called
    without the argument."""
    if path not in ("tables", "fused", "tables_noisy"):
        raise ValueError("path is 'tables', 'fused' or 'tables_noisy'")
    if noise is not None:
        if path != "fused":
            _no_profile(noise, f"path={path!r}")
        return curve(n, [sizeL], n_dishonest, runs, seed, engine, batch=batch, tally=tally, failures=failures,
                     flip_q16=flip_q16, adversary=adversary, explain=explain, coalition=coalition, net=net,
                     noise=noise)[int(sizeL)]
    if net is not None and check_net(net):
        if path != "fused":
            _no_net(net, f"path={path!r}")
        return curve(n, [sizeL], n_dishonest, runs, seed, engine, batch=batch, tally=tally, failures=failures,
                     flip_q16=flip_q16, adversary=adversary, explain=explain, coalition=coalition,
                     net=net)[int(sizeL)]
    if coalition is not None and check_coalition(coalition):
        if path != "fused" or explain:
            raise ValueError("coalition needs path='fused' and no explain: the tables path and the trace "
                             "kernels do not collude")
        return curve(n, [sizeL], n_dishonest, runs, seed, engine, batch=batch, tally=tally, failures=failures,
                     flip_q16=flip_q16, adversary=adversary, coalition=coalition)[int(sizeL)]
    noise = {"flip_q16": _check_flip(flip_q16)} if flip_q16 else {}
    if noise and path == "tables":
        raise ValueError("flip_q16 > 0 needs path='fused' or path='tables_noisy'")
    adv = {} if adversary is None else {"adversary": check_adversary(adversary)}
    lists = None

    def decide(key, b, out=None):
        nonlocal lists
        into = {} if out is None else {"out": out[0]}
        if path == "fused":
            return engine.montecarlo_sampled(n, n_dishonest, key, b, sizeL, **into, **noise, **adv)
        buf, counts = engine.sample_check_batched(n, key, b, sizeL, None if lists is None else lists[:b],
                                                  packed=packed, **noise)
        if lists is None:
            lists = buf
        return engine.protocol_batched(n, n_dishonest, key, counts, **into, **adv)
    ex = ([(sizeL, n_dishonest, adversary)], flip_q16, explain) if explain else None
    return _batches(n, 1, runs, batch, seed, engine, decide, tally, failures, ex)[0]


def curve_host(n: int, counts, n_dishonest: int, n_inst: int, seed_base: int, engine, lists=None,
               flip_q16: int = 0, adversary: Optional[int] = None, coalition: Optional[int] = None,
               net: Optional[int] = None, noise=None) -> np.ndarray:
    """The specification of the curve calls: the stack of :func:`run_host` at
    each count of ``counts``, int32 [len(counts), n_inst, out_words(n)].
    Injected ``lists`` [n_inst, n+1, >= max(counts)] are truncated to
    ``[:, :, :c]`` for the count c.  ``flip_q16`` as in :func:`run_host` (the
    flips of entry e are the same at every count), ``adversary``,
    ``coalition`` and ``net`` (a packet's loss does not depend on the count),
    and ``noise`` (a profile's masks of entry e are the same at every count)."""
    counts = [int(c) for c in counts]
    li = None if lists is None else np.asarray(lists)
    how = {"flip_q16": flip_q16} if flip_q16 else {}
    if adversary is not None:
        how["adversary"] = adversary
    if coalition is not None:
        how["coalition"] = coalition
    if net is not None:
        how["net"] = net
    if noise is not None:
        how["noise"] = noise
    rows = [run_host(n, c, n_dishonest, n_inst, seed_base, engine, lists=None if li is None else li[:, :, :c],
                     **how)
            for c in counts]
    return np.stack(rows) if rows else np.zeros((0, n_inst, out_words(n)), np.int32)


def curve(n: int, counts, n_dishonest: int, runs: int, seed: int, engine, batch: int = 4096, tally: bool = False,
          failures: int = 0, flip_q16: int = 0, adversary: Optional[int] = None, explain: int = 0,
          coalition: Optional[int] = None, net: Optional[int] = None, noise=None) -> dict:
    """The failure curve over sizeL: ``runs`` instances, ``batch`` at a time as
    :func:`run` keys them, each decided at every sizeL of the strictly
    increasing ``counts`` by one montecarlo_curve_sampled call per batch.
    Returns ``{sizeL: summarize(...)}`` in checkpoint order; the summary at
    sizeL = c is that of ``run(n, c, ..., path="fused")``.  ``tally`` and
    ``failures`` as in :func:`run`, per checkpoint; ``flip_q16``,
    ``adversary`` and ``explain`` as there (one trace call per checkpoint).
    ``coalition=word`` (not with ``explain``): one
    montecarlo_curve_sampled_coal call per batch instead; ``None`` and ``0``
    call what is called without it.  ``net=word`` (not with ``explain`` or
    ``coalition``): one montecarlo_curve_sampled_net call per batch instead;
    ``None`` and ``0`` call what is called without it.  ``noise=(rates,
    depol_q16)`` (not with ``flip_q16``, ``coalition``, a non-zero ``net`` or
    ``explain``): one montecarlo_curve_sampled_nprof call per batch instead;
    ``None`` calls what is called without it."""
    counts = [int(c) for c in counts]
    prof = None if noise is None else check_noise_profile(n, *noise)
    noise = {"flip_q16": _check_flip(flip_q16)} if flip_q16 else {}
    if adversary is not None:
        noise["adversary"] = check_adversary(adversary)
    coal = 0 if coalition is None else check_coalition(coalition)
    lossy = 0 if net is None else check_net(net)
    if prof is not None:
        _profile_alone(noise.get("flip_q16", 0), coal, lossy, explain)
    if lossy and coal:
        _no_net(lossy, "a coalition")
    if lossy and explain:
        _no_net(lossy, "explain (the trace kernels)")
    if coal and explain:
        raise ValueError("explain is not built for a coalition: the trace kernels do not collude")
    if tally or failures:
        engine._check_curve(n, n_dishonest, 0, counts)  # before any device buffer: an empty list has no slice

    def decide(key, b, **into):
        if prof is not None:
            return engine.montecarlo_curve_sampled_nprof(n, n_dishonest, key, b, counts, noise=prof, **into, **noise)
        if lossy:
            return engine.montecarlo_curve_sampled_net(n, n_dishonest, key, b, counts, net=lossy, **into, **noise)
        if coal:
            return engine.montecarlo_curve_sampled_coal(n, n_dishonest, key, b, counts, coalition=coal, **into,
                                                        **noise)
        return engine.montecarlo_curve_sampled(n, n_dishonest, key, b, counts, **into, **noise)
    ex = ([(c, n_dishonest, adversary) for c in counts], flip_q16, explain) if explain else None
    return dict(zip(counts, _batches(n, len(counts), runs, batch, seed, engine, decide, tally, failures, ex)))


def _scenarios(n: int, scenarios) -> list:
    """``scenarios`` as a list of ``(n_dishonest, checked policy word)``."""
    try:
        sc = [(int(k), word) for k, word in scenarios]
    except (TypeError, ValueError):
        raise QbaError("scenarios must be a sequence of (n_dishonest, policy word) pairs") from None
    for i, (k, word) in enumerate(sc):
        if not 0 <= k <= n:
            raise QbaError(f"scenario {i}: n_dishonest={k} outside [0, {n}]")
        sc[i] = (k, check_adversary(word))
    return sc


def sweep_host(n: int, counts, scenarios, n_inst: int, seed_base: int, engine, lists=None,
               flip_q16: int = 0) -> np.ndarray:
    """The specification of the sweep calls: the stack
    of :func:`curve_host` under each scenario ``(n_dishonest, word)`` of
    ``scenarios``, int32 [len(counts), len(scenarios), n_inst, out_words(n)].

    Under one key the traitor draw is a partial Fisher-Yates
    (:meth:`ProtocolRng.choice`): the traitors at k are the first k of the
    traitors at k + 1.  Scenarios that differ in ``n_dishonest`` therefore run
    on nested traitor sets, the same lists and the same commander's order."""
    sc = _scenarios(n, scenarios)
    rows = [curve_host(n, counts, k, n_inst, seed_base, engine, lists=lists, flip_q16=flip_q16, adversary=word)
            for k, word in sc]
    if not rows:
        return np.zeros((len(list(counts)), 0, n_inst, out_words(n)), np.int32)
    return np.stack(rows, axis=1)


def sweep(n: int, counts, scenarios, runs: int, seed: int, engine, batch: int = 4096, tally: bool = False,
          failures: int = 0, flip_q16: int = 0, explain: int = 0, net: Optional[int] = None, noise=None) -> dict:
    """:func:`curve` under every scenario ``(n_dishonest, word)`` of
    ``scenarios`` at once: ``runs`` instances, ``batch`` at a time as
    :func:`run` keys them, each sampled and distilled once and decided at every
    sizeL of ``counts`` under every scenario by one montecarlo_sweep_sampled
    call per batch (at most 16 scenarios and 32 slices).  Returns ``{(sizeL,
    n_dishonest, word): summary}`` in slice order, checkpoints outermost; each
    summary is that of ``curve(..., n_dishonest, adversary=word)`` at that
    sizeL.  ``tally``, ``failures``, ``flip_q16`` and ``explain`` as there (one
    trace call per slice).  Duplicate scenarios would share a key: ValueError.
    ``net`` is taken only to be refused when it is a non-zero network word,
    ``noise`` when it is a noise profile."""
    _no_net(net, "a sweep")
    _no_profile(noise, "a sweep")
    counts = [int(c) for c in counts]
    sc = _scenarios(n, scenarios)
    if len(set(sc)) != len(sc):
        raise ValueError("duplicate scenarios: every (n_dishonest, word) may be given once")
    noise = {"flip_q16": _check_flip(flip_q16)} if flip_q16 else {}
    engine._check_sweep(n, 0, counts, sc)  # before any device buffer: an empty grid has no slice
    k = len(counts) * len(sc)

    keys = [(c, kd, word) for c in counts for kd, word in sc]

    def decide(key, b, out=None):
        into = {} if out is None else {"out": out}
        return engine.montecarlo_sweep_sampled(n, key, b, counts, sc, **into, **noise).view(k, b, out_words(n))
    ex = (keys, flip_q16, explain) if explain else None
    return dict(zip(keys, _batches(n, k, runs, batch, seed, engine, decide, tally, failures, ex)))


def _grid_scenarios(n: int, scenarios) -> list:
    """``scenarios`` as a list of ``(n_dishonest, checked policy word, checked
    network word)``; an error names the scenario by its index."""
    try:
        sc = [(int(k), word, net) for k, word, net in scenarios]
    except (TypeError, ValueError):
        raise QbaError("scenarios must be a sequence of (n_dishonest, policy word, network word) triples") from None
    for i, (k, word, net) in enumerate(sc):
        if not 0 <= k <= n:
            raise QbaError(f"scenario {i}: n_dishonest={k} outside [0, {n}]")
        try:
            sc[i] = (k, check_adversary(word), check_net(net))
        except QbaError as e:
            raise QbaError(f"scenario {i}: {e}") from None
    return sc


def grid_host(n: int, counts, scenarios, n_inst: int, seed_base: int, engine, lists=None,
              flip_q16: int = 0) -> np.ndarray:
    """The specification of the grid calls: the stack
    of :func:`curve_host` under each scenario ``(n_dishonest, word, net)`` of
    ``scenarios``, int32 [len(counts), len(scenarios), n_inst, out_words(n)].

    Under one key the lists, the traitor draw and the commander's order are the
    same in every scenario (:func:`sweep_host`), and :func:`net_lost` compares
    a word that does not depend on ``drop_q16``: a packet lost at ``drop_q16 =
    K`` is lost at every ``K' >= K``.  Scenarios that differ in ``drop_q16``
    alone therefore lose nested sets of the packets they have in common."""
    sc = _grid_scenarios(n, scenarios)
    rows = [curve_host(n, counts, k, n_inst, seed_base, engine, lists=lists, flip_q16=flip_q16, adversary=word,
                       net=net)
            for k, word, net in sc]
    if not rows:
        return np.zeros((len(list(counts)), 0, n_inst, out_words(n)), np.int32)
    return np.stack(rows, axis=1)


def grid(n: int, counts, scenarios, runs: int, seed: int, engine, batch: int = 4096, tally: bool = False,
         failures: int = 0, flip_q16: int = 0, noise=None) -> dict:
    """:func:`curve` under every scenario ``(n_dishonest, word, net)`` of
    ``scenarios`` at once: ``runs`` instances, ``batch`` at a time as
    :func:`run` keys them, each sampled and distilled once and decided at every
    sizeL of ``counts`` under every scenario by one montecarlo_grid_sampled call
    per batch (at most 16 scenarios and 32 slices).  Returns ``{(sizeL,
    n_dishonest, word, net): summary}`` in slice order, checkpoints outermost;
    each summary is that of ``curve(..., n_dishonest, adversary=word, net=net)``
    at that sizeL.  ``tally``, ``failures`` and ``flip_q16`` as there.  There is
    no ``explain``: the trace kernels are not built for a lossy network.
    Duplicate scenarios would share a key: ValueError.  ``noise`` is taken only
    to be refused when it is a noise profile."""
    _no_profile(noise, "a grid")
    counts = [int(c) for c in counts]
    sc = _grid_scenarios(n, scenarios)
    if len(set(sc)) != len(sc):
        raise ValueError("duplicate scenarios: every (n_dishonest, word, net) may be given once")
    noise = {"flip_q16": _check_flip(flip_q16)} if flip_q16 else {}
    engine._check_grid(n, 0, counts, sc)  # before any device buffer: an empty grid has no slice
    k = len(counts) * len(sc)
    keys = [(c, kd, word, net) for c in counts for kd, word, net in sc]

    def decide(key, b, out=None):
        into = {} if out is None else {"out": out}
        return engine.montecarlo_grid_sampled(n, key, b, counts, sc, **into, **noise).view(k, b, out_words(n))
    return dict(zip(keys, _batches(n, k, runs, batch, seed, engine, decide, tally, failures, None)))


# ---------------------------------------------------------------------------
# The transcript of a run
# ---------------------------------------------------------------------------
EV_RECV, EV_SEND, EV_DECIDE = 1, 2, 3
EV_HONEST = 7                       # SEND code of an honest sender
EV_SLOT_FULL, EV_SLOT_MUTED = 30, 31
EV_SLOT_LOST = 29                   # SEND slot of a packet lost in flight (section 13.13)
EV_NO_PACKET = 6                    # RECV code of a lieutenant whose commander packet was lost
TRACE_CAP_MAX = 4096
PKT_CLEARED, PKT_EMPTY = 1 << 8, 1 << 13
VERDICTS = ("accepted", "Cond1", "Cond2", "Cond3", "known v", "wrong length")
ACTIONS = ("maybe not send", "replace the order", "clear P", "clear L", "relay")


def event_head(kind: int, rnd: int = 0, peer: int = 0, slot: int = 0, code: int = 0, length: int = 0) -> int:
    """kind [0:3) | round [3:8) | peer [8:12) | slot [12:17) | code [17:21) | len [21:26)"""
    return kind | rnd << 3 | peer << 8 | slot << 12 | code << 17 | length << 21


def event_fields(head: int) -> dict:
    h = int(head) & _U32
    return {"kind": h & 7, "round": (h >> 3) & 31, "peer": (h >> 8) & 15, "slot": (h >> 12) & 31,
            "code": (h >> 17) & 15, "len": (h >> 21) & 31}


def packet_word(P, v, L) -> int:
    """The packet (P, v, L) of a CountParty as the 32-bit word of the decision
    kernels (csrc/qba_proto_rounds.h), in the form the events carry: v [0:4) |
    P's u [4:8) | P cleared [8] | the tuples' u [9:13) | an empty tuple present
    [13] | mask of the tuples' representatives [16:32); P's u is 0 under the
    cleared bit and the tuples' u is 0 when no tuple is left."""
    descs = [d for d in L if d != ()]
    mask = 0
    for _, rep in descs:
        mask |= 1 << rep
    cleared = P.u is None
    return (int(v) | (0 if cleared else int(P.u) << 4) | (PKT_CLEARED if cleared else 0) |
            ((descs[0][0] << 9) if descs else 0) | (PKT_EMPTY if () in L else 0) | mask << 16)


class TraceParty(AdversaryParty):
    """AdversaryParty that writes down what it does: ``events``, the list of
    ``(head, pkt)`` of its rank in the order of its own calls, which is the
    order of the lane's loop in the trace kernels.  The verdict of a received
    packet comes from Cond1, Cond2 and Cond3 evaluated in order on the same
    CountTables, and its boolean is asserted against ``consistent``'s."""

    sink = None  # {rank: party} of the run, set on the subclass trace_host makes

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.events = []
        self._rnd = 0          # 0: the commander's epoch
        self._inbox = []       # (source, slot, word) of the drained, unprocessed packets
        self._slots = (None, {})  # the round the send slots belong to, {dest: sends so far}
        if self.sink is not None:
            self.sink[self.rank] = self

    def _put(self, kind, peer, slot, code, length, pkt):
        self.events.append((event_head(kind, self._rnd, peer, slot, code, length), int(pkt) & _U32))

    def verdict(self, v, L) -> int:
        """0, or the first of Cond1, Cond2, Cond3 (tfg.py:87-98) that fails."""
        t = self.tables
        if len({t.length(d) for d in L}) != 1:
            return 1
        descs = [d for d in L if d != ()]
        if any(t.H[u, g, int(v)] != 0 for u, g in descs):
            return 2
        if any(t.C[a[0], a[1], b[1]] != 0 for i, a in enumerate(descs) for b in descs[i + 1:]):
            return 3
        return 0

    def recv(self, src):
        P, v, L = super().recv(src)
        self._inbox.append((src, sum(1 for s, _, _ in self._inbox if s == src), packet_word(P, v, L)))
        return P, v, L

    def add_own_and_check(self, P, v, L, pre=None) -> bool:
        src, slot, word = self._inbox.pop(0)
        L.add(self.own_tuple(P))
        code = self.verdict(v, L)
        ok = code == 0
        assert ok == self.tables.consistent(v, L), "the verdict and consistent() disagree"
        self._tally(ok)
        if ok:  # what lieu_receive tests next (epoch 0: V_i is empty and the one list is the own)
            code = 4 if v in self.Vi else 5 if len(L) != self._rnd + 1 else 0
        self._put(EV_RECV, src, slot, code, len(L), word)
        return ok

    def lieu_receive(self, P, v, L, rnd, pre=None):
        self._rnd = rnd
        super().lieu_receive(P, v, L, rnd, pre)

    def send(self, dest, P, v, L):
        if self.rank == 1:
            self._put(EV_SEND, dest, 0, EV_HONEST, len(L), packet_word(P, v, L))
        super().send(dest, P, v, L)

    def lieu_broadcast(self, P, v, L):
        """AdversaryParty.lieu_broadcast, draw for draw, with a SEND event per
        destination (trace_host's rows are held to run_host's)."""
        acts = [a for a in range(5) if (self.adv >> a) & 1]
        order, fresh = (self.adv >> 8) & 3, (self.adv >> 12) & 1
        if self._slots[0] != self._rnd:
            self._slots = (self._rnd, {})
        P0, v0, L0 = P, v, L
        for dest in range(2, self.n + 1):
            if dest == self.rank:
                continue
            go, action = 1, EV_HONEST
            if self.dishonest:
                if fresh:
                    P, v, L = copy.copy(P0), v0, set(L0)
                action = acts[self.rng.randint(len(acts))]
                if action == ACT_MUTE:
                    go = self.rng.randint(2)
                elif action == ACT_REORDER:
                    if order == ORDER_LOW:
                        v = 1 if int(v) == 0 else 0
                    else:
                        v = self.rng.randint(self.n + 1 if order == ORDER_REFERENCE else self.w)
                elif action == ACT_CLEAR_P:
                    P.clear()
                elif action == ACT_CLEAR_L:
                    L.clear()
            slot = EV_SLOT_MUTED
            if go:
                k = self._slots[1].get(dest, 0)
                self._slots[1][dest] = k + 1
                slot = k if k < self.w else EV_SLOT_FULL
                self.send(dest, P, v, L)
            self._put(EV_SEND, dest, slot, action, len(L), packet_word(P, v, L))


def trace_host(n: int, sizeL: int, n_dishonest: int, indices, seed_base: int, engine, lists=None,
               flip_q16: int = 0, adversary: Optional[int] = None):
    """The specification of the trace calls: :func:`run_host` of the instance
    keyed ``seed_base + i`` for every i of ``indices`` (``lists[j]`` belongs to
    ``indices[j]``) with :class:`TraceParty` at the ``party_cls`` seam.  Returns
    ``(rows, counts, events)``: int32 [k, out_words(n)], int32 [k, n+1] and, per
    index and rank 0..n, the whole list of ``(head, pkt)`` -- the device keeps
    the first ``cap`` of each.  An instance with a nonzero status has no events."""
    word = check_adversary(ADV_REFERENCE if adversary is None else adversary)
    indices = [int(i) for i in indices]
    rows = np.zeros((len(indices), out_words(n)), np.int32)
    counts = np.zeros((len(indices), n + 1), np.int32)
    events = []
    for j, i in enumerate(indices):
        sink: Dict[int, TraceParty] = {}
        cls = type(f"TraceParty_{word:x}", (TraceParty,), {"adv": word, "sink": sink})
        rows[j] = run_host(n, sizeL, n_dishonest, 1, (int(seed_base) + i) & MASK64, engine,
                           lists=None if lists is None else np.asarray(lists)[j:j + 1], party_cls=cls,
                           flip_q16=flip_q16)[0]
        per_rank = [[] for _ in range(n + 1)]
        if rows[j, 3] == 0:
            for r in range(1, n + 1):
                dec, vi = int(rows[j, 4 + 5 * r]), int(rows[j, 5 + 5 * r])
                per_rank[r] = sink[r].events + [(event_head(EV_DECIDE, length=bin(vi).count("1")), dec & _U32)]
        counts[j] = [len(e) for e in per_rank]
        events.append(per_rank)
    return rows, counts, events


class TraceNetParty(NetParty):
    """NetParty that writes down what it does: the
    events of :class:`TraceParty` on the network the word ``net`` describes,
    recorded through the ``lose`` and ``recv`` seams NetParty offers.  A send
    lost in flight is a SEND event with slot :data:`EV_SLOT_LOST`, the packet as
    it was handed over; it takes no mailbox slot.  A lieutenant whose commander
    packet was lost records one RECV event with code :data:`EV_NO_PACKET`.  Its
    draws are NetParty's, draw for draw (trace_net_host's rows are held to
    ``run_host(..., net=)``), and with ``net == 0`` its events are TraceParty's."""

    sink = None  # {rank: party} of the run, set on the subclass trace_net_host makes
    verdict = TraceParty.verdict
    _put = TraceParty._put

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.events = []
        self._rnd = 0          # 0: the commander's epoch
        self._inbox = []       # (source, slot, word) of the drained, unprocessed packets
        self._slots = (None, {})  # the round the send slots belong to, {dest: packets delivered so far}
        self._lost = False     # whether the last send was lost in flight
        if self.sink is not None:
            self.sink[self.rank] = self

    def lose(self, dest, P, v, L, epoch, seq):
        self._lost = True
        super().lose(dest, P, v, L, epoch, seq)

    def recv(self, src):
        P, v, L = super().recv(src)
        if P is NetLost:
            self._put(EV_RECV, src, 0, EV_NO_PACKET, 0, 0)
        else:
            self._inbox.append((src, sum(1 for s, _, _ in self._inbox if s == src), packet_word(P, v, L)))
        return P, v, L

    def add_own_and_check(self, P, v, L, pre=None) -> bool:
        src, slot, word = self._inbox.pop(0)
        L.add(self.own_tuple(P))
        code = self.verdict(v, L)
        ok = code == 0
        assert ok == self.tables.consistent(v, L), "the verdict and consistent() disagree"
        self._tally(ok)
        if ok:  # what lieu_receive tests next (epoch 0: V_i is empty and the one list is the own)
            code = 4 if v in self.Vi else 5 if len(L) != self._rnd + 1 else 0
        self._put(EV_RECV, src, slot, code, len(L), word)
        return ok

    def lieu_receive(self, P, v, L, rnd, pre=None):
        self._rnd = rnd
        super().lieu_receive(P, v, L, rnd, pre)

    def send(self, dest, P, v, L):
        self._lost = False
        super().send(dest, P, v, L)
        if self.rank == 1:
            self._put(EV_SEND, dest, EV_SLOT_LOST if self._lost else 0, EV_HONEST, len(L), packet_word(P, v, L))

    def lieu_broadcast(self, P, v, L):
        """AdversaryParty.lieu_broadcast, draw for draw, with a SEND event per
        destination; a packet lost in flight leaves the destination's next
        mailbox slot free."""
        acts = [a for a in range(5) if (self.adv >> a) & 1]
        order, fresh = (self.adv >> 8) & 3, (self.adv >> 12) & 1
        if self._slots[0] != self._rnd:
            self._slots = (self._rnd, {})
        P0, v0, L0 = P, v, L
        for dest in range(2, self.n + 1):
            if dest == self.rank:
                continue
            go, action = 1, EV_HONEST
            if self.dishonest:
                if fresh:
                    P, v, L = copy.copy(P0), v0, set(L0)
                action = acts[self.rng.randint(len(acts))]
                if action == ACT_MUTE:
                    go = self.rng.randint(2)
                elif action == ACT_REORDER:
                    if order == ORDER_LOW:
                        v = 1 if int(v) == 0 else 0
                    else:
                        v = self.rng.randint(self.n + 1 if order == ORDER_REFERENCE else self.w)
                elif action == ACT_CLEAR_P:
                    P.clear()
                elif action == ACT_CLEAR_L:
                    L.clear()
            slot = EV_SLOT_MUTED
            if go:
                self.send(dest, P, v, L)
                if self._lost:
                    slot = EV_SLOT_LOST
                else:
                    k = self._slots[1].get(dest, 0)
                    self._slots[1][dest] = k + 1
                    slot = k if k < self.w else EV_SLOT_FULL
            self._put(EV_SEND, dest, slot, action, len(L), packet_word(P, v, L))


def trace_net_host(n: int, sizeL: int, n_dishonest: int, indices, seed_base: int, engine, lists=None,
                   flip_q16: int = 0, adversary: Optional[int] = None, net: Optional[int] = None):
    """The specification of the ``_net`` trace calls: :func:`trace_host` with
    :class:`TraceNetParty` on the network ``net``, the same ``(rows, counts,
    events)`` layout.  With ``net`` None or 0 it is :func:`trace_host` itself."""
    lossy = 0 if net is None else check_net(net)
    if not lossy:
        return trace_host(n, sizeL, n_dishonest, indices, seed_base, engine, lists=lists, flip_q16=flip_q16,
                          adversary=adversary)
    word = check_adversary(ADV_REFERENCE if adversary is None else adversary)
    indices = [int(i) for i in indices]
    rows = np.zeros((len(indices), out_words(n)), np.int32)
    counts = np.zeros((len(indices), n + 1), np.int32)
    events = []
    for j, i in enumerate(indices):
        sink: Dict[int, TraceNetParty] = {}
        cls = type("TraceNetParty_sink", (TraceNetParty,), {"sink": sink})
        rows[j] = run_host(n, sizeL, n_dishonest, 1, (int(seed_base) + i) & MASK64, engine,
                           lists=None if lists is None else np.asarray(lists)[j:j + 1], party_cls=cls,
                           flip_q16=flip_q16, adversary=word, net=lossy)[0]
        per_rank = [[] for _ in range(n + 1)]
        if rows[j, 3] == 0:
            for r in range(1, n + 1):
                dec, vi = int(rows[j, 4 + 5 * r]), int(rows[j, 5 + 5 * r])
                per_rank[r] = sink[r].events + [(event_head(EV_DECIDE, length=bin(vi).count("1")), dec & _U32)]
        counts[j] = [len(e) for e in per_rank]
        events.append(per_rank)
    return rows, counts, events


def replay(n: int, sizeL: int, n_dishonest: int, indices, seed: int, engine, flip_q16: int = 0,
           adversary: Optional[int] = None, net: Optional[int] = None, cap: int = 1024, noise=None) -> dict:
    """The transcripts of the runs ``indices`` of a ``run`` / ``curve`` / ``grid``
    item under ``seed`` (key = seed + index, the rule of ``failed_runs``), as the
    device re-runs them: one trace call -- ``montecarlo_trace_sampled_net`` when
    ``net`` is a non-zero network word, ``montecarlo_trace_sampled`` otherwise
    -- and one synchronisation.  ``indices``: host integers or an int64 device
    tensor (a tally's capture row).  Returns ``{"indices", "rows", "counts",
    "events"}`` as host arrays, slot j belonging to ``indices[j]``;
    :func:`format_trace` renders a slot.  A coalition's runs have no transcript:
    there is no argument for its word, and ``noise`` is taken only to be
    refused when it is a noise profile."""
    _no_profile(noise, "replay (the trace kernels)")
    lossy = 0 if net is None else check_net(net)
    if lossy:
        out = engine.montecarlo_trace_sampled_net(n, n_dishonest, seed, indices, sizeL, cap=cap, flip_q16=flip_q16,
                                                  adversary=adversary, net=lossy)
    else:
        out = engine.montecarlo_trace_sampled(n, n_dishonest, seed, indices, sizeL, cap=cap, flip_q16=flip_q16,
                                              adversary=adversary)
    if hasattr(indices, "cpu"):  # the indices come to the host with the outputs, as int32 pairs
        import torch
        rows, counts, events, pairs = _to_host(out + (indices.view(torch.int32),))
        idx = [int(i) for i in np.ascontiguousarray(pairs).view(np.int64)]
    else:
        idx = [int(i) for i in indices]
        rows, counts, events = _to_host(out)
    return {"indices": idx, "rows": rows, "counts": counts, "events": events}


def _to_host(tensors) -> tuple:
    """Int32 device tensors as host arrays through one copy (one synchronisation)."""
    import torch
    flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
    out, at = [], 0
    for t in tensors:
        out.append(flat[at:at + t.numel()].reshape(tuple(t.shape)))
        at += t.numel()
    return tuple(out)


def trace_events(counts, events, j: int = 0) -> list:
    """Slot ``j`` of a device trace (int32 or uint32 arrays of
    ``Engine.montecarlo_trace_*``, on the host) as :func:`trace_host` lays its
    events out: per rank 0..n the stored ``(head, pkt)``, the first ``min(count,
    cap)`` of them."""
    ev = np.asarray(events[j]).view(np.uint32) if np.asarray(events[j]).dtype == np.int32 else np.asarray(events[j])
    return [[(int(h), int(p)) for h, p in ev[r, :min(int(c), ev.shape[1])]]
            for r, c in enumerate(np.asarray(counts[j]))]


def _bits(mask: int) -> list:
    return [b for b in range(32) if (int(mask) >> b) & 1]


def _packet_text(pkt: int, length: int) -> str:
    p = "P cleared, " if pkt & PKT_CLEARED else ""
    return f"v={pkt & 15}, {p}{length} list{'' if length == 1 else 's'}"


def format_trace(n: int, row, counts, events) -> str:
    """One instance's transcript as text, a line per event in the spirit of the
    reference's log, rank by rank: ``row`` its result row, ``counts`` [n+1] and
    ``events`` per rank the stored ``(head, pkt)`` (a list per rank, or the
    [n+1, cap, 2] array of a device trace).  ``B`` marks a dishonest rank.
    Events that were counted and not stored are reported as a count."""
    row = [int(x) for x in np.asarray(row).reshape(-1)]
    dis = row[1]
    name = lambda r: f"{'B' if (dis >> r) & 1 else ''}{r}"
    out = [f"success={row[0]} dishonest={_bits(dis)} empty V={_bits(row[2])} status={row[3]}"]
    if not isinstance(events, list):
        events = trace_events([counts], [events])
    for r in range(1, n + 1):
        for head, pkt in events[r]:
            f = event_fields(head)
            if f["kind"] == EV_RECV:
                what = "no packet arrived" if f["code"] == EV_NO_PACKET else \
                    f"accepted {_packet_text(pkt, f['len'])}" if f["code"] == 0 else \
                    f"rejected, {VERDICTS[f['code']]}" if f["code"] <= 3 else \
                    f"consistent, not taken ({VERDICTS[f['code']]}: {_packet_text(pkt, f['len'])})"
                out.append(f"[{name(r)} <- {name(f['peer'])}] round {f['round']}: {what}")
            elif f["kind"] == EV_SEND:
                act = "" if f["code"] == EV_HONEST else f" (action: {ACTIONS[f['code']]})"
                verb = {EV_SLOT_FULL: "drops (mailbox full)", EV_SLOT_LOST: "loses in flight"}.get(f["slot"], "sends")
                what = "does not send" if f["slot"] == EV_SLOT_MUTED else f"{verb} {_packet_text(pkt, f['len'])}"
                out.append(f"[{name(r)} -> {f['peer']}] round {f['round']}: {what}{act}")
            else:
                dec = pkt - (1 << 32) if pkt >> 31 else pkt
                v = "{" + ", ".join(str(b) for b in _bits(row[5 + 5 * r])) + "}"
                out.append(f"[{name(r)}] decides {dec}" + (f", V = {v}" if r > 1 else " (the commander's order)"))
        more = int(np.asarray(counts).reshape(-1)[r]) - len(events[r])
        if more > 0:
            out.append(f"[{name(r)}] ... {more} more event{'' if more == 1 else 's'} counted, not stored")
    return "\n".join(out)
