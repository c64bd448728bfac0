"""montecarlo.py on the CPU: the counter-based protocol RNG, the host
reference run_host (CountParty on that RNG), what the GPU tests' parameter
sets reach, and the C ABI of qba_protocol_batched without a device."""
import itertools
import json
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
import tfg_oracle as orc
from conftest import GOLDEN, sub
from kd_util import kernel_descriptors
from montecarlo_cases import (CASES, DUP_FAMILIES, HOSTILE, HOSTILE_IDS, INJECT_BASE, INJECT_KEYS, cpu_lists,
                              hostile_lists)
from oracle_engine import OracleEngine

mc = sub("montecarlo")
countmode = sub("countmode")
protocol = sub("protocol")


# ---------------------------------------------------------------------------
# RNG
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", [0, 1, 0x5EED, (1 << 64) - 1, 0x0123456789ABCDEF])
def test_rng_words_are_philox_on_the_stated_counters(key):
    for rank in (0, 1, 2, 15):
        rng = mc.ProtocolRng(key, rank)
        got = [rng.word() for _ in range(40)]
        ctr = np.array([[b, rank, 0, 0x51424150] for b in range(10)], np.uint32)
        want = oracle_lib.philox(ctr, key).reshape(-1)
        assert got == want.tolist()
    assert mc.ProtocolRng(key + (1 << 64), 3).word() == mc.ProtocolRng(key, 3).word()  # key mod 2^64


def test_randint_ranges_and_choice():
    rng = mc.ProtocolRng(77, 2)
    for k in (1, 2, 4, 8, 12, 16):
        draws = [rng.randint(k) for _ in range(400)]
        assert min(draws) >= 0 and max(draws) < k
        assert k == 1 or len(set(draws)) == k  # 400 draws of <= 16 values: every value
    assert not rng.capped
    for n, m in ((3, 1), (7, 2), (15, 15), (11, 0)):
        got = mc.ProtocolRng(5, 0).choice(np.arange(1, n + 1), m, replace=False)
        assert len(got) == m and len(set(got.tolist())) == m
        assert all(1 <= x <= n for x in got.tolist())
    # partial Fisher-Yates, restated
    rng, ref = mc.ProtocolRng(9, 0), mc.ProtocolRng(9, 0)
    a = list(range(1, 8))
    for j in range(3):
        s = j + ref.randint(7 - j)
        a[j], a[s] = a[s], a[j]
    assert rng.choice(np.arange(1, 8), 3, replace=False).tolist() == a[:3]


def test_randint_retry_cap_arithmetic():
    """The cap both sides share: a word is rejected when (uint32)(x * k) <
    2^32 mod k; after 64 rejected words randint gives up with `capped` set
    (the kernel's status bit 1).  Host side only: nothing forces it on the GPU."""
    class Zero(mc.ProtocolRng):
        def word(self):
            self.t += 1
            return 0

    assert mc.RNG_CAP == 64 and (mc.ST_MAILBOX, mc.ST_RNG) == (1, 2)
    r = Zero(0, 0)
    assert r.randint(3) == 0 and r.capped and r.t == 64  # 2^32 mod 3 = 1 > 0: every word rejected
    r = Zero(0, 0)
    assert r.randint(4) == 0 and not r.capped and r.t == 1  # power of two: threshold 0
    for k in list(range(1, 70)) + [1000, 65535, 65536]:
        assert (1 << 32) % k == ((1 << 32) - k) % k  # the kernel's (0u - k) % k
    # the mailbox bound: at most w distinct v can be newly added to a V_i
    for n in range(1, 16):
        w = 1 << int(n).bit_length()
        assert n + 1 <= w <= 16 and 2 * (n + 1) * ((n + 1) * w + 1) * 4 <= 32896


# ---------------------------------------------------------------------------
# host reference
# ---------------------------------------------------------------------------
def test_honest_runs_agree_on_the_commanders_order():
    n, inst = 3, 16
    out = mc.run_host(n, 200, 0, inst, 42, OracleEngine())
    assert out.shape == (inst, mc.out_words(n)) and out.dtype == np.int32
    rows = out[:, 4:].reshape(inst, n + 1, 5)
    assert np.all(out[:, 0] == 1) and np.all(out[:, 1:4] == 0)
    for r in range(2, n + 1):
        assert np.array_equal(rows[:, r, 0], rows[:, 1, 0])
        assert np.array_equal(rows[:, r, 1], 1 << rows[:, 1, 0])
    assert np.all(rows[:, 0] == 0) and np.all(rows[:, 1, 4] == n - 1)
    s = mc.summarize(n, out)
    assert s["runs"] == inst and s["successes"] == inst and s["rate"] == 1.0 and s["empty_vi_runs"] == 0
    assert sum(s["decisions"].values()) == inst * n
    bad = out.copy()
    bad[3, 3] = mc.ST_RNG
    with pytest.raises(sub("_lib").QbaError):
        mc.summarize(n, bad)


class _Seen:
    def __init__(self):
        self.tally, self.empty_desc, self.rngs = [], 0, []


def _watch(seen):
    class Watch(countmode.CountParty):
        _rnd = 0

        def lieu_receive(self, P, v, L, rnd, pre=None):
            self._rnd = rnd
            return super().lieu_receive(P, v, L, rnd, pre)

        def _tally(self, ok):
            seen.tally.append((self._rnd, bool(ok)))
            return super()._tally(ok)

        def own_tuple(self, P):
            d = super().own_tuple(P)
            if d == countmode.EMPTY and P.u is not None:
                seen.empty_desc += 1  # P[u] == 0: the EMPTY descriptor of an uncleared P
            return d

    class Rec(mc.ProtocolRng):
        def __init__(self, key, rank):
            super().__init__(key, rank)
            self.calls = []
            seen.rngs.append(self)

        def randint(self, k):
            r = super().randint(k)
            self.calls.append((k, r))
            return r

    return Watch, Rec


def _actions(calls, n):
    """A dishonest lieutenant's lieu_broadcast actions from its draws
    (tfg.py:271-283): randint(4), then randint(2) after 0, randint(n+1) after 1."""
    acts, i = set(), 0
    while i < len(calls):
        k, a = calls[i]
        assert k == 4
        acts.add(a)
        i += 1
        if a in (0, 1):
            assert calls[i][0] == (2 if a == 0 else n + 1)
            i += 1
    return acts


def test_parameter_sets_reach_every_path():
    """The GPU test's parameter sets, evaluated by the host reference alone,
    reach every path the kernel restates."""
    seen_all = dict(fail=0, empty_vi=0, dis_commander=0, actions=set(), late_accept=0, reject=0, empty_desc=0)
    golden = np.load(GOLDEN / "protocol_lists.npz")
    sets = [(k, v[0], v[1], cpu_lists(*k[::2], *v), True) for k, v in CASES.items()]
    for c in json.loads((GOLDEN / "protocol.json").read_text()):
        li = golden[c["name"]]
        sets.append(((c["n"], c["nDishonest"], c["sizeL"]), INJECT_BASE, INJECT_KEYS,
                     np.broadcast_to(li, (INJECT_KEYS,) + li.shape), False))
    for (n, nd, sizeL), base, inst, lists, sampled in sets:
        seen = _Seen()
        watch, rec = _watch(seen)
        out = mc.run_host(n, sizeL, nd, inst, base, OracleEngine(), lists=lists, party_cls=watch, rng_factory=rec)
        if sampled and n == 3:
            assert np.array_equal(out, mc.run_host(n, sizeL, nd, inst, base, OracleEngine(), lists=lists)), \
                "the seams change nothing"
        assert np.all(out[:, 3] == 0)
        assert all(bin(int(m)).count("1") == nd and not m & 1 for m in out[:, 1])
        seen_all["fail"] += int(np.sum(out[:, 0] == 0))
        seen_all["empty_vi"] += int(np.count_nonzero(out[:, 2]))
        seen_all["dis_commander"] += int(np.sum((out[:, 1] >> 1) & 1))
        seen_all["late_accept"] += sum(1 for rnd, ok in seen.tally if rnd >= 2 and ok)
        seen_all["reject"] += sum(1 for _, ok in seen.tally if not ok)
        seen_all["empty_desc"] += seen.empty_desc
        for i, row in enumerate(out):
            for rng in seen.rngs:
                if rng.key == base + i and rng.rank >= 2 and (int(row[1]) >> rng.rank) & 1:
                    seen_all["actions"] |= _actions(rng.calls, n)
    assert seen_all["actions"] == {0, 1, 2, 3}, seen_all
    for what in ("fail", "empty_vi", "dis_commander", "late_accept", "reject", "empty_desc"):
        assert seen_all[what] > 0, (what, seen_all)


# ---------------------------------------------------------------------------
# hostile sets: duplicated rows, many traitors (montecarlo_cases.HOSTILE)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostile_rows():
    """run_host's rows (CountParty) per hostile set, computed once, read-only."""
    memo = {}

    def get(case):
        if case["name"] not in memo:
            rows = mc.run_host(case["n"], case["sizeL"], case["nDishonest"], case["keys"], case["base"],
                               OracleEngine(), lists=hostile_lists(case))
            rows.setflags(write=False)
            memo[case["name"]] = rows
        return memo[case["name"]]
    return get


@pytest.mark.parametrize("case", HOSTILE, ids=HOSTILE_IDS)
def test_hostile_lists_carry_their_mutation(case):
    """The fixture's lists against its own description, in terms of the count
    tables: which C[u][g][h] equal P[u], and for `near` P[u] - 1."""
    n, fam, rows = case["n"], case["family"], case["rows"]
    _, C, P = orc.counts(hostile_lists(case)[0], n)
    full = {(u, g, h) for u in np.nonzero(P)[0] for g in range(n + 1) for h in range(g) if C[u, g, h] == P[u]}
    us = [int(u) for u in np.nonzero(P)[0]]
    if fam in ("dup_all", "dup3"):
        want = {(u, g, h) for u in us for g in rows for h in rows if h < g}
    elif fam == "dup_u":
        want = {(case["u"], rows[1], rows[0])}
    elif fam == "dup_cmd":
        want = {(u, rows[0], case["src"]) for u in us}
    else:
        u, (g, h) = case["u"], rows
        want = set()
        assert P[u] >= 2 and C[u, g, h] == P[u] - 1
    assert full == want and len(us) > 0
    assert "u" not in case or P[case["u"]] > 0


class SortedTupleParty(protocol.Party):
    """The exact-mode party on real tuples, gathered in ascending index order
    (count mode's canonical order): Python's own set of tuples de-duplicates,
    the oracle's `consistent` decides."""

    def own_tuple(self, P):
        return protocol.make_tuple(self.engine.gather(self.li, np.sort(protocol._wire(P))))


@pytest.mark.parametrize("case", HOSTILE, ids=HOSTILE_IDS)
def test_count_mode_equals_sorted_tuples_on_hostile_lists(hostile_rows, case):
    """CountParty's descriptor algebra (rep = min h with C[u][g][h] == P[u] for
    equal tuples, Cond1-3 from the counts) against real tuples: every field of
    every row.  The unsorted protocol.Party does differ on these lists (each
    rank gathers in its own set-iteration order, so equal rows need not give
    equal tuples: V_i, accept and reject counts differ on 15 of the 35 sets,
    and on other lists of these families a success flag was seen to flip):
    count mode is defined in canonical order, so that is by design and not
    asserted."""
    got = mc.run_host(case["n"], case["sizeL"], case["nDishonest"], case["keys"], case["base"], OracleEngine(),
                      lists=hostile_lists(case), party_cls=SortedTupleParty)
    want = hostile_rows(case)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        i = int(np.argwhere(got != want)[0][0])
        raise AssertionError(f"instance {i}:\ntuples {got[i].tolist()}\ncounts {want[i].tolist()}")


class _Reach:
    def __init__(self):
        self.desc = set()    # (u, g, rep) of every non-EMPTY own descriptor
        self.cond3 = set()   # (u, a, b): reps of one L rejected by Cond3 alone, C[u][a][b] != 0
        self.max_len = 0     # descriptors of the longest accepted L
        self.max_round = 0   # the latest round in which a packet was accepted
        self.max_box = 0     # most packets of one (source, destination, round)


def _reach_party(seen):
    class Reach(countmode.CountParty):
        _rnd = 0

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self._box = {}

        def lieu_receive(self, P, v, L, rnd, pre=None):
            self._rnd = rnd
            return super().lieu_receive(P, v, L, rnd, pre)

        def own_tuple(self, P):
            d = super().own_tuple(P)
            if d != countmode.EMPTY:
                seen.desc.add((d[0], self.rank, d[1]))
            return d

        def check(self, v, L):
            ok = super().check(v, L)
            if ok:
                seen.max_len = max(seen.max_len, len(L))
                seen.max_round = max(seen.max_round, self._rnd)
                return ok
            t, descs = self.tables, sorted(d for d in L if d != countmode.EMPTY)
            if len(descs) == len(L) and not any(t.H[u, g, int(v)] for u, g in descs):  # Cond1 and Cond2 hold
                seen.cond3 |= {(a[0], a[1], b[1]) for a, b in itertools.combinations(descs, 2)
                               if t.C[a[0], a[1], b[1]] != 0}
            return ok

        def send(self, dest, P, v, L):
            k = (dest, self._rnd)
            self._box[k] = self._box.get(k, 0) + 1
            seen.max_box = max(seen.max_box, self._box[k])
            super().send(dest, P, v, L)

    return Reach


def test_hostile_sets_reach_every_path(hostile_rows):
    """What the hostile sets add to test_parameter_sets_reach_every_path, on
    the host reference alone: canonicalised descriptors in every duplicate
    family (rep in {0, 1} too), a `near` pair that collides in Cond3 and does
    not canonicalise, L of >= 6 descriptors, acceptance in round >= 5, >= 3
    packets in one (source, destination, round) mailbox, V_i of >= 5 values,
    failed runs, empty V_i, and status 0 throughout."""
    got = dict(rep_ne_g={f: 0 for f in DUP_FAMILIES}, rep_01=0, near_cond3=0, max_len=0, max_round=0, max_box=0,
               max_vi=0, fail=0, empty_vi=0, runs=0)
    for case in HOSTILE:
        n, fam = case["n"], case["family"]
        seen = _Reach()
        out = mc.run_host(n, case["sizeL"], case["nDishonest"], case["keys"], case["base"], OracleEngine(),
                          lists=hostile_lists(case), party_cls=_reach_party(seen))
        assert np.array_equal(out, hostile_rows(case)), "the seam changes nothing"
        assert np.all(out[:, 3] == 0), case["name"]
        moved = {(u, g, rep) for u, g, rep in seen.desc if rep != g}
        if fam == "near":
            u, (g, h) = case["u"], case["rows"]
            assert not moved, (case["name"], moved)  # one entry apart: nothing canonicalises
            got["near_cond3"] += (u, g, h) in seen.cond3
        else:
            got["rep_ne_g"][fam] += len(moved)
            # only the duplicated rows move, and to the smallest equal row
            lo = case["src"] if fam == "dup_cmd" else case["rows"][0]
            assert all(g in case["rows"] and rep == lo for _, g, rep in moved), (case["name"], moved)
        got["rep_01"] += sum(1 for _, _, rep in moved if rep < 2)
        for what in ("max_len", "max_round", "max_box"):
            got[what] = max(got[what], getattr(seen, what))
        got["max_vi"] = max(got["max_vi"], max(bin(int(x)).count("1") for x in out[:, 5::5].ravel()))
        got["fail"] += int(np.sum(out[:, 0] == 0))
        got["empty_vi"] += int(np.count_nonzero(out[:, 2]))
        got["runs"] += len(out)
    print(got)
    assert all(c > 0 for c in got["rep_ne_g"].values()), got
    assert got["rep_01"] > 0 and got["near_cond3"] > 0, got
    assert got["max_len"] >= 6 and got["max_round"] >= 5 and got["max_box"] >= 3 and got["max_vi"] >= 5, got
    assert got["fail"] > 0 and got["empty_vi"] > 0, got


# ---------------------------------------------------------------------------
# C ABI without a device
# ---------------------------------------------------------------------------
def _call(n, nd, n_inst=1):
    lib = sub("_lib").lib()
    rc = lib.qba_protocol_batched(None, n, nd, 0, n_inst, None, None, None, None, None)
    return rc, lib.qba_last_error().decode()


def test_protocol_batched_is_exported_and_checks_its_envelope():
    lib_mod = sub("_lib")
    assert hasattr(lib_mod.lib(), "qba_protocol_batched") and "qba_protocol_batched" in lib_mod.SIGNATURES
    for n in (0, -1, 16, 1000):
        rc, msg = _call(n, 0)
        assert rc == lib_mod.QBA_EINVAL and "n_parties" in msg
    for n, nd in ((1, 2), (7, 8), (15, 16), (7, -1)):
        rc, msg = _call(n, nd)
        assert rc == lib_mod.QBA_EINVAL and "n_dishonest" in msg
    for n, nd in ((1, 0), (1, 1), (7, 2), (15, 15)):  # inside the envelope: only the device is missing
        rc, msg = _call(n, nd)
        assert rc == lib_mod.QBA_EINVAL and "ctx is NULL" in msg


def test_protocol_kernel_resources():
    """One wavefront per instance with the whole state in LDS: no scratch, and
    static + dynamic LDS at n = 15 lets 4 workgroups share a CU's 160 KiB."""
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    hits = [v for k, v in kds.items() if "qba_k_protocol" in k]
    assert len(hits) == 1
    assert hits[0]["scratch"] == 0
    assert 4 * (hits[0]["lds"] + 32896) <= 160 * 1024
