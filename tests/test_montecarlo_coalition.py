"""Colluding traitors without a GPU: the coalition
word's checks from Python and through the two C entry points, the host model
montecarlo.CoalitionParty at coal = 0 against the adversary path, the input
sets on which every field of the word shows in the rows, the stream words a
colluding traitor consumes, the events the model reaches on the recorded reach
sets (shared with tests/test_gpu_montecarlo_coalition.py, which holds both
kernels to the host model on them), and the static resources and launch shape
of the coalition kernels read from the cross-compiled library."""
import ctypes as C
import threading
from pathlib import Path

import numpy as np
import pytest

from conftest import sub
from kd_util import kernel_descriptors
from montecarlo_cases import HOSTILE, hostile_lists
from oracle_engine import OracleEngine
from test_montecarlo_adversary import BAD_WORDS, HostEngine, PRESETS, SETS, host_rows

LATE = 0x1
# one field at a time away from `late` (when [4:6), targets [8:10), starve [12])
FIELDS = {"when1": 0x11, "targets1": 0x101, "targets2": 0x201, "starve": 0x1001}
COALITIONS = {"late": 0x1, "late_relayed": 0x11, "late_one": 0x201, "starve_late": 0x1101}
WORDS = {**FIELDS, **{f"preset-{k}": v for k, v in COALITIONS.items()}}
BAD_COAL = {  # word -> what the message names
    0x2: "reserved", 0x4: "reserved", 0x8: "reserved", 0x41: "reserved", 0x81: "reserved", 0x401: "reserved",
    0x801: "reserved", 0x2001: "reserved", 0x10001: "reserved", 0x80000001: "reserved",
    0x21: "when", 0x31: "when", 0x301: "targets",
    0x10: "when", 0x100: "targets", 0x200: "targets", 0x1000: "starve", 0x1330: "when",
}
COAL_SETS = ("n3-d2-L8", "n7-d2-L8", "n7-d6-L3", "n7-d4-L60-dup_all", "n11-d3-L8")

_DUP7 = next(c for c in HOSTILE if c["name"] == "n7-d4-L60-dup_all")
_DUP3 = next(c for c in HOSTILE if c["name"] == "n7-d4-L60-dup3")
REACH_BASE, REACH_KEYS = 0xC0A1, 24
# name -> (n, n_dishonest, sizeL, seed_base, instances, injected lists or None, policy word, coalition word,
#          the events of observing() the set was chosen for)
REACH = {
    "n4-d2-L16-relayed": (4, 2, 16, REACH_BASE, REACH_KEYS, None, 0xF, 0x11,
                          ("padded_consistent", "padded_accepted", "padded_relayed", "broken")),
    "n4-d2-L16-reorder-relayed": (4, 2, 16, REACH_BASE, REACH_KEYS, None, 0x2, 0x11, ("padded_accepted", "broken")),
    "n7-d2-L16-late": (7, 2, 16, REACH_BASE, REACH_KEYS, None, 0xF, 0x1, ("short", "hold2", "padded_consistent")),
    "n7-d3-L16-starve-relayed": (7, 3, 16, REACH_BASE, REACH_KEYS, None, 0xF, 0x1011,
                                 ("padded_accepted", "padded_relayed", "hold2")),
    "n7-d4-L60-dup_all-late": (7, 4, 60, _DUP7["base"], _DUP7["keys"], hostile_lists(_DUP7), 0xF, 0x1,
                               ("skipped_dup", "short", "hold2")),
    # with pairwise distinct rows the pool fills R before it comes to the extra list:
    # duplicated rows, a reordering traitor and a non-target honest lieutenant to relay its packet
    "n7-d4-L60-dup3-reorder-lowest": (7, 4, 60, _DUP3["base"], _DUP3["keys"], hostile_lists(_DUP3), 0x2, 0x201,
                                      ("extra", "skipped_dup")),
}
# every event the issue lists has a set
EVENTS = ("padded_accepted", "padded_relayed", "short", "skipped_dup", "extra", "hold2", "broken")


def coal_rows(mc, name, coalition, adversary=None, counts=None):
    """run_host (or, with ``counts``, curve_host) of a set of SETS under a coalition word."""
    n, nd, sizeL, base, inst, lists, k = SETS[name]
    kw = {"flip_q16": k} if k else {}
    if adversary is not None:
        kw["adversary"] = adversary
    if counts is not None:
        return mc.curve_host(n, counts, nd, inst, base, HostEngine(), lists=lists, coalition=coalition, **kw)
    return mc.run_host(n, sizeL, nd, inst, base, HostEngine(), lists=lists, coalition=coalition, **kw)


def reach_rows(mc, name, counts=None, party_cls=None):
    n, nd, sizeL, base, inst, lists, adv, coal, _ = REACH[name]
    if counts is not None:
        return mc.curve_host(n, counts, nd, inst, base, HostEngine(), lists=lists, adversary=adv, coalition=coal)
    return mc.run_host(n, sizeL, nd, inst, base, HostEngine(), lists=lists, adversary=adv, coalition=coal,
                       party_cls=party_cls)


COUNTED = ("held", "hold2", "delivered", "padded", "short", "skipped", "skipped_dup", "extra", "padded_consistent",
           "padded_accepted", "padded_relayed")
_LOCK = threading.Lock()  # the ranks of a run are threads


def observing(mc, events):
    """A CoalitionParty subclass for run_host's party_cls seam that counts into
    ``events`` what the colluding parties of all instances do: packets held,
    hold lists that reach two packets, sends of a delivery and of a padded one,
    deliveries the pool left short, pool rows of another rank skipped as
    present (any, and those whose rep is a lower duplicate row), uses of the
    commander's extra list, and padded packets a receiver found consistent,
    took into V_i, and relayed on.  The pool walk is restated here and held to
    the model's result."""
    events.update(dict.fromkeys(COUNTED, 0))

    def count(what, by=1):
        with _LOCK:
            events[what] += int(by)

    class Observed(mc.CoalitionParty):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self._delivering, self._padded = False, False
            self.run_shared.__dict__.setdefault("noted", set())  # (dest, u, v, L) of the padded deliveries

        def lieu_broadcast(self, P, v, L):
            before = len(self.hold)
            super().lieu_broadcast(P, v, L)
            if len(self.hold) > before:
                count("held")
                count("hold2", len(self.hold) == 2)

        def pad(self, P, v, L):
            before, have = set(L), set(L)
            if P.u is not None and () not in L:
                for g, d in self.pool(P.u, v):
                    if len(have) >= self.delivery_round():
                        break
                    if d in have:
                        count("skipped", g != self.rank)
                        count("skipped_dup", g != self.rank and d[1] != g)
                        continue
                    have.add(d)
                    count("extra", g == 1)
                count("short", len(have) < self.delivery_round())
            super().pad(P, v, L)
            assert L == have
            self._padded = L != before

        def deliver(self):
            self._delivering = True
            super().deliver()
            self._delivering = False

        def send(self, dest, P, v, L):
            if self._delivering:
                count("delivered")
                if self._padded:
                    count("padded")
                    self.run_shared.noted.add((dest, P.u, int(v), frozenset(L)))
            super().send(dest, P, v, L)

        def lieu_receive(self, P, v, L, rnd, pre=None):
            noted = rnd == self.delivery_round() and (self.rank, P.u, int(v), frozenset(L)) in self.run_shared.noted
            known, sent, ok = len(self.Vi), self.stats.sent, self.stats.accept
            super().lieu_receive(P, v, L, rnd, pre)
            if noted:
                count("padded_consistent", self.stats.accept > ok)
                count("padded_accepted", len(self.Vi) > known)
                count("padded_relayed", self.stats.sent > sent)

    return Observed


def test_builder_presets_and_checks():
    mc = sub("montecarlo")
    assert mc.coalition() == LATE and mc.coalition(when=1) == 0x11 and mc.coalition(targets=2) == 0x201
    assert mc.coalition(targets=1, starve=True) == 0x1101
    assert {k: mc.COALITIONS[k] for k in COALITIONS} == COALITIONS
    for word in list(WORDS.values()) + [0, 0x1331 & ~0x220]:
        assert mc.check_coalition(word) == word
    assert mc.parse_coalition("late_one") == 0x201 and mc.parse_coalition("0x1101") == 0x1101
    assert mc.parse_coalition(17) == 17
    for bad, field in list(BAD_COAL.items()) + [(-1, "reserved"), (1 << 32, "reserved")]:
        with pytest.raises(mc.QbaError, match=field):
            mc.check_coalition(bad)
        with pytest.raises(mc.QbaError):
            mc.run_host(3, 4, 1, 1, 0, OracleEngine(), coalition=bad)
        with pytest.raises(mc.QbaError):
            mc.curve_host(3, [4], 1, 1, 0, OracleEngine(), coalition=bad)
        with pytest.raises(mc.QbaError):
            sub("engine").Engine._check_coalition(bad)
    for kw in ({"when": 2}, {"targets": 3}):
        with pytest.raises(mc.QbaError):
            mc.coalition(**kw)
    with pytest.raises(mc.QbaError):
        mc.parse_coalition("nobody")
    eng = sub("engine").Engine
    assert eng._check_coalition(None) == 0 and eng._check_coalition(0x11) == 0x11
    for f in (mc.run, mc.curve):  # refused before the engine is touched
        with pytest.raises(mc.QbaError):
            f(3, 8 if f is mc.run else [8], 1, 4, 0, None, coalition=0x10)
    with pytest.raises(ValueError):
        mc.run(3, 8, 1, 4, 0, None, path="tables", coalition=LATE)
    with pytest.raises(ValueError):
        mc.curve(3, [8], 1, 4, 0, None, coalition=LATE, explain=4, failures=4)


def test_outside_run_host_nobody_colludes():
    """A class of coalition_party used without run_host's per-run object: the
    rows of the adversary path, also under starve and a dishonest commander."""
    mc = sub("montecarlo")
    for coal in (0x1001, 0x1101, 0x11):
        rows = mc.run_host(7, 8, 3, 12, 0xAD0, OracleEngine(), party_cls=mc.coalition_party(0xF, coal))
        assert np.array_equal(rows, mc.run_host(7, 8, 3, 12, 0xAD0, OracleEngine(), adversary=0xF))
        assert ((rows[:, 1] >> 1) & 1).any()  # a dishonest commander among them


def _calls(lib):
    counts = (C.c_uint32 * 2)(5, 60)
    return {
        "sampled": lambda flip, a, c, cs=counts: lib.qba_montecarlo_curve_sampled_coal(None, 7, 2, 0, 4, cs, 2, flip,
                                                                                       None, None, a, c),
        "lists": lambda flip, a, c, cs=counts: lib.qba_montecarlo_curve_lists_coal(None, 7, 2, 0, 4, cs, 2, None, 64,
                                                                                   8 * 64, None, None, a, c),
    }


def test_symbols_are_exported_and_the_word_is_checked_after_adv_and_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    for name in ("qba_montecarlo_curve_sampled_coal", "qba_montecarlo_curve_lists_coal", "qba_montecarlo_coal_shape"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES
    err = lambda: lib.qba_last_error().decode()
    for name, f in _calls(lib).items():
        for bad, field in BAD_COAL.items():
            assert f(0, 0xF, bad) == lib_mod.QBA_EINVAL, (name, hex(bad))
            assert ": coal" in err() and field in err(), (name, hex(bad), err())
        for ok in [0] + list(WORDS.values()):  # only the device is missing
            assert f(0, 0xF, ok) == lib_mod.QBA_EINVAL and "ctx is NULL" in err(), (name, hex(ok), err())
        for bad_adv in BAD_WORDS:  # adv is looked at first
            assert f(0, bad_adv, 0x10) == lib_mod.QBA_EINVAL and ": adv" in err(), (name, err())
    # the rejection order of the other arguments is that of the _adv curve calls
    sampled = _calls(lib)["sampled"]
    assert sampled(65536, 0, 0x10) == lib_mod.QBA_EINVAL and "flip_q16" in err()
    down = (C.c_uint32 * 2)(60, 5)
    for f in _calls(lib).values():
        assert f(65536, 0, 0x10, down) == lib_mod.QBA_EINVAL and "counts" in err()
    assert lib.qba_montecarlo_curve_sampled_coal(None, 16, 2, 0, 4, down, 2, 65536, None, None, 0, 0x10) == \
        lib_mod.QBA_EINVAL and "n_parties" in err()
    assert lib.qba_montecarlo_curve_lists_coal(None, 7, 8, 0, 4, down, 2, None, 64, 512, None, None, 0, 0x10) == \
        lib_mod.QBA_EINVAL and "n_dishonest" in err()


@pytest.mark.parametrize("name", ["n3-d2-L8", "n7-d2-L8"])
def test_no_coalition_gives_the_adversary_rows(name):
    """coal = 0 and coalition=None against curve_host(..., adversary=), every
    word, under the reference policy and reorder_low."""
    mc = sub("montecarlo")
    sizeL = SETS[name][2]
    cps = [sizeL // 2, sizeL]
    for adv in (None, 0xF, PRESETS["reorder_low"]):
        want = host_rows(mc, name, adv, counts=cps)
        assert np.array_equal(coal_rows(mc, name, 0, adv, counts=cps), want)
        assert np.array_equal(coal_rows(mc, name, None, adv, counts=cps), want)
        assert np.array_equal(coal_rows(mc, name, 0, adv), want[1])


@pytest.fixture(scope="module")
def plain_rows():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = host_rows(sub("montecarlo"), name)
            memo[name].setflags(write=False)
        return memo[name]
    return get


@pytest.mark.parametrize("name", COAL_SETS)
def test_every_field_shows_on_the_recorded_sets(plain_rows, name):
    """Sensitivity: under `late` and under every word one field away from it,
    the host rows of the set differ from the no-coalition rows, and the word
    one field away differs from `late` somewhere on the sets taken together
    (test_every_field_differs_from_late_somewhere)."""
    mc = sub("montecarlo")
    ref = plain_rows(name)
    for what, word in {"late": LATE, **FIELDS}.items():
        rows = coal_rows(mc, name, word)
        assert not rows[:, 3].any()
        differ = int((rows != ref).any(axis=1).sum())
        print(f"{name} {what}: {differ} of {len(ref)} instances differ from no coalition")
        assert differ >= 1, (name, what)


def test_every_field_differs_from_late_somewhere():
    """... and every word one field away also differs from `late` itself on one
    of two sets (n7-d6-L3 has one honest lieutenant at most: every choice of
    targets is the same there)."""
    mc = sub("montecarlo")
    total = dict.fromkeys(FIELDS, 0)
    for name in ("n7-d2-L8", "n7-d6-L3"):
        late = coal_rows(mc, name, LATE)
        for what, word in FIELDS.items():
            differ = int((coal_rows(mc, name, word) != late).any(axis=1).sum())
            print(f"{name} {what}: {differ} instances differ from late")
            total[what] += differ
    assert all(total.values()), total


# (policy, words per ordinary destination)
ONE_ACTION = [(0x10, 1), (0x01, 2), (0x102, 1), (0x202, 2)]


@pytest.mark.parametrize("coal", [0x1, 0x11, 0x201], ids=["late", "when1", "lowest"])
@pytest.mark.parametrize("word,per", ONE_ACTION, ids=[f"{w:#x}" for w, _ in ONE_ACTION])
def test_a_colluding_traitor_draws_for_ordinary_destinations_only(word, per, coal):
    """Through the party_cls and rng_factory seams: per broadcast a colluding
    lieutenant draws nothing for a dishonest destination or a held one, and
    the policy's words for every other; an honest one draws nothing."""
    mc = sub("montecarlo")
    n, nd, sizeL, inst = 7, 3, 16, 24
    parties, seen = [], {"dishonest": 0, "held": 0, "ordinary": 0}

    class Counting(mc.coalition_party(word, coal)):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.want = 0
            parties.append(self)

        def lieu_broadcast(self, P, v, L):
            if self.dishonest:
                dis, targets = self.run_shared.dishonest(), self.targets()
                early = self._acc_rnd < self.delivery_round() - 1
                for dest in range(2, n + 1):
                    kind = None if dest == self.rank else "dishonest" if dest in dis else \
                        "held" if early and dest in targets else "ordinary"
                    if kind:
                        seen[kind] += 1
                    self.want += per * (kind == "ordinary")
            super().lieu_broadcast(P, v, L)

    rows = mc.run_host(n, sizeL, nd, inst, 0xAD0, OracleEngine(), party_cls=Counting,
                       rng_factory=lambda key, rank: mc.ProtocolRng(key, rank), adversary=word, coalition=coal)
    assert np.array_equal(rows, mc.run_host(n, sizeL, nd, inst, 0xAD0, OracleEngine(), adversary=word, coalition=coal))
    for p in parties:
        if p.rank >= 2:
            assert p.rng.t == p.want, (p.rank, p.dishonest, p.rng.t, p.want)
    # with every honest lieutenant a target nothing new reaches a traitor late enough to be sent on at
    # once; with one target the other honest lieutenants are ordinary destinations from epoch 0 on
    assert len(parties) == inst * (n + 1) and seen["dishonest"] and seen["held"], seen
    assert seen["ordinary"] or (coal >> 8) & 3 == 0, seen


@pytest.fixture(scope="module")
def reached():
    """name -> (rows, what observing() counted over the set's instances, no-coalition rows)"""
    memo = {}

    def get(name):
        if name not in memo:
            mc = sub("montecarlo")
            n, nd, sizeL, base, inst, lists, adv, coal, _ = REACH[name]
            ev = {}
            rows = reach_rows(mc, name, party_cls=observing(mc, ev))
            assert np.array_equal(rows, reach_rows(mc, name))  # observing changes nothing
            plain = mc.run_host(n, sizeL, nd, inst, base, HostEngine(), lists=lists, adversary=adv)
            ev["broken"] = int(((plain[:, 0] == 1) & (rows[:, 0] == 0)).sum())
            assert not rows[:, 3].any()
            memo[name] = (rows, ev, plain)
        return memo[name]
    return get


@pytest.mark.parametrize("name", list(REACH))
def test_reach_sets_show_the_events_they_were_chosen_for(reached, name):
    """Counted on the host model alone: no comparison of a kernel with the
    model on these sets can pass by never reaching the event."""
    rows, ev, plain = reached(name)
    print(name, ev)
    for event in REACH[name][8]:
        assert ev[event] > 0, (name, event, ev)
    assert ev["held"] > 0 and ev["delivered"] > 0 and (rows != plain).any()


def test_every_listed_event_is_reached_by_some_set(reached):
    """A padded packet accepted in round R; one accepted under when = 1 and
    relayed on; a delivery the pool could not fill; a pool row skipped because
    a duplicated row put its rep into the mask already; the commander's extra
    list used; a hold list of two packets; a run that succeeds without the
    coalition and fails with it."""
    total = {e: sum(reached(name)[1][e] for name in REACH) for e in EVENTS}
    print(total)
    for event in EVENTS:
        assert total[event] > 0, event
    relayed = [name for name in REACH if (REACH[name][7] >> 4) & 3 == 1 and reached(name)[1]["padded_relayed"]]
    assert relayed  # ... under when = 1


def test_coalition_kernels_use_no_scratch_no_static_lds_and_at_most_128_vgprs():
    lib = sub("_lib").lib()
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    new = {k: v for k, v in kds.items() if "qba_k_mc_coal_" in k}
    assert sum("19qba_k_mc_coal_listsE" in k for k in new) == 1
    for n in range(1, 16):
        kernel = f"_Z21qba_k_mc_coal_sampledILi{n}E"
        assert sum(k.startswith(kernel) for k in new) == (3 if n <= 11 else 2), n
        waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
        assert lib.qba_montecarlo_coal_shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
        samp = 2 if n <= 11 else 1
        assert any(k.startswith(f"{kernel}Li{samp}ELi{waves.value}E") for k in new), (n, waves.value)
        g, w = n + 1, 1 << n.bit_length()
        per_wave = 2064 + (2 * g * (g * w + 1) + 3) // 4 * 16 + (2 * w * g + 2 + 3) // 4 * 16 + (g * w + 3) // 4 * 16
        assert 1 <= waves.value <= 16 and wgs.value >= 1 and wgs.value * lds.value <= 160 * 1024
        assert waves.value * wgs.value <= 16
        assert lds.value >= waves.value * per_wave and (lds.value - waves.value * per_wave) % 16 == 0, n
    assert len(new) == 1 + 11 * 3 + 4 * 2  # only curve forms; one instantiation serves flip = 0 and flip > 0
    for k, v in new.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= 128, (k, v)
        assert not any(s in k for s in ("qba_k_protocol", "qba_k_mc_curve_", "qba_k_mc_lists", "qba_k_mc_sweep", "_adv"))
    assert lib.qba_montecarlo_coal_shape(16, None, None, None) == sub("_lib").QBA_EINVAL
    assert lib.qba_montecarlo_coal_shape(0, None, None, None) == sub("_lib").QBA_EINVAL


def test_cli_takes_collude_and_refuses_it_where_it_is_not_built():
    tfg = sub("tfg")
    a = tfg._args(["8", "2", "--parties", "7", "--runs", "16", "--collude", "late_one", "--curve", "3,8", "--flip", "9",
                   "--adversary", "strip", "--tally", "--failures", "2"])
    assert a.collude == 0x201 and a.fused and a.adversary == PRESETS["strip"]
    assert tfg._args(["8", "2", "--runs", "16", "--collude", "0x11"]).collude == 0x11
    for bad in (["--collude", "late"], ["--runs", "4", "--collude", "0x10"], ["--runs", "4", "--collude", "nobody"],
                ["--runs", "4", "--collude", "late", "--sweep", "1,2"],
                ["--runs", "4", "--collude", "late", "--explain", "2"],
                ["--runs", "4", "--collude", "late", "--tables"]):
        with pytest.raises(SystemExit):
            tfg._args(["8", "1"] + bad)
