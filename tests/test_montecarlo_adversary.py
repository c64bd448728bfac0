"""Adversary policies without a GPU: the host model
montecarlo.AdversaryParty at the reference word against the unchanged path, the
input sets on which every policy field shows in the rows (shared with
tests/test_gpu_montecarlo_adversary.py, which holds the _adv kernels to the host
model on them), the stream words a traitor consumes, the word's checks from
Python and through the C entry points, and the static resources of the _adv
kernels read from the cross-compiled library.

Small sizeL leaves most P_u empty, so honest receivers accept mutated packets
(EMPTY descriptors) and a traitor's choice shows in the rows."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
from conftest import sub
from kd_util import kernel_descriptors
from montecarlo_cases import HOSTILE, hostile_lists
from oracle_engine import OracleEngine


REFERENCE = 0xF
# one policy field at a time away from the reference: name -> word
# (acts [0:5), order [8:10), fresh [12], comm [16])
POLICIES = {
    "acts0": 0x01, "acts1": 0x02, "acts2": 0x04, "acts3": 0x08, "acts4": 0x10,
    "order1": 0x102, "order2": 0x202,
    "fresh": 0x100F, "comm": 0x1000F,
}
PRESETS = {"reference": 0xF, "relay": 0x10, "reorder_low": 0x11102, "mute": 0x01, "strip": 0x100C}

KEYS, BASE, NOISE_K = 24, 0xAD0, 0x1000
_HOSTILE7 = next(c for c in HOSTILE if c["name"] == "n7-d4-L60-dup_all")

# name -> (n, n_dishonest, sizeL, seed_base, instances, injected lists or None, flip_q16)
SETS = {
    "n3-d2-L8": (3, 2, 8, BASE, KEYS, None, 0),
    "n7-d2-L8": (7, 2, 8, BASE, KEYS, None, 0),
    "n7-d6-L3": (7, 6, 3, BASE, KEYS, None, 0),
    "n7-d2-L8-noisy": (7, 2, 8, BASE, KEYS, None, NOISE_K),
    "n7-d4-L60-dup_all": (7, 4, 60, _HOSTILE7["base"], _HOSTILE7["keys"], hostile_lists(_HOSTILE7), 0),
    "n11-d3-L8": (11, 3, 8, BASE, KEYS, None, 0),
}
# Which set serves which field, recorded from the host model
# (test_every_policy_field_shows_on_its_recorded_sets asserts it).  n = 3 has
# two lieutenants: one destination per broadcast and dest 2 / dest 3 on either
# side of both commander splits, so `fresh` and `comm` cannot show there.
EVERY = tuple(POLICIES)
SERVES = {
    "n3-d2-L8": ("acts0", "acts1", "acts2", "acts3", "acts4", "order1", "order2"),
    "n7-d2-L8": EVERY,
    "n7-d6-L3": EVERY,
    "n7-d2-L8-noisy": EVERY,
    "n7-d4-L60-dup_all": EVERY,
    "n11-d3-L8": EVERY,
}

BAD_WORDS = [0x0, 0x100, 0x30F, 0x302, 0x2F, 0x4F, 0x8F, 0x40F, 0x80F, 0x200F, 0x800F, 0x2000F, 0x10000F, 0x8000000F]

_DUMMY = {"nfac": 0, "desc": np.zeros((0, 6), np.int32), "pat": np.zeros(1, np.uint64),
          "apat": np.zeros(1, np.uint64), "thr": np.zeros(1, np.uint64)}


class HostEngine(OracleEngine):
    """The numpy engine with the C twin's closed-form sampler (n <= 11), which
    run_host needs to noise the lists an instance would have sampled."""

    def sample(self, n, key, first, count):
        return oracle_lib.sample(n, key & ((1 << 64) - 1), first, count, _DUMMY, _DUMMY, True)


def host_rows(mc, name, adversary=None, counts=None):
    """run_host (or, with ``counts``, curve_host) of a set under a policy."""
    n, nd, sizeL, base, inst, lists, k = SETS[name]
    kw = {"flip_q16": k} if k else {}
    if adversary is not None:
        kw["adversary"] = adversary
    if counts is not None:
        return mc.curve_host(n, counts, nd, inst, base, HostEngine(), lists=lists, **kw)
    return mc.run_host(n, sizeL, nd, inst, base, HostEngine(), lists=lists, **kw)


@pytest.fixture(scope="module")
def reference_rows():
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = host_rows(sub("montecarlo"), name)
            memo[name].setflags(write=False)
        return memo[name]
    return get


def test_builder_presets_and_checks():
    mc = sub("montecarlo")
    assert mc.adversary() == REFERENCE == mc.ADV_REFERENCE
    assert mc.adversary(acts=0xF) == 0xF and mc.adversary(acts=[4]) == 0x10
    assert mc.adversary([1], order=1, fresh=True, comm=True) == 0x11102
    assert {k: mc.ADVERSARIES[k] for k in PRESETS} == PRESETS
    for name, word in POLICIES.items():
        assert mc.check_adversary(word) == word, name
    assert mc.parse_adversary("strip") == 0x100C and mc.parse_adversary("0x11102") == 0x11102
    assert mc.parse_adversary(15) == 15
    for bad in BAD_WORDS + [-1, 1 << 32]:
        with pytest.raises(mc.QbaError):
            mc.check_adversary(bad)
        with pytest.raises(mc.QbaError):
            mc.run_host(3, 4, 1, 1, 0, OracleEngine(), adversary=bad)
        with pytest.raises(mc.QbaError):
            mc.curve_host(3, [4], 1, 1, 0, OracleEngine(), adversary=bad)
    for kw in ({"acts": []}, {"acts": [5]}, {"acts": 32}, {"order": 3}):
        with pytest.raises(mc.QbaError):
            mc.adversary(**kw)
    with pytest.raises(mc.QbaError):
        mc.parse_adversary("nobody")
    eng = sub("engine").Engine
    for bad in BAD_WORDS:  # refused before the engine is touched
        with pytest.raises(mc.QbaError):
            eng._check_adversary(bad)
    assert eng._check_adversary(None) is None and eng._check_adversary(0x10) == 0x10


@pytest.mark.parametrize("n,nd", [(3, 1), (7, 2)])
def test_reference_word_gives_the_default_rows(n, nd):
    """adversary=0xF against the unchanged path: every word of 67 instances at
    sizeL 8, single count and curve."""
    mc = sub("montecarlo")
    eng, base = OracleEngine(), 0x5EED0
    want = mc.run_host(n, 8, nd, 67, base, eng)
    assert np.array_equal(mc.run_host(n, 8, nd, 67, base, eng, adversary=0xF), want)
    assert 0 < want[:, 0].sum() and np.count_nonzero(want[:, 1]) == 67
    wantc = mc.curve_host(n, [3, 8], nd, 16, base, eng)
    assert np.array_equal(mc.curve_host(n, [3, 8], nd, 16, base, eng, adversary=0xF), wantc)
    assert np.array_equal(wantc[1], want[:16])


def test_reference_word_gives_the_default_rows_on_a_hostile_set(reference_rows):
    mc = sub("montecarlo")
    name = "n7-d4-L60-dup_all"
    assert np.array_equal(host_rows(mc, name, REFERENCE), reference_rows(name))
    assert np.array_equal(host_rows(mc, name, REFERENCE, counts=[7, 60])[1], reference_rows(name))
    noisy = "n7-d2-L8-noisy"
    assert np.array_equal(host_rows(mc, noisy, REFERENCE), reference_rows(noisy))


@pytest.mark.parametrize("name", list(SETS))
def test_every_policy_field_shows_on_its_recorded_sets(reference_rows, name):
    """Sensitivity: with one field away from the reference, the host rows of
    the set differ from the reference-policy rows in at least one instance --
    so no comparison of a kernel with the host model on these sets is vacuous."""
    mc = sub("montecarlo")
    ref = reference_rows(name)
    assert not ref[:, 3].any()
    for policy in SERVES[name]:
        rows = host_rows(mc, name, POLICIES[policy])
        assert not rows[:, 3].any()
        differ = int((rows != ref).any(axis=1).sum())
        print(f"{name} {policy}: {differ} of {len(ref)} instances differ")
        assert differ >= 1, (name, policy)


def test_every_field_is_served_by_a_set_of_every_n_it_can_show_at():
    for policy in POLICIES:
        ns = {SETS[s][0] for s, served in SERVES.items() if policy in served}
        assert ns >= {7, 11} and (ns >= {3} or policy in ("fresh", "comm")), policy
    kinds = {(SETS[s][5] is not None, SETS[s][6] != 0) for s in SETS}
    assert kinds == {(False, False), (True, False), (False, True)}  # sampled, hostile, noisy


def test_presets_differ_from_the_reference_where_they_should(reference_rows):
    mc = sub("montecarlo")
    name = "n7-d2-L8"
    ref = reference_rows(name)
    rows = {p: host_rows(mc, name, w) for p, w in PRESETS.items()}
    assert np.array_equal(rows["reference"], ref)
    for p in ("relay", "reorder_low", "mute", "strip"):
        assert (rows[p] != ref).any(), p
    # a traitor who relays unchanged is an honest party that is not counted: every run agrees
    # unless the commander is the traitor
    relay = rows["relay"]
    cmd_honest = ((relay[:, 1] >> 1) & 1) == 0
    assert relay[cmd_honest, 0].all()


# (policy, extra words per destination beyond the action draw)
ONE_ACTION = [(0x01, 1), (0x02, 1), (0x202, 1), (0x102, 0), (0x04, 0), (0x08, 0), (0x10, 0), (0x1010, 0), (0x1102, 0)]


@pytest.mark.parametrize("word,extra", ONE_ACTION, ids=[f"{w:#x}" for w, _ in ONE_ACTION])
def test_a_traitor_with_one_action_consumes_exact_stream_words(word, extra):
    """Through the rng_factory and party_cls seams: a dishonest lieutenant
    draws one word per destination for the action (randint(1) accepts its first
    word), one more for action 0 and for order 0 or 2, none for order 1; an
    honest one draws nothing."""
    mc = sub("montecarlo")
    n, nd, sizeL, inst = 7, 3, 8, 6
    parties, calls = [], {}

    class Counting(mc.adversary_party(word)):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            parties.append(self)

        def lieu_broadcast(self, P, v, L):
            calls[id(self)] = calls.get(id(self), 0) + 1
            super().lieu_broadcast(P, v, L)

    rows = mc.run_host(n, sizeL, nd, inst, BASE, OracleEngine(), party_cls=Counting,
                       rng_factory=lambda key, rank: mc.ProtocolRng(key, rank))
    assert np.array_equal(rows, mc.run_host(n, sizeL, nd, inst, BASE, OracleEngine(), adversary=word))
    seen = 0
    for p in parties:
        if p.rank < 2:
            continue
        b = calls.get(id(p), 0)
        want = b * (n - 2) * (1 + extra) if p.dishonest else 0
        assert p.rng.t == want, (p.rank, p.dishonest, b, p.rng.t)
        seen += b if p.dishonest else 0
    assert len(parties) == inst * (n + 1) and seen > 0


def test_reference_word_consumes_the_reference_stream():
    """Word for word: every rank's stream position after a run under 0xF is
    that of the unchanged parties."""
    mc = sub("montecarlo")

    def positions(**kw):
        rngs = []

        def make(key, rank):
            rngs.append(mc.ProtocolRng(key, rank))
            return rngs[-1]
        rows = mc.run_host(7, 8, 3, 8, BASE, OracleEngine(), rng_factory=make, **kw)
        return rows, [(r.key, r.rank, r.t) for r in rngs]
    a, b = positions(), positions(adversary=0xF)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and any(t for _, _, t in a[1])


SYMBOLS = ("qba_protocol_batched_adv", "qba_montecarlo_lists_adv", "qba_montecarlo_curve_lists_adv",
           "qba_montecarlo_sampled_adv", "qba_montecarlo_curve_sampled_adv")


def test_symbols_are_exported_and_the_word_is_checked_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES
    counts = (C.c_uint32 * 2)(5, 60)
    calls = {
        "tables": lambda a: lib.qba_protocol_batched_adv(None, 7, 2, 0, 4, None, None, None, None, None, a),
        "lists": lambda a: lib.qba_montecarlo_lists_adv(None, 7, 2, 0, 4, 60, None, 64, 8 * 64, None, None, a),
        "curve_lists": lambda a: lib.qba_montecarlo_curve_lists_adv(None, 7, 2, 0, 4, counts, 2, None, 64, 8 * 64,
                                                                    None, None, a),
        "sampled": lambda a: lib.qba_montecarlo_sampled_adv(None, 7, 2, 0, 4, 60, 0x1000, None, None, a),
        "curve_sampled": lambda a: lib.qba_montecarlo_curve_sampled_adv(None, 7, 2, 0, 4, counts, 2, 0, None, None, a),
    }
    for name, f in calls.items():
        for bad in BAD_WORDS:
            assert f(bad) == lib_mod.QBA_EINVAL, (name, hex(bad))
            assert "adv" in lib.qba_last_error().decode(), (name, hex(bad))
        for ok in list(POLICIES.values()) + list(PRESETS.values()):  # only the device is missing
            assert f(ok) == lib_mod.QBA_EINVAL, (name, hex(ok))
            assert "ctx is NULL" in lib.qba_last_error().decode(), (name, hex(ok))
    # the rejection order of the existing arguments is kept: n, n_dishonest, count(s), flip_q16, then the word
    assert lib.qba_montecarlo_sampled_adv(None, 16, 2, 0, 4, 60, 0, None, None, 0) == lib_mod.QBA_EINVAL
    assert "n_parties" in lib.qba_last_error().decode()
    assert lib.qba_montecarlo_lists_adv(None, 7, 8, 0, 4, 60, None, 64, 512, None, None, 0) == lib_mod.QBA_EINVAL
    assert "n_dishonest" in lib.qba_last_error().decode()
    assert lib.qba_montecarlo_sampled_adv(None, 7, 2, 0, 4, 1 << 31, 65536, None, None, 0) == lib_mod.QBA_EINVAL
    assert "count" in lib.qba_last_error().decode()
    assert lib.qba_montecarlo_sampled_adv(None, 7, 2, 0, 4, 60, 65536, None, None, 0) == lib_mod.QBA_EINVAL
    assert "flip_q16" in lib.qba_last_error().decode()
    down = (C.c_uint32 * 2)(60, 5)
    assert lib.qba_montecarlo_curve_lists_adv(None, 7, 2, 0, 4, down, 2, None, 64, 512, None, None, 0) == \
        lib_mod.QBA_EINVAL
    assert "counts" in lib.qba_last_error().decode()


def test_adv_kernels_use_no_scratch_no_static_lds_and_at_most_128_vgprs():
    lib = sub("_lib").lib()
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    adv = {k: v for k, v in kds.items() if "qba_k_" in k and "_adv" in k}
    for name in ("qba_k_proto_adv", "qba_k_mc_lists_adv", "qba_k_mc_lists_curve_adv"):
        assert sum(f"{len(name)}{name}E" in k for k in adv) == 1, name
    for n in range(1, 16):
        samp = 2 if n <= 11 else 1
        for kernel, shape in ((f"_Z20qba_k_mc_sampled_advILi{n}E", lib.qba_montecarlo_shape),
                              (f"_Z26qba_k_mc_curve_sampled_advILi{n}E", lib.qba_montecarlo_curve_shape)):
            waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
            assert shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
            # all samplers of the n, the shipped one at the noiseless kernel's wave count
            assert sum(k.startswith(kernel) for k in adv) == (3 if n <= 11 else 2), (n, kernel)
            assert any(k.startswith(f"{kernel}Li{samp}ELi{waves.value}E") for k in adv), (n, kernel)
    assert len(adv) == 3 + 2 * (11 * 3 + 4 * 2)  # one instantiation serves flip = 0 and flip > 0
    for k, v in adv.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= 128, (k, v)
    # the kernels that were there stay findable by the names the sibling tests use
    assert sum("qba_k_protocol" in k for k in kds) == 1
    assert sum("qba_k_mc_curve_lists" in k for k in kds) == 1
