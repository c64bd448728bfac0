"""qba_resource_compile against the exact tableau reference
(oracle/stabilizer.py) on the generated circuit pairs of
tests/resource_circuits.py, n in {3, 7, 11, 12, 15} (N = 8 .. 64 qubits): random
registers interleaved over the groups, X on fixed qubits, H after CX, CX chains
and fan-outs, factor widths that do not merge, Q circuits under random
permutations and with registers beside the GHZ ones.  The reference runs the
whole gate list through one tableau and knows nothing of registers, pattern
bits, merges or the permutation mask.  Then the compiler's envelope, and the
sampler on four of the programs (a Q program past Philox block 0, the most
factors 64 qubits allow, three not-Q column words, a random n = 15 pair)
against the C twin, which had the words past block 0 already
(oracle/sampler_ref.c, stream_word).

Two cases of the envelope cannot be reached through qba_resource_compile (the
arithmetic is in tests/resource_circuits.py): a program of 16 factors and the
refusal of 17.  The most 64 qubits allow is 15, compiled and sampled here;
csrc/sanitize/plan_check.cpp holds qba_plan_program to 16 and 17 directly."""
import numpy as np
import pytest

import oracle_lib
import stabilizer as st
from conftest import sub
from montecarlo_programs import same_program
from resource_circuits import (FACTORS15, NS, PAIRS_PER_N, SAMPLED, WORDS3, chained_h, column_bits, column_words,
                               misplaced_x, n_qubits, pair, perm_mask, program_subspace, shipped_notq, shipped_q)

pytestmark = pytest.mark.gpu

COUNT, FIRSTS, SEED = 20_001, (0, (1 << 32) - 7), 0xC0DE5EED


@pytest.fixture(scope="module")
def eng():
    """An engine of its own: the session's keeps the shipped programs."""
    e = sub("engine").Engine(0)
    yield e
    e.close()


def _assert_shipped_n3_still_samples(eng):
    info = eng.prepare(3, perm=[1, 2, 3])
    assert info["closed"] and info["canonical"]
    want = oracle_lib.sample(3, SEED, 5, 2001, info["notq"], info["q"], info["closed"])
    assert np.array_equal(eng.sample(3, SEED, 5, 2001)[:, :2001].cpu().numpy(), want)


@pytest.mark.parametrize("n", NS)
def test_compiled_programs_equal_the_tableau_distribution(eng, n):
    big = (n + 1) * n_qubits(n)
    ghz = [eng.prepare(n, perm=list(range(1, n + 1)))["q"]]
    kinds = []
    for i in range(PAIRS_PER_N):
        notq, q, kind = pair(n, i)
        info = eng.compile(n, notq, q)
        assert program_subspace(info["notq"]) == st.distribution(notq.ops, big), (n, i, "not-Q")
        got = st.shifted(program_subspace(info["q"]), perm_mask(n, q.perm))
        assert got == st.distribution(q.ops, big), (n, i, "Q", kind)
        if kind == "ghz":
            ghz.append(info["q"])
        kinds.append(kind)
    # the permutation is the sampler's to draw: it must leave no trace in the program
    assert len(ghz) >= 5 and all(same_program(ghz[0], g) for g in ghz[1:])
    assert kinds.count("extended") >= 5


@pytest.mark.parametrize("n", NS)
def test_a_misplaced_x_is_refused(eng, n):
    lib = sub("_lib")
    rng = np.random.default_rng([0xBAD, n])
    for _ in range(4):
        bad = misplaced_x(n, rng, rng.permutation(n) + 1)
        with pytest.raises(lib.QbaError) as err:
            eng.compile(n, shipped_notq(n), bad)
        assert err.value.code == lib.QBA_EINVAL and "permutation mask" in str(err.value)
    _assert_shipped_n3_still_samples(eng)


def test_named_programs_have_the_layouts_they_are_named_for(eng):
    desc = {}
    for name, (n, i) in SAMPLED.items():
        notq, q, _ = pair(n, i)
        desc[name] = eng.compile(n, notq, q)
    f15, w3, qw = desc["factors15"]["notq"], desc["words3"]["notq"], desc["q_wide"]["q"]
    assert f15["nfac"] == 15 and f15["desc"][:, 0].tolist() == FACTORS15 and column_words(f15) == 3
    assert w3["nfac"] == len(WORDS3) and w3["desc"][:, 0].tolist() == WORDS3
    assert w3["desc"][:, 3].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert column_bits(qw) > 32 and column_words(qw) == 2 and qw["desc"][:, 0].tolist() == [8, 8, 8, 1, 8, 8]
    assert not any(d["closed"] or d["canonical"] for d in desc.values())


@pytest.mark.parametrize("m", [9, 17])
def test_a_register_past_256_outcomes_is_unsupported(eng, m):
    """9 chained H qubits: a support of 512.  17: 2^17, twice the 65,536 slots of
    the compiler's support buffer, so the compaction's cap guard is all that
    keeps the emit pass inside it."""
    lib = sub("_lib")
    n = 7
    notq = chained_h(n, m, np.random.default_rng([0xE, m]))
    with pytest.raises(lib.QbaError) as err:
        eng.compile(n, notq, shipped_q(n, range(1, n + 1)))
    assert err.value.code == lib.QBA_EUNSUPPORTED and f"{1 << m} outcomes" in str(err.value)
    _assert_shipped_n3_still_samples(eng)
    info = eng.prepare(n, perm=list(range(1, n + 1)))  # and n itself compiles again
    assert info["closed"]


@pytest.fixture(scope="module")
def sampled(eng):
    """name -> (info, {first: the C twin's lists and count tables}), each once."""
    memo = {}

    def get(name):
        if name not in memo:
            n, i = SAMPLED[name]
            notq, q, _ = pair(n, i)
            info = eng.compile(n, notq, q)
            refs = {}
            for first in FIRSTS:
                li = oracle_lib.sample(n, SEED, first, COUNT, info["notq"], info["q"], info["closed"])
                H, C, P, bad = oracle_lib.counts(li, n)
                assert bad == 0
                for a in (li, H, C, P):
                    a.setflags(write=False)
                refs[first] = (li, H, C, P)
            memo[name] = (info, refs)
        else:  # another named program of this n may have been compiled since
            n, i = SAMPLED[name]
            notq, q, _ = pair(n, i)
            assert same_program(eng.compile(n, notq, q)["q"], memo[name][0]["q"])
        return memo[name]
    return get


CELLS = [(name, first) for name in SAMPLED for first in FIRSTS]


@pytest.mark.parametrize("name,first", CELLS, ids=[f"{name}-{'0' if not first else 'past32'}" for name, first in CELLS])
def test_sampler_on_generated_programs_equals_the_c_twin(eng, sampled, name, first):
    import torch
    n = SAMPLED[name][0]
    info, refs = sampled(name)
    want, H, C, P = refs[first]
    assert not info["closed"] and 0 < int(P.sum()) < COUNT
    got = eng.sample(n, SEED, first, COUNT)[:, :COUNT].cpu().numpy()
    assert np.array_equal(got, want), f"sample: first difference at {np.argwhere(got != want)[:1].tolist()}"
    lists, c = eng.sample_check(n, SEED, first, COUNT)
    packed, cp = eng.sample_check_packed(n, SEED, first, COUNT)
    torch.cuda.synchronize()
    assert np.array_equal(lists[:, :COUNT].cpu().numpy(), want), "sample_check lists"
    assert np.array_equal(sub("engine").unpack_nibbles(packed.cpu().numpy(), COUNT), want), "packed lists"
    for what, cc in (("byte", c), ("packed", cp)):
        gH, gC, gP = cc.numpy()
        assert np.array_equal(gH, H) and np.array_equal(gC, C) and np.array_equal(gP, P), what
    assert eng.last_stats()[0] == 0
