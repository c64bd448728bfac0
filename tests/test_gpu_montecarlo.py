"""qba_protocol_batched on the GPU: the kernel's result rows equal the host
reference (montecarlo.run_host: CountParty under run_local on the same
counter-based RNG) in every field of every instance."""
import json

import numpy as np
import pytest

from conftest import GOLDEN, sub
from montecarlo_cases import (CASES, HOSTILE, HOSTILE_IDS, IDS, INJECT_BASE, INJECT_KEYS, SWEEP, SWEEP_IDS,
                              hostile_lists)
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

GOLDEN_CASES = json.loads((GOLDEN / "protocol.json").read_text())
GOLDEN_LISTS = np.load(GOLDEN / "protocol_lists.npz")
FIELDS = ["success", "dishonest", "empty_vi", "status"]


def _assert_rows(got, want, n):
    assert got.shape == want.shape and got.dtype == np.int32
    if not np.array_equal(got, want):
        i, j = np.argwhere(got != want)[0]
        name = FIELDS[j] if j < 4 else f"rank {(j - 4) // 5} " + \
            ["decision", "V", "accept", "reject", "sent"][(j - 4) % 5]
        raise AssertionError(f"instance {i}, {name}: kernel {got[i, j]} != host {want[i, j]}\n"
                             f"kernel {got[i].tolist()}\nhost   {want[i].tolist()}")
    assert np.all(got[:, 3] == 0)


@pytest.fixture(scope="module")
def sampled(engine):
    """Per parameter set: the device tables, the kernel's rows and the host
    reference's rows, computed once."""
    import torch
    mc = sub("montecarlo")
    memo = {}

    def get(case):
        if case not in memo:
            n, nd, sizeL = case
            base, inst = CASES[case]
            lists, counts = engine.sample_check_batched(n, base, inst, sizeL)
            out = engine.protocol_batched(n, nd, base, counts)
            torch.cuda.synchronize()
            # the C twin samples n <= 11; above, the reference takes the device's own lists
            host_lists = None if n <= 11 else lists[:, :, :sizeL].cpu().numpy()
            want = mc.run_host(n, sizeL, nd, inst, base, OracleEngine(), lists=host_lists)
            want.setflags(write=False)
            memo[case] = (counts, out.cpu().numpy(), want)
        return memo[case]
    return get


@pytest.mark.parametrize("case", list(CASES), ids=IDS)
def test_kernel_equals_host_reference(sampled, case):
    _, got, want = sampled(case)
    _assert_rows(got, want, case[0])


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c["name"] for c in GOLDEN_CASES])
def test_injected_lists_equal_host_reference(engine, case):
    """Lists with Cond3 collisions (rejected commander packets, empty V_i):
    one table set replicated under 16 protocol keys."""
    import torch
    mc = sub("montecarlo")
    n, nd, sizeL = case["n"], case["nDishonest"], case["sizeL"]
    li = GOLDEN_LISTS[case["name"]]
    _, w = engine.sizes(n)
    g = n + 1
    flat = engine.count_tables(n, sizeL, lists=li, device_out=True)
    h, c = w * g * w, w * g * g
    rep = lambda t, *s: t.view(1, *s).expand(INJECT_KEYS, *s).contiguous()  # noqa: E731
    counts = sub("engine").Counts(rep(flat[:h], w, g, w), rep(flat[h:h + c], w, g, g), rep(flat[h + c:], w))
    got = engine.protocol_batched(n, nd, INJECT_BASE, counts)
    torch.cuda.synchronize()
    want = mc.run_host(n, sizeL, nd, INJECT_KEYS, INJECT_BASE, OracleEngine(),
                       lists=np.broadcast_to(li, (INJECT_KEYS,) + li.shape))
    _assert_rows(got.cpu().numpy(), want, n)


@pytest.fixture(scope="module")
def hostile(engine):
    """Per hostile set or sweep entry: the device tables under its keys, the
    kernel's rows and the host reference's rows, computed once."""
    import torch
    mc, Counts = sub("montecarlo"), sub("engine").Counts
    memo = {}

    def get(case):
        if case["name"] not in memo:
            n, nd, sizeL, keys = case["n"], case["nDishonest"], case["sizeL"], case["keys"]
            li = hostile_lists(case)
            _, w = engine.sizes(n)
            g = n + 1
            h, c = w * g * w, w * g * g
            # a hostile set: one list, its tables replicated under the keys; a sweep entry: a list per key
            distinct = 1 if li.strides[0] == 0 else keys
            flat = torch.stack([engine.count_tables(n, sizeL, lists=np.array(li[i]), device_out=True)
                                for i in range(distinct)]).expand(keys, -1)
            counts = Counts(flat[:, :h].reshape(keys, w, g, w).contiguous(),
                            flat[:, h:h + c].reshape(keys, w, g, g).contiguous(), flat[:, h + c:].contiguous())
            got = engine.protocol_batched(n, nd, case["base"], counts).cpu().numpy()
            want = mc.run_host(n, sizeL, nd, keys, case["base"], OracleEngine(), lists=li)
            for a in (got, want):
                a.setflags(write=False)
            memo[case["name"]] = (counts, got, want)
        return memo[case["name"]]
    return get


@pytest.mark.parametrize("case", HOSTILE + SWEEP, ids=HOSTILE_IDS + SWEEP_IDS)
def test_hostile_lists_equal_host_reference(hostile, case):
    """Lists with duplicated rows and many traitors (canonicalised descriptors,
    rep in {0, 1}, L of 8 descriptors, round 7, 6 packets in one mailbox, V_i
    of 10 values: test_montecarlo.test_hostile_sets_reach_every_path), and
    honest lists at every n from 1 to 15."""
    _, got, want = hostile(case)
    _assert_rows(got, want, case["n"])


WIDE = [c for c in HOSTILE if c["name"] in ("n3-d2-L30-dup_u", "n15-d14-L96-dup3")]  # w = 4 and w = 16


@pytest.mark.parametrize("shift", [32, 31])
@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_tables_are_read_as_64_bit_values(engine, hostile, case, shift):
    """The specification consults only != 0, == 0 and C == P, so tables scaled
    by 2^32 (low words all zero) or 2^31 (low word = the count's parity, in the
    sign bit) give the same rows."""
    Counts = sub("engine").Counts
    counts, got, want = hostile(case)
    big = Counts(counts.H * (1 << shift), counts.C * (1 << shift), counts.P * (1 << shift))
    assert int(big.P.max()) >= 1 << shift and int(big.C.max()) >= 1 << shift and int(big.H.max()) >= 1 << shift
    rows = engine.protocol_batched(case["n"], case["nDishonest"], case["base"], big).cpu().numpy()
    assert np.array_equal(rows, got)
    _assert_rows(rows, want, case["n"])


def test_out_is_overwritten_in_every_word_and_checked(engine, hostile):
    import torch
    QbaError, Counts = sub("_lib").QbaError, sub("engine").Counts
    case = next(c for c in HOSTILE if c["name"] == "n7-d4-L60-dup_all")
    n, nd, base, keys = case["n"], case["nDishonest"], case["base"], case["keys"]
    counts, got, _ = hostile(case)
    words = 4 + 5 * (n + 1)
    fill = 0x7F7F7F7F
    out = torch.full((keys, words), fill, dtype=torch.int32, device=engine.device)
    ret = engine.protocol_batched(n, nd, base, counts, out=out)
    assert ret.data_ptr() == out.data_ptr()
    rows = out.cpu().numpy()
    assert not np.any(rows == fill) and np.array_equal(rows, got)

    def run(c=counts, o=None):
        return engine.protocol_batched(n, nd, base, c, out=o)

    new = lambda *shape, dtype=torch.int32, device=engine.device: \
        torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
    for bad in (new(keys, words, dtype=torch.int64), new(keys, words, dtype=torch.float32),
                new(keys + 1, words), new(keys, words + 1), new(keys * words),
                new(keys, words, device="cpu"), new(keys, 2 * words)[:, ::2], new(words, keys).t()):
        with pytest.raises(QbaError):
            run(o=bad)
    H, C, P = counts.H, counts.C, counts.P
    assert H.transpose(1, 3).shape == H.shape and not H.transpose(1, 3).is_contiguous()
    for bad in (Counts(H.transpose(1, 3), C, P), Counts(H, C.transpose(2, 3), P),
                Counts(H, C, torch.stack([P, P], 2)[:, :, 0]),
                Counts(H.to(torch.int32), C, P), Counts(H, C.cpu(), P), Counts(H, C, P[:-1]),
                Counts(H[:, :, :, :-1].contiguous(), C, P)):
        with pytest.raises(QbaError):
            run(c=bad)
    assert np.array_equal(run().cpu().numpy(), got)  # and the engine still works


def test_streams_split_batches_and_single_instance(engine, sampled):
    import torch
    case = (7, 2, 200)
    n, nd, _ = case
    base, inst = CASES[case]
    counts, got, _ = sampled(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = engine.protocol_batched(n, nd, base, counts)
    side.synchronize()
    assert np.array_equal(again.cpu().numpy(), got)
    Counts = sub("engine").Counts
    half = inst // 2
    parts = [engine.protocol_batched(n, nd, base + a, Counts(counts.H[a:b], counts.C[a:b], counts.P[a:b]))
             for a, b in ((0, half), (half, inst))]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), got)
    k = 5
    one = engine.protocol_batched(n, nd, base + k, Counts(counts.H[k:k + 1], counts.C[k:k + 1], counts.P[k:k + 1]))
    assert np.array_equal(one.cpu().numpy(), got[k:k + 1])


def test_run_sums_its_batches(engine):
    mc = sub("montecarlo")
    n, nd, sizeL, seed = 7, 2, 200, 3000
    total = mc.run(n, sizeL, nd, 96, seed, engine, batch=32)
    rows = []
    for off in (0, 32, 64):
        _, counts = engine.sample_check_batched(n, seed + off, 32, sizeL, packed=True)
        rows.append(engine.protocol_batched(n, nd, seed + off, counts).cpu().numpy())
    parts = [mc.summarize(n, r) for r in rows]
    assert total["runs"] == 96 and total["successes"] == sum(p["successes"] for p in parts)
    assert total["empty_vi_runs"] == sum(p["empty_vi_runs"] for p in parts)
    assert total["rate"] == total["successes"] / 96
    hist = {}
    for p in parts:
        for v, c in p["decisions"].items():
            hist[v] = hist.get(v, 0) + c
    assert total["decisions"] == hist
    assert total == mc.summarize(n, np.concatenate(rows))
    # unpacked rows and one big batch: the same instances
    assert mc.run(n, sizeL, nd, 96, seed, engine, packed=False, batch=4096) == total


def test_engine_rejects_what_the_library_would(engine):
    QbaError = sub("_lib").QbaError
    _, counts = engine.sample_check_batched(3, 1, 2, 60)
    with pytest.raises(QbaError):
        engine.protocol_batched(3, 4, 1, counts)   # n_dishonest > n
    with pytest.raises(QbaError):
        engine.protocol_batched(4, 1, 1, counts)   # tables of another n
