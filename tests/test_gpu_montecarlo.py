"""qba_protocol_batched on the GPU: the kernel's result rows equal the host
reference (montecarlo.run_host: CountParty under run_local on the same
counter-based RNG) in every field of every instance."""
import json

import numpy as np
import pytest

from conftest import GOLDEN, sub
from montecarlo_cases import CASES, IDS, INJECT_BASE, INJECT_KEYS
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
