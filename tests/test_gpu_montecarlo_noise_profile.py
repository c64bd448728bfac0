"""The noise-profile kernels on the GPU.  Every
comparison is exact, status included.  Both curve kernels must write the rows
of the host model (montecarlo.curve_host with ``noise=``) on a grid of shapes
under 20 profiles that rotate with the grid point; the all-zero and the uniform
profiles must write the rows of the _adv curve calls at that flip_q16 word for
word; noise_profile_apply must give montecarlo.noisy_lists_profile.  Up to
n = 11 the host model samples with the C twin; at n = 15, beyond its sampler,
the host model takes the device's own clean lists (the grid holds no n of 12
to 14)."""
import numpy as np
import pytest

from conftest import sub
from montecarlo_noise_profile_cases import (CASE_IDS, CASES, COUNTS, GRID, GRID_BASE, INST, MASK64, NS, POLICIES,
                                            PROFILES, _nds, policy_at, rates_of)
from test_gpu_montecarlo_adversary import _batched, _eq
from test_montecarlo_adversary import HostEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clean_lists(engine):
    """n -> (device lists [INST, n+1, >= 130], host copy [INST, n+1, 130]) of the
    clean entries of the grid's instances, sampled once and left unchanged."""
    memo = {}

    def get(n):
        if n not in memo:
            dev, _ = _batched(engine, n, GRID_BASE, INST, COUNTS[-1])
            host = np.ascontiguousarray(dev.cpu().numpy()[:, :, :COUNTS[-1]])
            host.setflags(write=False)
            memo[n] = (dev, host)
        return memo[n]
    return get


@pytest.mark.parametrize("gi,pi", CASES, ids=CASE_IDS)
def test_every_profile_on_the_grid_equals_the_host_model(engine, clean_lists, gi, pi):
    """Both kernels at the checkpoints [0, 3, 65, 130], all 67 instances, against
    curve_host (tests/test_montecarlo_noise_profile.py checks the rotation)."""
    mc = sub("montecarlo")
    (n, nd), (kind, depol) = GRID[gi], PROFILES[pi]
    prof, adv = (rates_of(kind, n), depol), policy_at(gi, pi)
    dev, host = clean_lists(n)
    got = engine.montecarlo_curve_sampled_nprof(n, nd, GRID_BASE, INST, COUNTS, adversary=adv, noise=prof)
    got = got.cpu().numpy()
    _eq(engine.montecarlo_curve_lists_nprof(n, nd, GRID_BASE, dev, COUNTS, adversary=adv, noise=prof).cpu().numpy(),
        got, f"adv={adv:#x} lists:")
    if n <= 11:  # the C twin samples the clean lists
        want = mc.curve_host(n, COUNTS, nd, INST, GRID_BASE, HostEngine(), adversary=adv, noise=prof)
    else:  # the clean lists the device sampled; the host model puts the noise in
        want = mc.curve_host(n, COUNTS, nd, INST, GRID_BASE, HostEngine(), lists=host, adversary=adv, noise=prof)
    _eq(got, want, f"adv={adv:#x} host:")
    assert not got[:, :, 3].any()  # noise never raises a status bit


@pytest.mark.parametrize("n", NS)
def test_zero_and_uniform_profiles_equal_the_adv_curve_calls(engine, clean_lists, n):
    """All-zero == flip_q16 0 and uniform k == flip_q16 k for k in {1, 0x1000,
    0x8000}: the sampled kernel against the _adv curve call, the lists kernel
    against the _adv lists call on lists the existing noise_apply noised."""
    dev, _ = clean_lists(n)
    for nd in _nds(n):
        for k, adv in zip((0, 1, 0x1000, 0x8000), POLICIES + POLICIES[:1]):
            prof = ([k] * (n + 1), 0)
            _eq(engine.montecarlo_curve_sampled_nprof(n, nd, GRID_BASE, INST, COUNTS, adversary=adv, noise=prof)
                .cpu().numpy(),
                engine.montecarlo_curve_sampled(n, nd, GRID_BASE, INST, COUNTS, flip_q16=k, adversary=adv).cpu().numpy(),
                f"sampled nd={nd} k={k:#x}:")
            noised = engine.noise_apply(n, GRID_BASE, dev.clone(), COUNTS[-1], k)
            _eq(engine.montecarlo_curve_lists_nprof(n, nd, GRID_BASE, dev, COUNTS, adversary=adv, noise=prof)
                .cpu().numpy(),
                engine.montecarlo_curve_lists(n, nd, GRID_BASE, noised, COUNTS, adversary=adv).cpu().numpy(),
                f"lists nd={nd} k={k:#x}:")
    none = engine.montecarlo_curve_sampled_nprof(n, 0, GRID_BASE, INST, COUNTS).cpu().numpy()  # noise=None: all zero
    _eq(none, engine.montecarlo_curve_sampled(n, 0, GRID_BASE, INST, COUNTS, adversary=0xF).cpu().numpy(), "None:")


@pytest.mark.parametrize("n", [3, 7, 15])
def test_apply_equals_numpy_and_touches_nothing_else(engine, clean_lists, n):
    import torch
    mc = sub("montecarlo")
    count, fill, guard = COUNTS[-1], 0xA5, 256
    _, host = clean_lists(n)
    ld = (count + 3) // 4 * 4 + 8
    for prof in ((rates_of("mixed", n), 0x4000), (rates_of("zero", n), 0xFFFF), (rates_of("last", n), 0)):
        buf = torch.full((INST * (n + 1) * ld + guard,), fill, dtype=torch.uint8, device=engine.device)
        lists = buf[:INST * (n + 1) * ld].view(INST, n + 1, ld)
        lists[:, :, :count] = torch.from_numpy(np.array(host)).to(engine.device)
        before = buf.cpu().numpy().copy()
        assert engine.noise_profile_apply(n, GRID_BASE, lists, count, (rates_of("zero", n), 0)) is lists
        assert np.array_equal(buf.cpu().numpy(), before)
        engine.noise_profile_apply(n, GRID_BASE, lists, count, prof)
        after = buf.cpu().numpy()
        body = after[:INST * (n + 1) * ld].reshape(INST, n + 1, ld)
        want = np.stack([mc.noisy_lists_profile(n, (GRID_BASE + i) & MASK64, li, *prof) for i, li in enumerate(host)])
        assert np.array_equal(body[:, :, :count], want), (n, prof)
        assert np.all(body[:, :, count:] == fill) and np.all(after[-guard:] == fill)


def test_tally_and_failed_runs(engine):
    mc = sub("montecarlo")
    n, nd, cps, runs, base = 7, 2, [65, 200], 300, 0xAD0
    prof = mc.noise_profile(n, 0x0400, {0: 0x4000}, 0x0800)
    rows = engine.montecarlo_curve_sampled_nprof(n, nd, base, runs, cps, noise=prof)
    import torch
    tal = torch.zeros((len(cps), mc.TALLY_WORDS), dtype=torch.int64, device=engine.device)
    engine.montecarlo_tally(n, rows, tal)
    want, _ = mc.tally_host(n, rows.cpu().numpy())
    assert np.array_equal(tal.cpu().numpy(), want)
    plain = mc.curve(n, cps, nd, runs, base, engine, batch=128, noise=prof)
    for j, c in enumerate(cps):
        assert plain[c] == mc.summarize(n, rows[j].cpu().numpy()), c
    assert plain != mc.curve(n, cps, nd, runs, base, engine, batch=128)  # it matters
    few = mc.run(n, 200, nd, runs, base, engine, batch=128, path="fused", noise=prof, tally=True, failures=4)
    assert all(few[key] == plain[200][key] for key in plain[200])
    assert 1 <= len(few["failed_runs"]) == min(4, few["failed_total"])
    for i in few["failed_runs"]:
        row = mc.run_host(n, 200, nd, 1, base + i, HostEngine(), noise=prof)[0]
        assert row[3] == 0 and row[0] == 0, i


def test_a_capture_of_the_sampled_call_replays_the_uncaptured_rows(engine):
    """The call allocates and copies nothing: legal in a stream capture."""
    import torch
    n, nd, cps, base = 7, 2, [3, 65], 0xAD0
    prof = (rates_of("mixed", n), 0x4000)
    want = engine.montecarlo_curve_sampled_nprof(n, nd, base, INST, cps, noise=prof).cpu().numpy()  # warm: the program
    out = torch.zeros((2, INST, 4 + 5 * (n + 1)), dtype=torch.int32, device=engine.device)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            engine.montecarlo_curve_sampled_nprof(n, nd, base, INST, cps, out=out, noise=prof)
    torch.cuda.synchronize()
    assert not out.any()  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    _eq(out.cpu().numpy(), want, "replay:")
