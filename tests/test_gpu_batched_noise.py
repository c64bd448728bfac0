"""The noisy batched sampler on the GPU (qba_k_batched_noisy, DESIGN.md section
13.6).  Every comparison is exact, and the reference is never the new kernel:
the rows are those of the existing sample_check_batched followed by the existing
Engine.noise_apply (compared on the device) and of montecarlo.noisy_lists in
numpy; the tables are those of the single-instance Engine.check_counts and of
the Python oracle on those rows; the result rows are those of the fused noisy
kernel and of the lists kernel.

Rows that do not allow wide stores start 4 bytes into a larger buffer: the
calls refuse a base that is not 4-byte aligned (test_unaligned_base_is_refused),
so that is the nearest start that is not 8-byte aligned.  It takes byte rows to
the one-quad kernel; nibble rows need 4-byte alignment only and stay wide."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, sub
from montecarlo_programs import PROGRAMS
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

NS = [1, 3, 7, 11, 12, 15]
KS = [1, 0x1000, 0x5555, 0x8000, 0xFFFF]
# empty; inside and across a quad; a partial last quad after whole steps; under, at and over one queue drain;
# under and over one workgroup step of both QPT; a second trip of the step loop with leftover quads and an odd count
COUNTS = [0, 1, 3, 4, 5, 17, 63, 64, 65, 4095, 4097, 8205]
INST, HOST_INST, BASE = 67, 8, 0x5EED0
MASK64 = (1 << 64) - 1
FILL = 0xA5


def _eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)[0].tolist()
        raise AssertionError(f"{what} first difference at {at}: {got[tuple(at)]} != {want[tuple(at)]}")


def _rows(eng, n, inst, nb, off=0, guard=64):
    """A [inst, n+1, ld] view of rows of >= nb bytes, `off` bytes into a buffer
    filled with FILL that also holds `guard` bytes after the rows."""
    import torch
    ld = (nb + 7) // 8 * 8 + 8
    size = inst * (n + 1) * ld
    buf = torch.full((off + size + guard,), FILL, dtype=torch.uint8, device=eng.device)
    return buf[off:off + size].view(inst, n + 1, ld), buf


def _noisy_reference(eng, n, base, inst, count, k):
    """Device rows [inst, n+1, ld]: the existing batched sampler's, then the
    existing noise_apply.  Entry e depends on the key and e alone, so a smaller
    count is a prefix."""
    lists, _ = eng.sample_check_batched(n, base & MASK64, inst, count)
    clean = lists[:, :, :count].cpu().numpy()
    eng.noise_apply(n, base & MASK64, lists, count, k)
    return lists, clean


@pytest.fixture(scope="module")
def reference(engine):
    """(n, k) -> (noisy device rows at the largest count, the same on the host), read-only;
    the first HOST_INST instances are held to montecarlo.noisy_lists once."""
    memo = {}

    def get(n, k):
        if (n, k) not in memo:
            mc = sub("montecarlo")
            dev, clean = _noisy_reference(engine, n, BASE, INST, COUNTS[-1], k)
            host = np.ascontiguousarray(dev[:, :, :COUNTS[-1]].cpu().numpy())
            for i in range(HOST_INST):
                _eq(host[i], mc.noisy_lists(n, (BASE + i) & MASK64, clean[i], k), f"noise_apply against numpy, {i}:")
            assert (host != clean).any()
            host.setflags(write=False)
            memo[n, k] = dev, host
        return memo[n, k]
    return get


def _tables_of(eng, n, rows, count):
    """H, C, P of one instance's rows from the single-instance kernel."""
    return eng.check_counts(rows, n, count).numpy()


def _check_rows(got_view, packed, count, want_dev, want_host, what):
    import torch
    if not packed:
        assert torch.equal(got_view[:, :, :count], want_dev[:, :, :count]), what
        return
    em = sub("engine")
    inst, g, ld = got_view.shape
    raw = got_view.cpu().numpy().reshape(inst * g, ld)
    _eq(em.unpack_nibbles(raw, count).reshape(inst, g, -1)[:, :, :count], want_host[:, :, :count], what)
    if count & 1:
        assert not (raw[:, count // 2] >> 4).any(), what + " padding nibble"


@pytest.mark.parametrize("k", KS, ids=[f"k{k:#x}" for k in KS])
@pytest.mark.parametrize("n", NS)
def test_rows_and_tables(engine, reference, n, k):
    want_dev, want = reference(n, k)
    g = n + 1
    offdiag = 0
    for count in COUNTS:
        ref = [_tables_of(engine, n, want_dev[i], count) for i in range(HOST_INST)] if count else None
        if 0 < count <= 130:
            for i in (0, 1):
                flat = OracleEngine().count_tables(n, count, lists=want[i, :, :count])
                _eq(np.concatenate([t.ravel() for t in ref[i]]), flat, f"check_counts against the oracle, {i}:")
        for off in (0, 4):
            for packed in (False, True):
                what = f"n={n} k={k:#x} count={count} off={off} packed={packed}:"
                view, buf = _rows(engine, n, INST, (count + 1) // 2 if packed else count, off)
                lists, c = engine.sample_check_batched(n, BASE, INST, count, lists=view, packed=packed, flip_q16=k)
                assert lists is view
                _check_rows(view, packed, count, want_dev, want, what)
                if not count:
                    assert (buf == FILL).all(), what  # an empty call writes nothing
                    continue
                H, C, P = c.numpy()
                for i in range(HOST_INST):
                    _eq(H[i], ref[i][0], what + f" H[{i}]")
                    _eq(C[i], ref[i][1], what + f" C[{i}]")
                    _eq(P[i], ref[i][2], what + f" P[{i}]")
        if count:
            C8 = np.stack([r[1] for r in ref])
            offdiag += int(np.count_nonzero(C8 * (1 - np.eye(g, dtype=np.int64))))
    # Colliding Q entries, so the exact pair loop was reached: C[u][g][h], g != h, counts the Q entries of P_u whose
    # groups g and h hold the same value; the kernel's C of these instances was held equal to these tables above.
    # n = 1 is exempt: its entries have groups 0 and 1 alone, and a Q entry is one where those two differ.
    if k in (0x8000, 0xFFFF) and n > 1:
        assert offdiag > 0


@pytest.mark.parametrize("k", KS, ids=[f"k{k:#x}" for k in KS])
@pytest.mark.parametrize("n", NS)
def test_result_rows_equal_the_fused_noisy_kernel_and_the_lists_kernel(engine, n, k):
    for count in COUNTS:
        lists, c = engine.sample_check_batched(n, BASE, INST, count, flip_q16=k)
        if count == 0:  # the batched sampler writes nothing: the rows are defined on all-zero tables
            for t in (c.H, c.C, c.P):
                t.zero_()
        for nd in sorted({0, n // 3}):
            got = engine.protocol_batched(n, nd, BASE, c).cpu().numpy()
            what = f"n={n} k={k:#x} nd={nd} count={count}:"
            _eq(got, engine.montecarlo_sampled(n, nd, BASE, INST, count, flip_q16=k).cpu().numpy(), what + " fused")
            _eq(got, engine.montecarlo_lists(n, nd, BASE, lists, count).cpu().numpy(), what + " lists kernel")
            assert not got[:, 3].any()


def test_second_trip_of_the_instance_loop(engine):
    """More instances than the grid holds: a workgroup's second instance starts
    from a cleared histogram."""
    import torch
    n, count, k = 2, 37, 0x5555
    inst = torch.cuda.get_device_properties(engine.device).multi_processor_count * 16 + 3
    want_dev, _ = _noisy_reference(engine, n, BASE, inst, count, k)
    for packed in (False, True):
        lists, c = engine.sample_check_batched(n, BASE, inst, count, packed=packed, flip_q16=k)
        _check_rows(lists, packed, count, want_dev, want_dev.cpu().numpy(), f"packed={packed}:")
        P = c.P.cpu().numpy()
        for i in range(inst - 3, inst):
            _eq(P[i], _tables_of(engine, n, want_dev[i], count)[2], f"P[{i}] packed={packed}:")


@pytest.mark.parametrize("name", ["tables7", "general3"])
def test_other_samplers(name):
    """The canonical-table sampler at n = 7 and the general alias-table sampler:
    non-shipped programs on an engine of their own."""
    n, pair, _, _ = PROGRAMS[name]
    eng = sub("engine").Engine(0)
    try:
        info = eng.compile(n, *pair())
        assert not info["closed"]
        k, top = 0x1000, 4097
        want_dev, _ = _noisy_reference(eng, n, BASE, INST, top, k)
        want = want_dev.cpu().numpy()
        for count in (5, 65, top):
            ref = [_tables_of(eng, n, want_dev[i], count) for i in range(HOST_INST)]
            for off in (0, 4):
                for packed in (False, True):
                    what = f"{name} count={count} off={off} packed={packed}:"
                    view, _ = _rows(eng, n, INST, (count + 1) // 2 if packed else count, off)
                    _, c = eng.sample_check_batched(n, BASE, INST, count, lists=view, packed=packed, flip_q16=k)
                    _check_rows(view, packed, count, want_dev, want, what)
                    for i in range(HOST_INST):
                        for got, w in zip((c.H[i], c.C[i], c.P[i]), ref[i]):
                            _eq(got.cpu().numpy(), w, what + f" tables of {i}")
    finally:
        eng.close()


def _abi_call(eng, n, base, inst, count, k, packed, name=None, fill=FILL):
    """The C call on buffers of its own with canary words around the lists, H, C
    and P; returns the four whole buffers and their payload slices."""
    import torch
    em = sub("engine")
    _, w = eng.sizes(n)
    g = n + 1
    nb = (count + 1) // 2 if packed else count
    ld = (nb + 7) // 8 * 8 + 8
    pad = 64  # int64 words / bytes of canary on either side (8-byte aligned payloads)
    sizes = {"L": inst * g * ld, "H": inst * w * g * w, "C": inst * w * g * g, "P": inst * w}
    bufs = {key: torch.full((size + 2 * pad,), fill if key == "L" else -0x5A5A5A5A5A5A5A5B,
                            dtype=torch.uint8 if key == "L" else torch.int64, device=eng.device)
            for key, size in sizes.items()}
    pay = {key: b[pad:pad + sizes[key]] for key, b in bufs.items()}
    name = name or ("qba_sample_check_batched_packed_noisy" if packed else "qba_sample_check_batched_noisy")
    em.call(name, eng.ctx, n, base & MASK64, inst, count, k, em._ptr(pay["L"]), ld, g * ld, em._ptr(pay["H"]),
            em._ptr(pay["C"]), em._ptr(pay["P"]), eng.stream())
    return bufs, pay, pad, ld


@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
@pytest.mark.parametrize("n", [7, 12])
def test_canaries_and_zero_flip_is_the_noiseless_call(engine, n, packed):
    inst, count, k = 9, 65, 0x1000
    engine.prepare(n)
    nb = (count + 1) // 2 if packed else count
    for flip in (k, 0):
        bufs, pay, pad, ld = _abi_call(engine, n, BASE, inst, count, flip, packed)
        for key, b in bufs.items():
            canary = FILL if key == "L" else -0x5A5A5A5A5A5A5A5B
            assert (b[:pad] == canary).all() and (b[-pad:] == canary).all(), (key, flip)
        rows = pay["L"].view(inst, n + 1, ld)
        assert (rows[:, :, nb:] == FILL).all()  # nothing past the rows' bytes
        if flip:
            want_dev, _ = _noisy_reference(engine, n, BASE, inst, count, k)
            _check_rows(rows, packed, count, want_dev, want_dev.cpu().numpy(), "canary call:")
        else:
            lists, c = engine.sample_check_batched(n, BASE, inst, count, packed=packed)
            _eq(rows[:, :, :nb].cpu().numpy(), lists[:, :, :nb].cpu().numpy(), "k = 0 rows:")
            for key, t in (("H", c.H), ("C", c.C), ("P", c.P)):
                _eq(pay[key].cpu().numpy(), t.cpu().numpy().ravel(), f"k = 0 {key}:")


def test_unaligned_base_is_refused(engine):
    import torch
    em = sub("engine")
    n, count = 7, 65
    buf = torch.zeros(8 * 80 * 2 + 8, dtype=torch.uint8, device=engine.device)
    view = buf[1:1 + 2 * 8 * 80].view(2, 8, 80)
    with pytest.raises(sub("_lib").QbaError):
        engine.sample_check_batched(n, BASE, 2, count, lists=view, flip_q16=0x1000)
    assert not buf.any()


def test_other_stream_and_key_wrap(engine):
    import torch
    n, k, count = 7, 0x1000, 130
    want_lists, want_c = engine.sample_check_batched(n, BASE, INST, count, flip_q16=k)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lists, c = engine.sample_check_batched(n, BASE, INST, count, flip_q16=k)
    s.synchronize()
    assert torch.equal(lists[:, :, :count], want_lists[:, :, :count])
    for a, b in zip((c.H, c.C, c.P), (want_c.H, want_c.C, want_c.P)):
        assert torch.equal(a, b)
    base, inst = (1 << 64) - 3, 8
    want_dev, _ = _noisy_reference(engine, n, base, inst, count, k)
    lists, c = engine.sample_check_batched(n, base, inst, count, flip_q16=k)
    assert torch.equal(lists[:, :, :count], want_dev[:, :, :count])
    low, c_low = engine.sample_check_batched(n, 0, inst - 3, count, flip_q16=k)
    assert torch.equal(lists[3:, :, :count], low[:, :, :count]) and torch.equal(c.P[3:], c_low.P)
    for i in range(inst):
        _eq(c.C[i].cpu().numpy(), _tables_of(engine, n, want_dev[i], count)[1], f"wrapped key, C[{i}]:")


def test_run_tables_noisy_equals_run_fused(engine):
    mc = sub("montecarlo")
    n, nd, k, count, runs = 7, 2, 0x1000, 200, 300
    how = dict(batch=128, flip_q16=k)  # a batch split: 128 + 128 + 44
    want = mc.run(n, count, nd, runs, BASE, engine, path="fused", **how)
    assert mc.run(n, count, nd, runs, BASE, engine, path="tables_noisy", **how) == want
    assert mc.run(n, count, nd, runs, BASE, engine, path="tables_noisy", packed=False, **how) == want
    assert want != mc.run(n, count, nd, runs, BASE, engine, batch=128, path="tables")
    fused_all = mc.run(n, count, nd, runs, BASE, engine, path="fused", failures=runs, **how)
    fails = fused_all["failed_runs"]
    assert len(fails) == fused_all["failed_total"] > 4
    # montecarlo_tally hands its capture slots out in the order the tiles arrive, so with fewer slots than failed
    # runs WHICH runs are captured differs from launch to launch (tests/test_gpu_montecarlo_tally.py holds them to a
    # subset too): failures=4 is held to everything else and to a 4-subset, failed_runs themselves at full capture
    for extra in ({"tally": True}, {"failures": 4}, {"failures": runs}):
        got = mc.run(n, count, nd, runs, BASE, engine, path="tables_noisy", **how, **extra)
        fused = mc.run(n, count, nd, runs, BASE, engine, path="fused", **how, **extra)
        assert {key: v for key, v in got.items() if key != "failed_runs"} == \
            {key: v for key, v in fused.items() if key != "failed_runs"}, extra
        assert all(got[key] == want[key] for key in want)
        if "failures" in extra:
            cap = min(extra["failures"], len(fails))
            for r in (got, fused):
                assert len(r["failed_runs"]) == cap and r["failed_runs"] == sorted(set(r["failed_runs"])), extra
                assert set(r["failed_runs"]) <= set(fails), extra
    assert got["failed_runs"] == fused["failed_runs"] == fails  # every failed run captured: the same runs
    # without noise the new path is the tables path
    assert mc.run(n, count, nd, runs, BASE, engine, batch=128, path="tables_noisy") == \
        mc.run(n, count, nd, runs, BASE, engine, batch=128, path="tables")


def test_cli_tables_line_equals_the_fused_line():
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for extra in (["--tables"], []):
        cmd = [sys.executable, "-m", "tfg---quantum-byzantine-agreement_amd.tfg", "200", "2", "--parties", "7",
               "--runs", "256", "--flip", "4096", "--seed", "4242"] + extra
        res = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
        outs.append(res.stdout.strip().splitlines())
    assert outs[0] == outs[1] and len(outs[0]) == 1
    assert outs[0][0].startswith("Runs: 256 ") and outs[0][0].endswith(" flip=4096/65536")
