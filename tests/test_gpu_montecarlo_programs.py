"""The fused and the curve Monte-Carlo kernels on programs that are not the
shipped ones (tests/montecarlo_programs.py): the general alias-table sampler
inside qba_k_mc_sampled / qba_k_mc_curve_sampled and qba_k_batched, the
canonical-table sampler at an n whose shipped program is closed, and the
launchers' path on which fewer wavefronts of a workgroup take instances than
the kernel is built with (nw_run < NW), reached by tables smaller and by tables
larger than the canonical ones.

Every comparison is exact.  The references are the C twin's lists, the host
specification on them (montecarlo.run_host / curve_host, n <= 11), the lists
kernels on them (montecarlo_lists / montecarlo_curve_lists, which stage no
program) and the tables path (protocol_batched on sample_check_batched) --
never the kernel under test."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_lib
from conftest import sub
from montecarlo_cases import tables_rows
from montecarlo_programs import (LARGER_TABLES, PROGRAMS, REDUCED, SAMPLER_GENERAL, SAMPLER_TABLES, host_info,
                                 same_program, shifted_copy_pair, twin_lists)
from oracle_engine import OracleEngine

pytestmark = pytest.mark.gpu

NAMES = list(PROGRAMS)
COUNTS = [0, 1, 3, 63, 64, 65, 130]                    # empty, under / at / over a wave-step, over two
CHECKPOINTS = [0, 1, 2, 3, 5, 63, 64, 65, 127, 130]    # a superset of COUNTS
INST, BASE = 67, 0xA11CE                               # a ragged last workgroup for 2..8 running waves
TAIL_COUNT, TAIL_BASE = 33, 0xBEE5                     # the instance sets past the resident wave slots
TAIL_CHECKPOINTS = [0, 5, TAIL_COUNT]
HOST_MAX_N = 11                                        # montecarlo.run_host is the specification up to here


def _nds(n):
    return sorted({min(max(d, 0), n) for d in (0, 1, n // 3, n - 1)})


NAME_ND = [(name, nd) for name in NAMES for nd in _nds(PROGRAMS[name][0])]
NAME_ND_IDS = [f"{name}-d{nd}" for name, nd in NAME_ND]
REDUCED_ND = [(name, nd) for name, nd in NAME_ND if name in REDUCED]
REDUCED_ND_IDS = [f"{name}-d{nd}" for name, nd in REDUCED_ND]
HOST_ND = [(name, nd) for name, nd in NAME_ND if PROGRAMS[name][0] <= HOST_MAX_N]


def _eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        i, j = np.argwhere(got != want)[0]
        raise AssertionError(f"{what} instance {i}, word {j}: {got[i, j]} != {want[i, j]}\n"
                             f"got  {got[i].tolist()}\nwant {want[i].tolist()}")


@pytest.fixture(scope="module")
def programs():
    """name -> the program compiled on one fresh Engine (the session's engine
    keeps the shipped programs), with the shapes the launchers will use."""
    import torch
    eng = sub("engine").Engine(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {}
    for name, (n, pair, reduced, sampler) in PROGRAMS.items():
        info = eng.compile(n, *pair())
        assert not info["closed"] and info["canonical"] == (sampler == SAMPLER_TABLES), name
        shape = {"single": eng.montecarlo_program_shape(n), "curve": eng.montecarlo_program_shape(n, curve=True)}
        tail = {}
        for kernel, sh in shape.items():
            assert sh["sampler"] == sampler and (reduced == () or sampler == SAMPLER_GENERAL), (name, kernel, sh)
            assert 1 <= sh["waves_run"] <= sh["waves_compiled"] and sh["wgs_per_cu"] >= 1, (name, kernel, sh)
            assert (sh["waves_run"] < sh["waves_compiled"]) == (kernel in reduced), (name, kernel, sh)
            # every resident wave slot of the chip once, then a second, partial trip of the
            # persistent loop that is no whole number of workgroups
            tail[kernel] = cus * sh["wgs_per_cu"] * sh["waves_run"] + 2 * sh["waves_run"] + 1
        out[name] = SimpleNamespace(eng=eng, n=n, info=info, shape=shape, tail=tail, cus=cus)
    yield out
    eng.close()


@pytest.fixture(scope="module")
def refs(programs):
    """Memos of the references, each computed once and read-only: the C twin's
    lists (host and device copy), the host specification's rows, the lists
    kernel's rows and the device rows of the single-count call."""
    import torch
    mc = sub("montecarlo")
    lists, host, from_lists, single = {}, {}, {}, {}

    def sets(name):
        """set -> (base, instances, entries)"""
        p = programs[name]
        return {"grid": (BASE, INST, CHECKPOINTS[-1]), "tail": (TAIL_BASE, max(p.tail.values()), TAIL_COUNT)}

    def get_lists(name, which):
        if (name, which) not in lists:
            p = programs[name]
            base, inst, count = sets(name)[which]
            li = twin_lists(p.info, base, inst, count)
            lists[name, which] = (li, torch.from_numpy(np.array(li)).to(p.eng.device))
        return lists[name, which]

    def get_host(name, nd, count, curve=False):
        """Grid set, n <= 11: run_host, or the one-checkpoint curve_host (the same rows by definition)."""
        if (name, nd, count) not in host:
            p = programs[name]
            li = get_lists(name, "grid")[0]
            rows = mc.curve_host(p.n, [count], nd, INST, BASE, OracleEngine(), lists=li)[0] if curve else \
                mc.run_host(p.n, count, nd, INST, BASE, OracleEngine(), lists=li[:, :, :count])
            rows.setflags(write=False)
            host[name, nd, count] = rows
        return host[name, nd, count]

    def get_from_lists(name, nd, count):
        if (name, nd, count) not in from_lists:
            p = programs[name]
            rows = p.eng.montecarlo_lists(p.n, nd, BASE, get_lists(name, "grid")[1], count).cpu().numpy()
            rows.setflags(write=False)
            from_lists[name, nd, count] = rows
        return from_lists[name, nd, count]

    def get_single(name, nd, which, inst, count):
        if (name, nd, which, inst, count) not in single:
            p = programs[name]
            rows = p.eng.montecarlo_sampled(p.n, nd, sets(name)[which][0], inst, count).cpu().numpy()
            rows.setflags(write=False)
            single[name, nd, which, inst, count] = rows
        return single[name, nd, which, inst, count]

    return SimpleNamespace(sets=sets, lists=get_lists, host=get_host, from_lists=get_from_lists, single=get_single)


def test_reduced_wave_counts_are_reached_for_both_kernels_on_both_sides_of_the_host_limit():
    """About the program list: each of the two kernels runs fewer waves than
    compiled on a program the host specification reaches and on one above it
    (where the kernels have no closed-form instantiation beside the general one)."""
    for kernel in ("single", "curve"):
        ns = [PROGRAMS[name][0] for name in REDUCED if kernel in PROGRAMS[name][2]]
        assert any(n <= HOST_MAX_N for n in ns) and any(n > HOST_MAX_N for n in ns), kernel
    assert 11 in [PROGRAMS[name][0] for name in REDUCED]


def test_shipped_programs_report_the_static_shapes(engine):
    lib = sub("_lib").lib()
    import ctypes as C
    for n in range(1, 16):
        engine.prepare(n)
        for curve, static in ((False, lib.qba_montecarlo_shape), (True, lib.qba_montecarlo_curve_shape)):
            waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
            assert static(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
            sh = engine.montecarlo_program_shape(n, curve=curve)
            assert sh == {"sampler": 2 if n <= 11 else 1, "waves_compiled": waves.value, "waves_run": waves.value,
                          "lds_bytes": lds.value, "wgs_per_cu": wgs.value}, (n, curve, sh)


@pytest.mark.parametrize("name", NAMES)
def test_compiled_program_equals_the_golden_file(programs, name):
    """The CPU tests sample from tests/golden/montecarlo_programs.npz."""
    want = host_info(name)
    for kind in ("notq", "q"):
        assert same_program(programs[name].info[kind], want[kind]), (name, kind)


def test_larger_tables_cost_a_wave_of_the_one_workgroup_a_cu_holds(programs):
    """The other side from the small-table programs: more table entries than the
    canonical program the kernel is built for, one workgroup per CU before and
    after, one wave fewer."""
    for name in LARGER_TABLES:
        p = programs[name]
        nbits = p.n * p.info["nq"]
        canonical = 256 * ((nbits + 7) // 8 - 1) + (1 << (nbits - 8 * ((nbits + 7) // 8 - 1))) + (1 << p.info["nq"])
        assert len(p.info["notq"]["pat"]) + len(p.info["q"]["pat"]) > canonical
        reduced = [p.shape[k] for k in PROGRAMS[name][2]]
        assert reduced and all(sh["wgs_per_cu"] == 1 and sh["waves_run"] == sh["waves_compiled"] - 1 for sh in reduced)


BATCHED = [(name, "grid") for name in NAMES] + [(name, "tail") for name in REDUCED]


@pytest.mark.parametrize("name,which", BATCHED, ids=[f"{name}-{which}" for name, which in BATCHED])
def test_batched_lists_and_counts_equal_the_c_twin(programs, refs, name, which):
    """qba_k_batched on the general sampler: every instance's rows and tables."""
    p = programs[name]
    base, inst, count = refs.sets(name)[which]
    want = refs.lists(name, which)[0]
    lists, c = p.eng.sample_check_batched(p.n, base, inst, count)
    got = lists[:, :, :count].cpu().numpy()
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        raise AssertionError(f"lists differ first at (instance, row, entry) {np.argwhere(got != want)[0].tolist()}")
    gH, gC, gP = c.numpy()
    with oracle_lib.single_thread():
        for i in range(inst):
            H, C, P, bad = oracle_lib.counts(want[i], p.n)
            assert bad == 0 and np.array_equal(gH[i], H) and np.array_equal(gC[i], C) and np.array_equal(gP[i], P), i
    assert (want[:, 0] != want[:, 1]).any() and (want[:, 0] == want[:, 1]).any()


SINGLE = [(name, nd, c) for name, nd in NAME_ND for c in COUNTS]


@pytest.mark.parametrize("name,nd,count", SINGLE, ids=[f"{name}-d{nd}-L{c}" for name, nd, c in SINGLE])
def test_single_count_equals_host_lists_form_and_tables_path(programs, refs, name, nd, count):
    p = programs[name]
    got = refs.single(name, nd, "grid", INST, count)
    if p.n <= HOST_MAX_N:
        _eq(got, refs.host(name, nd, count), "host:")
    _eq(got, refs.from_lists(name, nd, count), "lists form:")
    _eq(got, tables_rows(p.eng, p.n, nd, BASE, INST, count), "tables path:")
    assert not got[:, 3].any()


def _host_ends(p, refs, name, nd, inst, got, what):
    """n <= 11: the host specification on the first instances and on the last
    ones, those of the persistent loop's second trip (instance i depends on
    key base + i and its own lists alone)."""
    if p.n > HOST_MAX_N:
        return
    mc = sub("montecarlo")
    li = refs.lists(name, "tail")[0]
    for a, b in ((0, 9), (inst - 24, inst)):
        want = mc.run_host(p.n, TAIL_COUNT, nd, b - a, TAIL_BASE + a, OracleEngine(), lists=li[a:b])
        _eq(got[a:b], want, f"{what} host, instances {a}..{b}:")


@pytest.mark.parametrize("name,nd", REDUCED_ND, ids=REDUCED_ND_IDS)
def test_single_count_past_the_resident_wave_slots(programs, refs, name, nd):
    """More instances than num_cus * wgs_per_cu * waves_run, by no multiple of
    waves_run: the reduced stride gridDim.x * nw_run of the second trip."""
    p = programs[name]
    inst = p.tail["single"]
    sh = p.shape["single"]
    assert inst > p.cus * sh["wgs_per_cu"] * sh["waves_run"] and (sh["waves_run"] == 1 or inst % sh["waves_run"])
    got = refs.single(name, nd, "tail", inst, TAIL_COUNT)
    dev = refs.lists(name, "tail")[1][:inst]
    _eq(got, p.eng.montecarlo_lists(p.n, nd, TAIL_BASE, dev, TAIL_COUNT).cpu().numpy(), "lists form:")
    _eq(got, tables_rows(p.eng, p.n, nd, TAIL_BASE, inst, TAIL_COUNT), "tables path:")
    _host_ends(p, refs, name, nd, inst, got, "single")
    assert not got[:, 3].any()


def _eq_slices(got, want_of, counts, what=""):
    got = np.asarray(got)
    assert got.ndim == 3 and got.shape[0] == len(counts)
    for j, c in enumerate(counts):
        _eq(got[j], want_of(c), f"{what} checkpoint {j} (count {c}):")


@pytest.fixture(scope="module")
def curves(programs):
    memo = {}

    def get(name, nd):
        if (name, nd) not in memo:
            p = programs[name]
            rows = p.eng.montecarlo_curve_sampled(p.n, nd, BASE, INST, CHECKPOINTS).cpu().numpy()
            rows.setflags(write=False)
            memo[name, nd] = rows
        return memo[name, nd]
    return get


@pytest.mark.parametrize("name,nd", NAME_ND, ids=NAME_ND_IDS)
def test_curve_equals_the_single_count_call_and_the_lists_form_at_every_checkpoint(programs, refs, curves, name, nd):
    p = programs[name]
    got = curves(name, nd)
    assert got.shape == (len(CHECKPOINTS), INST, 4 + 5 * (p.n + 1))
    _eq_slices(got, lambda c: refs.single(name, nd, "grid", INST, c), CHECKPOINTS, "single:")
    dev = refs.lists(name, "grid")[1]
    _eq_slices(p.eng.montecarlo_curve_lists(p.n, nd, BASE, dev, CHECKPOINTS).cpu().numpy(),
               lambda c: got[CHECKPOINTS.index(c)], CHECKPOINTS, "curve lists:")
    _eq_slices(got, lambda c: refs.from_lists(name, nd, c), CHECKPOINTS, "lists form:")
    assert not got[:, :, 3].any()


HOST_CURVE = [(name, nd, j) for name, nd in HOST_ND for j in range(len(CHECKPOINTS))]


@pytest.mark.parametrize("name,nd,j", HOST_CURVE, ids=[f"{name}-d{nd}-L{CHECKPOINTS[j]}" for name, nd, j in HOST_CURVE])
def test_curve_slice_equals_the_host_specification(refs, curves, name, nd, j):
    """montecarlo.curve_host on the C twin's lists, one checkpoint per case (it
    is the stack of run_host over the checkpoints: tests/test_montecarlo_programs.py)."""
    _eq(curves(name, nd)[j], refs.host(name, nd, CHECKPOINTS[j], curve=True), f"count {CHECKPOINTS[j]}:")


@pytest.mark.parametrize("name,nd", REDUCED_ND, ids=REDUCED_ND_IDS)
def test_curve_past_the_resident_wave_slots(programs, refs, name, nd):
    p = programs[name]
    inst = p.tail["curve"]
    sh = p.shape["curve"]
    assert inst > p.cus * sh["wgs_per_cu"] * sh["waves_run"] and (sh["waves_run"] == 1 or inst % sh["waves_run"])
    got = p.eng.montecarlo_curve_sampled(p.n, nd, TAIL_BASE, inst, TAIL_CHECKPOINTS).cpu().numpy()
    dev = refs.lists(name, "tail")[1][:inst]
    _eq_slices(got, lambda c: p.eng.montecarlo_lists(p.n, nd, TAIL_BASE, dev, c).cpu().numpy(), TAIL_CHECKPOINTS,
               "lists form:")
    _eq_slices(p.eng.montecarlo_curve_lists(p.n, nd, TAIL_BASE, dev, TAIL_CHECKPOINTS).cpu().numpy(),
               lambda c: got[TAIL_CHECKPOINTS.index(c)], TAIL_CHECKPOINTS, "curve lists:")
    _eq(got[-1], refs.single(name, nd, "tail", inst, TAIL_COUNT), "single:")
    _host_ends(p, refs, name, nd, inst, got[-1], "curve")
    assert not got[:, :, 3].any()


@pytest.mark.parametrize("name", NAMES)
def test_reference_rows_hold_both_outcomes_and_tell_checkpoints_apart(programs, refs, name):
    """About the inputs, not the kernels under test: on the reference rows alone.
    They come from the lists kernel on the C twin's lists -- device output, but
    of a kernel that stages no program and shares nothing with the launches
    under test.  For n <= 11 they are held to the host specification (here at
    one nd and count, in the single-count test at all); above n = 11 there is
    no host specification, and both outcomes are asserted on these rows alone."""
    p = programs[name]
    ok = total = 0
    for nd in _nds(p.n):
        rows = [refs.from_lists(name, nd, c) for c in CHECKPOINTS]
        if nd >= 1:
            assert len({r.tobytes() for r in rows}) >= 2, (name, nd)
        assert not any(r[:, 3].any() for r in rows)
        ok += sum(int(r[:, 0].sum()) for r in rows)
        total += sum(len(r) for r in rows)
    assert 0 < ok < total, (name, ok, total)
    if p.n <= HOST_MAX_N:
        nd = max(1, p.n // 3)
        host = refs.host(name, nd, CHECKPOINTS[-1])
        _eq(refs.from_lists(name, nd, CHECKPOINTS[-1]), host, "lists form against the host:")


@pytest.mark.parametrize("name", REDUCED)
def test_reduced_launches_write_their_rows_only(programs, refs, name):
    """Fill words before, after and inside the [k, inst, words] block: nothing
    outside is written and none inside is left."""
    import torch
    p = programs[name]
    n, nd, inst, counts = p.n, max(1, p.n // 3), 37, [0, 3, 70]
    words, fill, guard = 4 + 5 * (n + 1), 0x5A5A5A5A, 64
    for k, run, want_of in (
            (1, lambda o: p.eng.montecarlo_sampled(n, nd, BASE, inst, counts[-1], out=o[0]),
             lambda c: refs.from_lists(name, nd, counts[-1])[:inst]),
            (len(counts), lambda o: p.eng.montecarlo_curve_sampled(n, nd, BASE, inst, counts, out=o),
             lambda c: refs.from_lists(name, nd, c)[:inst])):
        buf = torch.full((guard + k * inst * words + guard,), fill, dtype=torch.int32, device=p.eng.device)
        out = buf[guard:guard + k * inst * words].view(k, inst, words)
        run(out)
        flat = buf.cpu().numpy()
        assert np.all(flat[:guard] == fill) and np.all(flat[-guard:] == fill)
        rows = out.cpu().numpy()
        assert not np.any(rows == fill)
        _eq_slices(rows, want_of, counts[-k:])


def test_prepare_after_compile_restores_the_shipped_program_and_shape(engine):
    """compile, then prepare on the same engine: the rows and the shape are the
    shipped program's again (no stale shape, no stale staged tables).  The
    small-table program shows a stale shape; its rows are the shipped ones'
    (its not-Q entries keep L0 == L1), so a stale table shows on the program
    with group 0 copied from group 2, whose rows differ."""
    import ctypes as C
    lib = sub("_lib").lib()
    eng = sub("engine").Engine(0)
    try:
        for name in ("narrow11", "narrow12"):
            n, pair, reduced, _ = PROGRAMS[name]
            nd, count = n // 3, 65
            eng.compile(n, *pair())
            sh = eng.montecarlo_program_shape(n, curve="curve" in reduced)
            assert sh["sampler"] == SAMPLER_GENERAL and sh["waves_run"] < sh["waves_compiled"]
            info = eng.compile(n, *shifted_copy_pair(n))
            assert info["canonical"] and not info["closed"]
            assert eng.montecarlo_program_shape(n)["sampler"] == SAMPLER_TABLES
            other = eng.montecarlo_sampled(n, nd, BASE, INST, count).cpu().numpy()
            info = eng.prepare(n, perm=list(range(1, n + 1)))
            assert info["canonical"] and info["closed"] == (n <= 11)
            want = engine.montecarlo_sampled(n, nd, BASE, INST, count).cpu().numpy()
            _eq(eng.montecarlo_sampled(n, nd, BASE, INST, count).cpu().numpy(), want, name)
            _eq(eng.montecarlo_curve_sampled(n, nd, BASE, INST, [3, count]).cpu().numpy()[1], want, name)
            assert not np.array_equal(other, want)
            for curve, static in ((False, lib.qba_montecarlo_shape), (True, lib.qba_montecarlo_curve_shape)):
                waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
                assert static(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
                assert eng.montecarlo_program_shape(n, curve=curve) == {
                    "sampler": 2 if n <= 11 else 1, "waves_compiled": waves.value, "waves_run": waves.value,
                    "lds_bytes": lds.value, "wgs_per_cu": wgs.value}
    finally:
        eng.close()
