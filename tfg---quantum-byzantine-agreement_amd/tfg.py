"""Command line of the engine, interface-compatible with the reference
(README.md:4):

    mpiexec -n <nParties+1> python -m tfg---quantum-byzantine-agreement_amd.tfg <sizeL> <nDishonest>

Three launch shapes:

* ``mpiexec -n <n+1>`` -- one process per party, as the reference.  The MPI
  layer is mpi4py when importable, else the package's ctypes binding of
  MPICH (mpi.py).  Exact mode: every party owns a GPU engine (device =
  rank % visible GPUs).  Count mode: the first G = min(n+1, GPUs) ranks own
  a GPU each, sample + check their sizeL shard and sum the counts with one
  RCCL all-reduce (C ABI qba_allreduce_i64; the unique id travels over MPI).
  ``--rounds epoch`` gives the rounds barrier-epoch delivery (deterministic,
  = the golden fixtures); the default keeps the reference's own rounds.
* ``torchrun --nproc-per-node G ... --mode count`` -- G GPU owners, one per
  GPU; rank 0 runs all n+1 parties in-process (LocalWorld), the count pass is
  sharded over the G ranks (torch.distributed all-reduce over RCCL).
* plain ``python -m ...tfg`` -- all parties in-process on one GPU
  (``--parties N`` sets nParties, default 3).

``--mode count`` evaluates the protocol from device count histograms
(canonical order), which is what makes sizeL = 1e9 practical; the default
``exact`` mode reproduces tfg.py's own set-order semantics.  Without
``--seed`` the lists and every party's random choices are drawn from OS
entropy, as the reference's unseeded ``np.random``; with it runs repeat.
"""
from __future__ import annotations

import argparse
import os
import secrets
import sys
import time

import numpy as np

from . import comm as comm_mod
from . import countmode, protocol

RCCL_ID_TAG = 29_999


CURVE_MAX = 32  # checkpoints of one --curve run (QBA_MC_CURVE_MAX)


def _sizes(text: str):
    return [int(float(x)) for x in text.split(",") if x.strip()]


SWEEP_MAX = 16  # scenarios of one --sweep run (QBA_MC_SWEEP_MAX)
GRID_MAX = 16  # items of one --grid run (QBA_MC_GRID_MAX)
EXPLAIN_CAP = 1024  # events kept per rank of an --explain transcript (the rest are counted)


def _scenarios(text: str, n_dishonest: int, montecarlo) -> list:
    """--sweep's K:POLICY,... as [(K, policy word)]: a bare POLICY takes
    ``n_dishonest``, a bare K the reference policy."""
    out = []
    for item in (x.strip() for x in text.split(",") if x.strip()):
        k, sep, pol = item.partition(":")
        if not sep:  # a decimal number is a traitor count; anything else a policy
            k, pol = (k, "reference") if k.isdigit() else (str(n_dishonest), k)
        out.append((int(k), montecarlo.parse_adversary(pol.strip())))
    if len(set(out)) != len(out):
        raise ValueError("a scenario is given twice")
    return out


def _grid_items(text: str, n_dishonest: int, montecarlo) -> list:
    """--grid's SCENARIO[@DROP[:cmd]],... as [(K, policy word, network word)]:
    SCENARIO as --sweep takes it, DROP[:cmd] as --drop does; absent, the
    perfect network."""
    out = []
    for item in (x.strip() for x in text.split(",") if x.strip()):
        scen, sep, drop = item.partition("@")
        sc = _scenarios(scen, n_dishonest, montecarlo)
        if len(sc) != 1 or (sep and not drop.strip()):
            raise ValueError(f"{item!r} is not SCENARIO[@DROP[:cmd]]")
        out.append(sc[0] + (montecarlo.parse_net(drop.strip()) if sep else 0,))
    if len(set(out)) != len(out):
        raise ValueError("an item is given twice")
    return out


def _args(argv):
    ap = argparse.ArgumentParser(prog="tfg", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sizeL", type=float)
    ap.add_argument("nDishonest", type=int)
    ap.add_argument("--parties", type=int, default=3, help="nParties for an in-process run")
    ap.add_argument("--mode", choices=["exact", "count"], default="exact")
    ap.add_argument("--rounds", choices=["reference", "epoch"], default="reference",
                    help="reference: tfg.py's own (racy) rounds; epoch: barrier-epoch delivery")
    ap.add_argument("--seed", type=int, default=None, help="rank RNG seed and list seed")
    ap.add_argument("--runs", type=int, default=None,
                    help="in-process: this many independent count-mode instances, lists, rounds and decisions "
                         "on the device (montecarlo.run); prints runs, successes and the success rate")
    ap.add_argument("--batch", type=int, default=4096, help="instances per device batch of --runs")
    ap.add_argument("--fused", action="store_true",
                    help="with --runs: sample, distil and decide each batch in one kernel, with no list buffer and "
                         "no count tables (montecarlo.run path='fused'); the same instances and summary")
    ap.add_argument("--curve", type=_sizes, default=None, metavar="C0,C1,...",
                    help="with --runs: decide every instance at each of these sizeL and at the positional sizeL in "
                         "one pass per batch (montecarlo.curve; at most 32 in all); one summary line per sizeL, "
                         "increasing; implies --fused")
    ap.add_argument("--tally", action="store_true",
                    help="with --runs: reduce each batch's result rows on the device (montecarlo.run tally=True); the "
                         "same summary lines, from device memory that does not grow with --runs")
    ap.add_argument("--failures", type=int, default=0, metavar="K",
                    help="with --runs: after each summary line, the indices of up to K runs without success, to "
                         "replay under key seed + index; implies --tally")
    ap.add_argument("--explain", type=int, default=0, metavar="K",
                    help="with --runs: --failures K, and after each line's failed indices the transcript of those "
                         "runs' protocol rounds as the device re-ran them (montecarlo.format_trace: every packet "
                         "received with its verdict, every send with the traitor's action, every decision)")
    ap.add_argument("--flip", type=int, default=None, metavar="K",
                    help="with --runs: every measured qubit flips with probability K / 65536, 0 <= K <= 65535 "
                         "(montecarlo.noise_masks); implies --fused unless --tables is given; with K > 0 the "
                         "summary lines end in flip=K/65536")
    ap.add_argument("--tables", action="store_true",
                    help="with --runs: sample and count each batch's lists in the batched sampler, then decide them "
                         "(montecarlo.run path='tables_noisy'): with --flip K the noisy lists and tables, the same "
                         "instances and summary as the fused kernels'; not with --curve or --fused")
    ap.add_argument("--adversary", default=None, metavar="NAME|0xHEX",
                    help="with --runs: the dishonest parties follow this policy, a preset (reference, relay, "
                         "reorder_low, mute, strip) or a policy word (montecarlo.adversary); the summary lines "
                         "end in adversary=0xWORD")
    ap.add_argument("--collude", default=None, metavar="NAME|0xHEX",
                    help="with --runs: the dishonest parties collude, a preset (late, late_relayed, late_one, "
                         "starve_late) or a coalition word (montecarlo.coalition): they withhold packets from honest "
                         "lieutenants and inject them in a late round, padded with each other's tuples; implies "
                         "--fused; the summary lines end in collude=0xWORD; not with --sweep, --explain or --tables")
    ap.add_argument("--drop", default=None, metavar="K[:cmd]",
                    help="with --runs: every lieutenant-to-lieutenant packet is lost in flight with probability "
                         "K / 65536 (K decimal or 0x hex; montecarlo.net), with :cmd the commander's packets too; "
                         "implies --fused; the summary lines end in drop=K/65536 [cmd]; not with --collude, --sweep, "
                         "--explain or --tables")
    ap.add_argument("--noise", default=None, metavar="all:K,G:K,...,depol:K",
                    help="with --runs: a noise profile (montecarlo.noise_profile): every measured bit of list row G "
                         "flips with probability K / 65536 (row 0 the commander's list, 1 Lc, G >= 2 lieutenant G; "
                         "all:K sets every row, a row given after it overrides), and with depol:K a whole entry is "
                         "depolarised with probability K / 65536 (K decimal or 0x hex); implies --fused; the summary "
                         "lines end in noise=SPEC in normal form; not with --flip, --collude, --drop, --sweep, --grid, "
                         "--explain, --tables or --replay")
    ap.add_argument("--sweep", default=None, metavar="K:POLICY,...",
                    help="with --runs: decide every instance under each of these scenarios in one pass per batch "
                         "(montecarlo.sweep; at most 16, and 32 lines with --curve): K traitors following POLICY "
                         "(as --adversary takes it); a bare POLICY uses the positional nDishonest, a bare K the "
                         "reference policy; one summary line per sizeL and scenario; implies --fused")
    ap.add_argument("--grid", default=None, metavar="SCENARIO[@DROP[:cmd]],...",
                    help="with --runs: decide every instance under each of these items in one pass per batch "
                         "(montecarlo.grid; at most 16, and 32 lines with --curve): SCENARIO as --sweep takes it "
                         "(K:POLICY, a bare K or a bare POLICY) on the network DROP[:cmd] as --drop takes it (absent: "
                         "the perfect network), e.g. 2@0,2@0x0100,2@0x1000:cmd,2:reorder_low@0x0400; one summary "
                         "line per sizeL and item; implies --fused; not with --sweep, --drop, --adversary, "
                         "--collude, --explain or --tables")
    ap.add_argument("--replay", default=None, metavar="I[,J,...]",
                    help="with --seed: re-run the runs I, J, ... of a --runs command with these flags (--flip, "
                         "--adversary, --drop K[:cmd], --curve) on the device under key seed + index, the indices "
                         "--failures prints, and print each one's transcript (montecarlo.replay, "
                         "montecarlo.format_trace) headed 'run I', with --curve 'sizeL=C run I'; a lost packet shows "
                         "as 'loses in flight', a lost commander packet as 'no packet arrived'; not with --runs, "
                         "--collude, --sweep, --grid, --tables or --explain")
    ap.add_argument("--quiet", action="store_true", help="print only the outcome")
    ap.add_argument("--timing", action="store_true", help="print the wall time of the run")
    ap.add_argument("--wire", action="store_true",
                    help="in-process exact mode: send the lists in the reference's int64-per-bit wire layout "
                         "(tfg.py:142-161) instead of handing each rank its device row")
    a = ap.parse_args(argv)
    if a.noise is not None:
        given = [flag for flag, on in (("--flip", a.flip is not None), ("--collude", a.collude is not None),
                                       ("--drop", a.drop is not None), ("--sweep", a.sweep is not None),
                                       ("--grid", a.grid is not None), ("--explain", a.explain),
                                       ("--tables", a.tables), ("--replay", a.replay is not None)) if on]
        if given:
            ap.error(f"--noise: not with {', '.join(given)} (a profile holds the flip rates itself, and the "
                     "coalition, lossy-network, sweep, grid, trace and tables paths are not built for one)")
        if a.runs is None:
            ap.error("--noise needs --runs")
        from . import montecarlo
        try:
            a.noise = montecarlo.parse_noise_profile(a.parties, a.noise)
        except montecarlo.QbaError as e:
            ap.error(f"--noise: {e}")
        a.fused = True
    if a.replay is not None:
        given = [flag for flag, on in (("--runs", a.runs is not None), ("--collude", a.collude is not None),
                                       ("--sweep", a.sweep is not None), ("--grid", a.grid is not None),
                                       ("--tables", a.tables), ("--explain", a.explain)) if on]
        if given:
            ap.error(f"--replay: not with {', '.join(given)} (it re-runs the indices it is given, one transcript "
                     "each; name a --grid or --sweep item's K, --adversary and --drop; a coalition's runs have no "
                     "transcript)")
        if a.seed is None:
            ap.error("--replay needs --seed (key = seed + index)")
        try:
            a.replay = [int(x, 0) for x in a.replay.split(",") if x.strip()]
        except ValueError:
            ap.error("--replay: I[,J,...] are run indices (decimal or 0x hex)")
        if not a.replay or min(a.replay) < 0 or max(a.replay) >= 1 << 64:
            ap.error("--replay: at least one index, each in [0, 2^64)")
    if a.curve is not None:
        if a.runs is None and a.replay is None:
            ap.error("--curve needs --runs")
        a.curve = sorted(set(a.curve) | {int(a.sizeL)})
        if len(a.curve) > CURVE_MAX:
            ap.error(f"--curve: at most {CURVE_MAX} checkpoints (the positional sizeL included), not {len(a.curve)}")
        if a.curve[0] < 0 or a.curve[-1] >= 1 << 31:
            ap.error("--curve: every sizeL must be in [0, 2^31)")
    if a.explain < 0:
        ap.error("--explain: K >= 0")
    if a.explain:
        if a.runs is None:
            ap.error("--explain needs --runs")
        a.failures = a.explain
    if a.failures < 0:
        ap.error("--failures: K >= 0")
    if (a.tally or a.failures) and a.runs is None:
        ap.error("--tally and --failures need --runs")
    if a.tables:
        if a.runs is None:
            ap.error("--tables needs --runs")
        if a.curve is not None or a.fused:
            ap.error("--tables: not with --curve or --fused")
    if a.flip is not None:
        if a.runs is None and a.replay is None:
            ap.error("--flip needs --runs")
        if not 0 <= a.flip <= 65535:
            ap.error("--flip: K must be in [0, 65535] (out of 65536)")
        a.fused = not a.tables
    if a.adversary is not None:
        if a.runs is None and a.replay is None:
            ap.error("--adversary needs --runs")
        from . import montecarlo
        try:
            a.adversary = montecarlo.parse_adversary(a.adversary)
        except montecarlo.QbaError as e:
            ap.error(f"--adversary: {e}")
    if a.collude is not None:
        if a.runs is None:
            ap.error("--collude needs --runs")
        if a.sweep is not None or a.explain or a.tables:
            ap.error("--collude: not with --sweep, --explain or --tables (the sweep, trace and tables paths "
                     "are not built for a coalition)")
        from . import montecarlo
        try:
            a.collude = montecarlo.parse_coalition(a.collude)
        except montecarlo.QbaError as e:
            ap.error(f"--collude: {e}")
        a.fused = True
    if a.drop is not None:
        if a.runs is None and a.replay is None:
            ap.error("--drop needs --runs")
        if a.collude is not None or a.sweep is not None or a.explain or a.tables:
            ap.error("--drop: not with --collude, --sweep, --explain or --tables (the coalition, sweep, trace and "
                     "tables paths are not built for a lossy network)")
        from . import montecarlo
        try:
            a.drop = montecarlo.parse_net(a.drop)
        except montecarlo.QbaError as e:
            ap.error(f"--drop: {e}")
        a.fused = True
    if a.sweep is not None:
        if a.runs is None:
            ap.error("--sweep needs --runs")
        if a.adversary is not None or a.tables:
            ap.error("--sweep: not with --adversary (name the policy per scenario) or --tables")
        from . import montecarlo
        try:
            a.sweep = _scenarios(a.sweep, a.nDishonest, montecarlo)
        except (ValueError, montecarlo.QbaError) as e:
            ap.error(f"--sweep: {e}")
        if not 1 <= len(a.sweep) <= SWEEP_MAX or len(a.sweep) * len(a.curve or [0]) > CURVE_MAX:
            ap.error(f"--sweep: between 1 and {SWEEP_MAX} scenarios, and at most {CURVE_MAX} lines with --curve")
    if a.grid is not None:
        if a.runs is None:
            ap.error("--grid needs --runs")
        if a.sweep is not None or a.drop is not None or a.adversary is not None or a.collude is not None or \
                a.explain or a.tables:
            ap.error("--grid: not with --sweep, --drop, --adversary (name the policy and the network per item), "
                     "--collude, --explain or --tables (the coalition, trace and tables paths are not built for a "
                     "lossy network)")
        from . import montecarlo
        try:
            a.grid = _grid_items(a.grid, a.nDishonest, montecarlo)
        except (ValueError, montecarlo.QbaError) as e:
            ap.error(f"--grid: {e}")
        if not 1 <= len(a.grid) <= GRID_MAX or len(a.grid) * len(a.curve or [0]) > CURVE_MAX:
            ap.error(f"--grid: between 1 and {GRID_MAX} items, and at most {CURVE_MAX} lines with --curve")
        a.fused = True
    return a


def _outcome(res, verbose):
    if res is not None and not verbose:
        print("Decisions:", np.array(res["decisions"]))
        print("Dishonests:", np.array(res["dishonest"]))
        print("Success:", res["success"])


class RcclLink:
    """How the GPU owners of an mpiexec count run form their all-reduce group:
    an RCCL communicator through the C ABI (qba_rccl_init), its unique id
    created on rank 0 and sent to the other owners over MPI."""

    @staticmethod
    def unique_id() -> bytes:
        from .engine import Engine
        return Engine.rccl_unique_id()

    @staticmethod
    def allreduce(eng, uid: bytes, owners: int, rank: int):
        eng.rccl_init(uid, owners, rank)
        return countmode.rccl_allreduce(eng)


def count_owners(world, mpi, ndev: int, make_engine, link=RcclLink):
    """Count mode under mpiexec: the first G = min(ranks,
    GPUs) ranks own a GPU each (device = rank % ndev) and shard the count pass
    (countmode.ShardCounter); for G > 1 rank 0 makes the group's unique id and
    sends it to owners 1..G-1 over MPI, and every owner joins the group; a
    one-element all-reduce of ones then checks that the group sums exactly G
    owners (ShardCounter.check_group).
    Returns (engine or None, CountParty keyword arguments).  make_engine and
    link are the seams the CPU test of G > 1 owners fills with the numpy engine
    and an all-reduce over MPI (tests/mpi_driver.py --owners)."""
    rank, size = world.Get_rank(), world.Get_size()
    g = min(size, ndev)
    eng = make_engine(rank % ndev) if rank < g else None
    kw = {}
    if g > 1 and rank < g:
        uid = np.frombuffer(link.unique_id() if rank == 0 else bytes(128), np.uint8).copy()
        if rank == 0:
            for r in range(1, g):
                world.Send([uid, mpi.INT], dest=r, tag=RCCL_ID_TAG)
        else:
            world.Recv([uid, mpi.INT], source=0, tag=RCCL_ID_TAG)
        kw["counter"] = countmode.ShardCounter(eng, rank, g, link.allreduce(eng, uid.tobytes(), g, rank))
        kw["counter"].check_group()  # the communicator must sum exactly the G owners
    return eng, kw


def _mpiexec(a, mpi, size_l, verbose, log) -> int:
    import torch
    from .engine import Engine
    world = mpi.COMM_WORLD
    rank, size = world.Get_rank(), world.Get_size()
    ndev = max(torch.cuda.device_count(), 1)
    # list seed: explicit, or drawn on rank 0 and shared (the lists must agree)
    seed = np.array([a.seed if a.seed is not None else secrets.randbits(62)], np.int64)
    if rank == 0:
        for r in range(1, size):
            world.Send([seed, mpi.INT], dest=r, tag=RCCL_ID_TAG - 1)
    else:
        world.Recv([seed, mpi.INT], source=0, tag=RCCL_ID_TAG - 1)
    list_seed = int(seed[0])
    rng = np.random if a.seed is None else np.random.RandomState(a.seed * 1000 + rank)
    comm = comm_mod.EpochComm(world) if a.rounds == "epoch" else world
    kw = {}
    if a.mode == "count":
        eng, kw = count_owners(world, mpi, ndev, Engine, RcclLink)
        cls = countmode.CountParty
    else:
        eng = Engine(rank % ndev)
        cls = protocol.Party
    t0 = time.perf_counter()
    res = cls(comm, size_l, a.nDishonest, eng, rng, log, None, list_seed, **kw).run()
    _outcome(res, verbose)
    if a.timing and rank == 0:
        print(f"wall {time.perf_counter() - t0:.3f} s ({a.mode} mode, {size} ranks)")
    return 0


def _torchrun(a, size_l, verbose, log) -> int:
    """G torch ranks = G GPU owners; rank 0 hosts the protocol in-process."""
    import torch
    from . import distributed
    from .engine import Engine
    if a.mode != "count":
        raise SystemExit("torchrun launches shard the count pass: use --mode count")
    rank, local, world = distributed.init()
    eng = Engine(local)
    seed = torch.tensor([a.seed if a.seed is not None else secrets.randbits(62)], dtype=torch.int64,
                        device=eng.device)
    torch.distributed.broadcast(seed, 0)
    list_seed = int(seed.item())
    counter = countmode.ShardCounter(eng, rank, world, countmode.torch_allreduce, owners={0})
    counter.check_group()
    if rank != 0:
        counter.tables(a.parties, size_l, list_seed)
        return 0
    t0 = time.perf_counter()
    rank_seed = a.seed if a.seed is not None else secrets.randbits(20)
    run = protocol.run_local(a.parties, size_l, a.nDishonest, eng, seed=rank_seed, log=log,
                             party_cls=countmode.CountParty, timeout=600, list_seed=list_seed,
                             party_kwargs={"counter": counter})
    _outcome(run.result, verbose)
    if a.timing:
        print(f"wall {time.perf_counter() - t0:.3f} s (count mode, sizeL sharded over {world} GPUs)")
    return 1 if run.error else 0


def _montecarlo(a, eng, size_l) -> int:
    """--runs R: R independent count-mode instances decided on the device
    (montecarlo.run); one summary line, or with --curve one per sizeL
    (montecarlo.curve), or with --sweep one per sizeL and scenario
    (montecarlo.sweep), each the line of the --adversary run of that scenario,
    or with --grid one per sizeL and item (montecarlo.grid), each the line of
    the --adversary --drop run of that item."""
    from . import montecarlo
    seed = secrets.randbits(62) if a.seed is None else a.seed
    t0 = time.perf_counter()
    how = {"tally": True, "failures": a.failures} if a.tally or a.failures else {}
    if a.explain:
        how["explain"] = EXPLAIN_CAP
    if a.flip:
        how["flip_q16"] = a.flip
    noise = f" flip={a.flip}/65536" if a.flip else ""
    if a.adversary is not None:
        how["adversary"] = a.adversary
        noise += f" adversary={a.adversary:#x}"
    if a.collude is not None:
        how["coalition"] = a.collude
        noise += f" collude={a.collude:#x}"
    if a.drop is not None:
        how["net"] = a.drop
        noise += f" drop={a.drop & 0xFFFF}/65536" + (" cmd" if a.drop >> 16 else "")
    if a.noise is not None:
        how["noise"] = a.noise
        noise += f" noise={montecarlo.format_noise_profile(a.noise)}"
    if a.grid is not None:
        grid = montecarlo.grid(a.parties, a.curve if a.curve is not None else [size_l], a.grid, a.runs, seed, eng,
                               batch=a.batch, **how)
        points = {(c, k, f"{noise} adversary={word:#x}"
                   + (f" drop={net & 0xFFFF}/65536" + (" cmd" if net >> 16 else "") if net else "")): s
                  for (c, k, word, net), s in grid.items()}
    elif a.sweep is not None:
        grid = montecarlo.sweep(a.parties, a.curve if a.curve is not None else [size_l], a.sweep, a.runs, seed, eng,
                                batch=a.batch, **how)
        points = {(c, k, f"{noise} adversary={word:#x}"): s for (c, k, word), s in grid.items()}
    elif a.curve is not None:
        points = montecarlo.curve(a.parties, a.curve, a.nDishonest, a.runs, seed, eng, batch=a.batch, **how)
    else:
        points = {size_l: montecarlo.run(a.parties, size_l, a.nDishonest, a.runs, seed, eng, batch=a.batch,
                                         path="tables_noisy" if a.tables else "fused" if a.fused else "tables",
                                         **how)}
    for c, s in points.items():
        c, dis, tail = c if a.sweep is not None or a.grid is not None else (c, a.nDishonest, noise)
        print(f"Runs: {s['runs']} Successes: {s['successes']} Rate: {s['rate']:.6f} "
              f"(n={a.parties}, sizeL={c}, dishonest={dis}, empty-V_i runs={s['empty_vi_runs']}){tail}")
        if a.failures:
            print(f"Failed runs ({len(s['failed_runs'])} of {s['failed_total']}, key = seed + index, seed={seed}): "
                  + " ".join(str(i) for i in s["failed_runs"]))
        if a.explain:
            for i, row, counts, events in zip(s["failed_runs"], *s["trace"]):
                print(f"Run {i}:")
                print(montecarlo.format_trace(a.parties, row, counts, events))
    if a.timing:
        print(f"wall {time.perf_counter() - t0:.3f} s ({a.runs} instances on the device)")
    return 0


def _replay(a, eng, size_l) -> int:
    """--replay I,J,...: the transcripts of those runs of the --runs command
    with the same flags (montecarlo.replay), one per index, with --curve one
    per sizeL and index."""
    from . import montecarlo
    for c in a.curve if a.curve is not None else [size_l]:
        got = montecarlo.replay(a.parties, c, a.nDishonest, a.replay, a.seed, eng, flip_q16=a.flip or 0,
                                adversary=a.adversary, net=a.drop, cap=EXPLAIN_CAP)
        for i, row, counts, events in zip(got["indices"], got["rows"], got["counts"], got["events"]):
            print(f"sizeL={c} run {i}" if a.curve is not None else f"run {i}")
            print(montecarlo.format_trace(a.parties, row, counts, events))
    return 0


def main(argv=None) -> int:
    a = _args(sys.argv[1:] if argv is None else argv)
    size_l = int(a.sizeL)
    verbose = not a.quiet and size_l <= 100_000 and a.mode == "exact"
    log = print if verbose else None
    mpi = comm_mod.mpi_world()
    if mpi is not None and mpi.COMM_WORLD.Get_size() > 1:
        return _mpiexec(a, mpi, size_l, verbose, log)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return _torchrun(a, size_l, verbose, log)
    from .engine import Engine
    eng = Engine(0)
    if a.replay is not None:
        return _replay(a, eng, size_l)
    if a.runs is not None:
        return _montecarlo(a, eng, size_l)
    seed = secrets.randbits(20) if a.seed is None else a.seed
    list_seed = secrets.randbits(62) if a.seed is None else a.seed
    party_cls = countmode.CountParty if a.mode == "count" else protocol.Party
    t0 = time.perf_counter()
    run = protocol.run_local(a.parties, size_l, a.nDishonest, eng, seed=seed, log=log,
                             party_cls=party_cls, timeout=600, list_seed=list_seed,
                             party_kwargs={"wire": True} if a.wire else None)
    _outcome(run.result, verbose)
    if a.timing:
        print(f"wall {time.perf_counter() - t0:.3f} s ({a.mode} mode, in-process, {a.parties + 1} ranks)")
    if run.error:
        print(f"{run.error} (min of an empty V_i, tfg.py:306) on ranks {run.error_ranks}")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
