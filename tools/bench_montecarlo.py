#!/usr/bin/env python3
"""Where the time of BASELINE configs[3] as a Monte-Carlo run goes: 4096
instances x n = 7 x sizeL = 1e5, 2 dishonest, on one GPU.

  (a) sample_check_batched (nibble rows): lists + count tables of all instances
  (b) protocol_batched: every instance's rounds, decisions and success flag
  (c) the only route to the same answers without (b): montecarlo.run_host
      (CountParty under run_local, one instance at a time, on the GPU engine)
      over --host-instances instances, scaled to 4096 -- EXTRAPOLATED.

  (d) montecarlo_sampled: the fused path, lists to rows in one kernel with no
      list buffer and no tables -- the same rows as (a) + (b), which is
      checked; "a_plus_b" times (a) then (b) as one interval for comparison.
      --sizeL may be given several times (the fused path is meant for small
      ones); --host-instances 0 skips (c).

  --curve c0,c1,...  (repeatable) another mode: one montecarlo_curve_sampled
      call over the checkpoints against the K montecarlo_sampled calls at the
      same counts, the K timed as one interval; the rows of the two are compared
      at the timed shape.  One JSON line per --curve; nothing else is measured.

  --tally  another mode, per --sizeL: montecarlo_tally alone (with and without
      capturing failed runs), montecarlo_sampled followed by it, and as host
      wall time the two endings of a batch: tally + one [1, 32] copy +
      summary_from_tally against rows to host + summarize.

  --flip K  (repeatable) another mode, per --sizeL or per --curve: the noisy
      fused call (qba_montecarlo_sampled_noisy, or the noisy curve call) at each
      flip probability K / 65536 beside the noiseless call, which is timed first
      and again last in the same session; K = 0 goes through the noisy entry
      point and runs the noiseless kernel.  Reports noisy / noiseless at the
      medians and the Philox blocks per entry the noise adds.

  --flip K --tables  (per --sizeL and K) the noisy tables path beside the noisy
      fused call at the same shape, in one session: the noisy batched call
      (qba_sample_check_batched_packed_noisy, nibble rows), that call followed
      by protocol_batched as one interval, and qba_montecarlo_sampled_noisy.
      The rows of the two routes are compared; a route is called faster only
      where the min-max ranges are apart.

  --adversary NAME|0xHEX  (repeatable) another mode, per --sizeL: the fused call
      through the policy entry point (qba_montecarlo_sampled_adv) at the
      reference word 0xF -- the rows of the call without a policy, which is
      checked, so that column is the cost of the policy kernels' text -- and at
      each policy given, beside the call without a policy, which is timed first
      and again last in the same session.  Other policies run another protocol:
      their times are reported without a verdict.

  --sweep K:POLICY,...  (repeatable) another mode, per --sizeL and per --curve:
      one montecarlo_sweep_sampled call over the grid of scenarios (K traitors
      under POLICY; a bare POLICY takes --dishonest, a bare K the reference
      policy) against the S montecarlo_curve_sampled calls with adversary= of
      the same grid, the S timed as one interval; the rows of the two are
      compared at the timed shape.  One JSON line per --sweep and shape.

  --grid SCENARIO[@DROP[:cmd]],...  (repeatable) another mode, per --sizeL and
      per --curve: one montecarlo_grid_sampled call over the grid of items
      (SCENARIO as --sweep takes it, on the network DROP[:cmd]; tfg --grid's
      grammar) against the S montecarlo_curve_sampled_net calls of the same
      grid, the S timed as one interval; the rows of the two are compared at
      the timed shape, and the success counts of every slice are reported.  A
      call holds at most 32 slices: a grid past that (nine items on a ladder of
      four) goes in the fewest grid calls, timed as one interval ("grid_calls").
      One JSON line per --grid and shape.

  --collude NAME|0xHEX  (repeatable) another mode, per --sizeL: the coalition
      call (qba_montecarlo_curve_sampled_coal, one checkpoint) at coal = 0 -- the
      rows of the _adv curve call, which is checked -- and under each coalition
      word given, beside that _adv curve call, which is timed first and again
      last in the same session, under each of the policies reference and
      reorder_low (or those of --adversary).  A coalition runs another protocol:
      its times are reported without a verdict, its success counts beside them.

  --drop K[:cmd]  (repeatable) another mode, per --sizeL: the lossy-network
      call (qba_montecarlo_curve_sampled_net, one checkpoint) at net = 0 -- the
      rows of the _adv curve call, which is checked: unequal rows are an error
      -- and at each network word given (drop_q16 = K, with :cmd the
      commander's packets too), beside that _adv curve call, which is timed
      first and again last in the same session, under each of the policies
      reference and reorder_low (or those of --adversary).  A lossy network
      runs another protocol: its times are reported without a verdict, its
      success counts beside them.

  --noise all:K,G:K,...,depol:K  (repeatable) another mode, per --sizeL: the
      noise-profile call (qba_montecarlo_curve_sampled_nprof, one checkpoint)
      under each profile given, beside the _adv curve call at flip_q16 = the OR
      of the profile's rates (the same ladder steps; 0 for the all-zero and the
      depol-only profiles), which is timed first and again last in the same
      session.  A uniform profile without depol must give that call's rows:
      unequal rows are an error.  Every profile's success count stands beside
      its times.  --noise-split M adds the success counts with the total noise
      (n + 1) * M on all rows, on the commander's rows, on the honest parties'
      rows and on the traitors' rows of each instance.

  --trace  another mode, per --sizeL: the montecarlo_trace_sampled call at 16
      and at --instances indices (cap 256, the reference policy word) beside
      montecarlo_sampled(..., adversary=0xF) of the same number of instances --
      the yardstick: the trace is that call plus the event stores -- with the
      rows of the two compared, and the host wall time of montecarlo.trace_host
      for 16 runs on the engine's own count tables.
      With --drop K[:cmd] (repeatable): the montecarlo_trace_sampled_net call
      at net = 0 and at each network word, at 16 and at --instances indices,
      beside two calls whose code the build leaves as it was, timed in the same
      session: montecarlo_curve_sampled_net at one checkpoint over as many
      instances under the same word (rows compared), and
      montecarlo_trace_sampled at net = 0 (rows, counts and events compared).

(a), (b), (d), the --tally calls, the --flip calls and the --curve pair are device-event times of single calls on warm code: median, min
and max over --repeats launches after --warmup launches.  (c) is host wall
time around runs that end in device synchronisation (each reads its tables
back).  Prints one JSON line; --out also writes it to a file.  No GPU: fails.
"""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
PKG = "tfg---quantum-byzantine-agreement_amd"


def _events(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": repeats}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parties", type=int, default=7)
    ap.add_argument("--sizeL", type=int, action="append", default=None, help="default 100000; repeatable")
    ap.add_argument("--dishonest", type=int, default=2)
    ap.add_argument("--instances", type=int, default=4096)
    ap.add_argument("--host-instances", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--curve", action="append", default=None, metavar="C0,C1,...",
                    help="time one curve call against the separate calls at these counts; repeatable")
    ap.add_argument("--tally", action="store_true",
                    help="time montecarlo_tally alone, montecarlo_sampled followed by it, and the rows-to-host "
                         "ending it replaces, at each --sizeL; nothing else is measured")
    ap.add_argument("--flip", type=int, action="append", default=None, metavar="K",
                    help="time the noisy fused call (with --curve: the noisy curve call) at flip probability "
                         "K / 65536 beside the noiseless one; repeatable; nothing else is measured")
    ap.add_argument("--tables", action="store_true",
                    help="with --flip: time the noisy batched call, the same followed by protocol_batched, and the "
                         "noisy fused call at each --sizeL and K, and compare their rows")
    ap.add_argument("--adversary", action="append", default=None, metavar="NAME|0xHEX",
                    help="time montecarlo_sampled through the policy entry point at 0xF and at each policy given, "
                         "beside the call without a policy, at each --sizeL; repeatable; nothing else is measured")
    ap.add_argument("--sweep", action="append", default=None, metavar="K:POLICY,...",
                    help="time one sweep call over these scenarios against the separate curve calls with a policy, "
                         "at each --sizeL (one checkpoint) or each --curve; repeatable; nothing else is measured")
    ap.add_argument("--grid", action="append", default=None, metavar="SCENARIO[@DROP[:cmd]],...",
                    help="time one grid call over these items against the separate lossy-network curve calls, at "
                         "each --sizeL (one checkpoint) or each --curve; repeatable; nothing else is measured")
    ap.add_argument("--collude", action="append", default=None, metavar="NAME|0xHEX",
                    help="time the coalition call at coal = 0 and under each of these coalition words beside the "
                         "_adv curve call of one checkpoint, at each --sizeL, under the policies of --adversary "
                         "(default reference and reorder_low); nothing else is measured")
    ap.add_argument("--drop", action="append", default=None, metavar="K[:cmd]",
                    help="time the lossy-network call at net = 0 and at each of these network words beside the "
                         "_adv curve call of one checkpoint, at each --sizeL, under the policies of --adversary "
                         "(default reference and reorder_low); nothing else is measured")
    ap.add_argument("--noise", action="append", default=None, metavar="all:K,G:K,...,depol:K",
                    help="time the noise-profile call under each of these profiles beside the _adv curve call of one "
                         "checkpoint at flip_q16 = the OR of the profile's rates, at each --sizeL, under the first "
                         "policy of --adversary (default reference); repeatable; nothing else is measured")
    ap.add_argument("--noise-split", type=lambda t: int(t, 0), default=0, metavar="M",
                    help="with --noise: also the success counts with the total noise (n + 1) * M on all rows, on the "
                         "commander's rows, on the honest parties' rows and on the traitors' rows of each instance")
    ap.add_argument("--trace", action="store_true",
                    help="time montecarlo_trace_sampled at 16 and at --instances indices beside montecarlo_sampled "
                         "with the reference policy word at the same shapes, and the host wall time of trace_host "
                         "for 16 runs, at each --sizeL; with --drop: montecarlo_trace_sampled_net at net = 0 and at "
                         "each network word beside montecarlo_curve_sampled_net and montecarlo_trace_sampled; "
                         "nothing else is measured")
    a = ap.parse_args(argv)
    if a.noise and (a.trace or a.collude or a.drop or a.grid or a.sweep or a.flip or a.curve or a.tally or a.tables):
        ap.error("--noise goes with --sizeL, --adversary and --noise-split alone")
    if a.noise_split and not a.noise:
        ap.error("--noise-split needs --noise")
    if a.trace and (a.sweep or a.adversary or a.flip or a.curve or a.tally or a.tables):
        ap.error("--trace goes with --sizeL alone")
    if a.collude and (a.trace or a.sweep or a.flip or a.curve or a.tally or a.tables):
        ap.error("--collude goes with --sizeL and --adversary alone")
    if a.drop and (a.collude or a.sweep or a.flip or a.curve or a.tally or a.tables):
        ap.error("--drop goes with --sizeL and --adversary (or --trace) alone")
    if a.grid and (a.sweep or a.drop or a.collude or a.trace or a.flip or a.tally or a.tables or a.adversary):
        ap.error("--grid goes with --sizeL or --curve alone")
    if a.sweep and (a.flip or a.tally or a.tables or a.adversary):
        ap.error("--sweep goes with --sizeL or --curve alone")
    if a.adversary and (a.flip or a.curve or a.tally or a.tables):
        ap.error("--adversary goes with --sizeL alone")
    if a.tables and (not a.flip or a.curve or a.tally):
        ap.error("--tables needs --flip and goes with neither --curve nor --tally")

    eng = importlib.import_module(f"{PKG}.engine").Engine(0)
    if a.noise:
        lines = [json.dumps(_measure_noise(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    elif a.grid:
        shapes = [[s] for s in (a.sizeL or [])] + [sorted({int(c) for c in text.split(",")}) for text in a.curve or []]
        lines = [json.dumps(_measure_grid(a, eng, counts, text)) for text in a.grid for counts in shapes or [[100_000]]]
    elif a.trace and a.drop:
        lines = [json.dumps(_measure_nettrace(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    elif a.drop:
        lines = [json.dumps(_measure_drop(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    elif a.collude:
        lines = [json.dumps(_measure_collude(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    elif a.trace:
        lines = [json.dumps(_measure_trace(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    elif a.sweep:
        shapes = [[s] for s in (a.sizeL or [])] + [sorted({int(c) for c in text.split(",")}) for text in a.curve or []]
        lines = [json.dumps(_measure_sweep(a, eng, counts, text)) for text in a.sweep for counts in shapes or [[100_000]]]
    elif a.adversary:
        lines = [json.dumps(_measure_adversary(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    elif a.tables:
        lines = [json.dumps(_measure_flip_tables(a, eng, size_l, k)) for size_l in (a.sizeL or [100_000])
                 for k in a.flip]
    elif a.flip:
        shapes = ([sorted({int(c) for c in text.split(",")}) for text in a.curve] if a.curve
                  else [[s] for s in (a.sizeL or [100_000])])
        lines = [json.dumps(_measure_flip(a, eng, counts, bool(a.curve))) for counts in shapes]
    elif a.tally:
        lines = [json.dumps(_measure_tally(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    elif a.curve:
        lines = [json.dumps(_measure_curve(a, eng, sorted({int(c) for c in text.split(",")}))) for text in a.curve]
    else:
        lines = [json.dumps(_measure(a, eng, size_l)) for size_l in (a.sizeL or [100_000])]
    print("\n".join(lines))
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(lines) + "\n")
    eng.close()
    return 0


def _measure_curve(a, eng, counts) -> dict:
    import torch
    n, nd, inst = a.parties, a.dishonest, a.instances
    curve = eng.montecarlo_curve_sampled(n, nd, a.seed, inst, counts)
    single = torch.empty_like(curve)

    def separate():
        for j, c in enumerate(counts):
            eng.montecarlo_sampled(n, nd, a.seed, inst, c, single[j])

    separate()
    torch.cuda.synchronize()
    waves, lds, wgs = eng.montecarlo_curve_shape(n)
    res = {"config": {"n": n, "counts": counts, "dishonest": nd, "instances": inst, "seed": a.seed,
                      "device": torch.cuda.get_device_name(0), "entries_curve": counts[-1],
                      "entries_separate": sum(counts),
                      "curve_shape": {"waves": waves, "lds_bytes": lds, "wgs_per_cu": wgs}},
           "rows_equal_separate_calls": bool(torch.equal(curve, single))}
    res["separate_montecarlo_sampled"] = _events(separate, a.warmup, a.repeats)
    res["curve_montecarlo_curve_sampled"] = _events(
        lambda: eng.montecarlo_curve_sampled(n, nd, a.seed, inst, counts, curve), a.warmup, a.repeats)
    res["rows_equal_separate_calls"] = res["rows_equal_separate_calls"] and bool(torch.equal(curve, single))
    s, c = res["separate_montecarlo_sampled"], res["curve_montecarlo_curve_sampled"]
    res["separate_over_curve_at_median"] = s["median_ms"] / c["median_ms"]
    # faster only where the min-max ranges do not overlap
    res["curve_faster"] = c["max_ms"] < s["min_ms"]
    res["separate_faster"] = s["max_ms"] < c["min_ms"]
    return res


def _measure_sweep(a, eng, counts, text) -> dict:
    """--sweep: one sweep call against the separate policy curve calls of its grid."""
    import torch
    tfg = importlib.import_module(f"{PKG}.tfg")
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, inst = a.parties, a.instances
    scen = tfg._scenarios(text, a.dishonest, mc)
    sweep = eng.montecarlo_sweep_sampled(n, a.seed, inst, counts, scen)
    single = torch.empty((len(scen), len(counts), inst, sweep.shape[-1]), dtype=torch.int32, device=eng.device)

    def separate():
        for s, (k, word) in enumerate(scen):
            eng.montecarlo_curve_sampled(n, k, a.seed, inst, counts, single[s], adversary=word)

    def equal():
        return bool(torch.equal(sweep, single.transpose(0, 1)))

    separate()
    torch.cuda.synchronize()
    res = {"config": {"n": n, "counts": counts, "scenarios": [[k, f"{word:#x}"] for k, word in scen],
                      "instances": inst, "seed": a.seed, "device": torch.cuda.get_device_name(0),
                      "slices": len(counts) * len(scen), "entries_sweep": counts[-1],
                      "entries_separate": counts[-1] * len(scen)},
           "rows_equal_separate_calls": equal()}
    res["separate_montecarlo_curve_sampled_adv"] = _events(separate, a.warmup, a.repeats)
    res["sweep_montecarlo_sweep_sampled"] = _events(
        lambda: eng.montecarlo_sweep_sampled(n, a.seed, inst, counts, scen, sweep), a.warmup, a.repeats)
    res["rows_equal_separate_calls"] = res["rows_equal_separate_calls"] and equal()
    s, c = res["separate_montecarlo_curve_sampled_adv"], res["sweep_montecarlo_sweep_sampled"]
    res["separate_over_sweep_at_median"] = s["median_ms"] / c["median_ms"]
    # faster only where the min-max ranges do not overlap
    res["sweep_faster"] = c["max_ms"] < s["min_ms"]
    res["separate_faster"] = s["max_ms"] < c["min_ms"]
    return res


def _measure_grid(a, eng, counts, text) -> dict:
    """--grid: one grid call against the separate lossy-network curve calls of its items."""
    import torch
    tfg = importlib.import_module(f"{PKG}.tfg")
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, inst = a.parties, a.instances
    scen = tfg._grid_items(text, a.dishonest, mc)
    # a call holds at most 32 slices: a grid past that goes in the fewest calls, near-equal, timed as one interval
    calls = -(-len(counts) * len(scen) // eng.CURVE_MAX)
    if len(counts) * -(-len(scen) // calls) > eng.CURVE_MAX:
        calls += 1
    per = -(-len(scen) // calls)
    parts = [scen[i:i + per] for i in range(0, len(scen), per)]
    outs = [eng.montecarlo_grid_sampled(n, a.seed, inst, counts, part) for part in parts]
    single = torch.empty((len(scen), len(counts), inst, outs[0].shape[-1]), dtype=torch.int32, device=eng.device)

    def grid():
        for part, out in zip(parts, outs):
            eng.montecarlo_grid_sampled(n, a.seed, inst, counts, part, out)

    def separate():
        for s, (k, word, net) in enumerate(scen):
            eng.montecarlo_curve_sampled_net(n, k, a.seed, inst, counts, single[s], adversary=word, net=net)

    def equal():
        return bool(torch.equal(torch.cat(outs, dim=1), single.transpose(0, 1)))

    separate()
    torch.cuda.synchronize()
    res = {"config": {"n": n, "counts": counts, "scenarios": [[k, f"{word:#x}", f"{net:#x}"] for k, word, net in scen],
                      "instances": inst, "seed": a.seed, "device": torch.cuda.get_device_name(0),
                      "slices": len(counts) * len(scen), "grid_calls": len(parts),
                      "entries_grid": counts[-1] * len(parts), "entries_separate": counts[-1] * len(scen)},
           "rows_equal_separate_calls": equal()}
    res["separate_montecarlo_curve_sampled_net"] = _events(separate, a.warmup, a.repeats)
    res["grid_montecarlo_grid_sampled"] = _events(grid, a.warmup, a.repeats)
    res["rows_equal_separate_calls"] = res["rows_equal_separate_calls"] and equal()
    # successes of every slice, from the grid's rows: [checkpoint][item]
    res["successes"] = torch.cat(outs, dim=1)[..., 0].sum(dim=2).tolist()
    s, c = res["separate_montecarlo_curve_sampled_net"], res["grid_montecarlo_grid_sampled"]
    res["separate_over_grid_at_median"] = s["median_ms"] / c["median_ms"]
    # faster only where the min-max ranges do not overlap
    res["grid_faster"] = c["max_ms"] < s["min_ms"]
    res["separate_faster"] = s["max_ms"] < c["min_ms"]
    return res


def _measure_flip(a, eng, counts, curve: bool) -> dict:
    """--flip: the noisy call at each K beside the noiseless call of the same session."""
    import ctypes as C

    import torch
    em = importlib.import_module(f"{PKG}.engine")
    n, nd, inst = a.parties, a.dishonest, a.instances
    eng.prepare(n)
    shape = (len(counts), inst, 4 + 5 * (n + 1)) if curve else (inst, 4 + 5 * (n + 1))
    rows = torch.empty(shape, dtype=torch.int32, device=eng.device)
    cs = (C.c_uint32 * len(counts))(*counts)

    def noisy(k):  # the C entry point itself: the Engine sends k = 0 to the noiseless symbol
        if curve:
            em.call("qba_montecarlo_curve_sampled_noisy", eng.ctx, n, nd, a.seed, inst, cs, len(counts), k,
                    em._ptr(rows), eng.stream())
        else:
            em.call("qba_montecarlo_sampled_noisy", eng.ctx, n, nd, a.seed, inst, counts[0], k, em._ptr(rows),
                    eng.stream())

    def clean():
        if curve:
            eng.montecarlo_curve_sampled(n, nd, a.seed, inst, counts, rows)
        else:
            eng.montecarlo_sampled(n, nd, a.seed, inst, counts[0], rows)

    res = {"config": {"n": n, "counts" if curve else "sizeL": counts if curve else counts[0], "dishonest": nd,
                      "instances": inst, "seed": a.seed, "device": torch.cuda.get_device_name(0)}}
    res["noiseless"] = _events(clean, a.warmup, a.repeats)
    ref = rows.clone()
    res["flips"] = {}
    for k in a.flip:
        t = _events(lambda: noisy(k), a.warmup, a.repeats)
        t["noise_blocks_per_entry"] = 0 if k == 0 else (16 - ((k & -k).bit_length() - 1) + 1) // 2
        t["rows_equal_noiseless"] = bool(torch.equal(rows, ref))
        res["flips"][str(k)] = t
    res["noiseless_again"] = _events(clean, a.warmup, a.repeats)
    base = min(res["noiseless"]["median_ms"], res["noiseless_again"]["median_ms"])
    res["noiseless_spread_at_median"] = abs(res["noiseless"]["median_ms"] - res["noiseless_again"]["median_ms"]) / base
    for t in res["flips"].values():
        t["over_noiseless_at_median"] = t["median_ms"] / base
    return res


def _measure_adversary(a, eng, size_l) -> dict:
    """--adversary: the policy call at 0xF and at each policy beside the call without one."""
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, inst = a.parties, a.dishonest, a.instances
    rows = eng.montecarlo_sampled(n, nd, a.seed, inst, size_l)
    ref = rows.clone()
    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "instances": inst, "seed": a.seed,
                      "device": torch.cuda.get_device_name(0)}}
    res["no_policy"] = _events(lambda: eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, rows), a.warmup, a.repeats)
    res["policies"] = {}
    for name in ["reference"] + [p for p in a.adversary if p != "reference"]:
        word = mc.parse_adversary(name)
        t = _events(lambda: eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, rows, adversary=word), a.warmup,
                    a.repeats)
        t["word"] = f"{word:#x}"
        t["rows_equal_no_policy"] = bool(torch.equal(rows, ref))
        t["successes"] = int(rows[:, 0].sum())
        res["policies"][name] = t
    res["no_policy_again"] = _events(lambda: eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, rows), a.warmup,
                                     a.repeats)
    first, last = res["no_policy"], res["no_policy_again"]
    base = min(first["median_ms"], last["median_ms"])
    res["no_policy_spread_at_median"] = abs(first["median_ms"] - last["median_ms"]) / base
    for t in res["policies"].values():
        t["over_no_policy_at_median"] = t["median_ms"] / base
    r = res["policies"]["reference"]
    lo, hi = min(first["min_ms"], last["min_ms"]), max(first["max_ms"], last["max_ms"])
    # a verdict only for 0xF (equal rows), and only where the min-max ranges do not overlap
    res["reference_word_slower"] = r["min_ms"] > hi
    res["reference_word_faster"] = r["max_ms"] < lo
    return res


def _measure_collude(a, eng, size_l) -> dict:
    """--collude: per policy, the _adv curve call of one checkpoint first and last, the coalition call at
    coal = 0 (equal rows, checked) and under each coalition word between them."""
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, inst = a.parties, a.dishonest, a.instances
    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "instances": inst, "seed": a.seed,
                      "device": torch.cuda.get_device_name(0)}, "policies": {}}
    for policy in a.adversary or ["reference", "reorder_low"]:
        adv = mc.parse_adversary(policy)
        rows = eng.montecarlo_curve_sampled(n, nd, a.seed, inst, [size_l], adversary=adv)
        ref = rows.clone()
        parent = lambda: eng.montecarlo_curve_sampled(n, nd, a.seed, inst, [size_l], rows, adversary=adv)  # noqa: E731
        r = {"word": f"{adv:#x}", "adv_curve_call": _events(parent, a.warmup, a.repeats), "coalitions": {}}
        r["adv_curve_call"]["successes"] = int(ref[0, :, 0].sum())
        for name in ["0"] + [c for c in a.collude if c != "0"]:
            coal = mc.parse_coalition(name)
            t = _events(lambda: eng.montecarlo_curve_sampled_coal(n, nd, a.seed, inst, [size_l], rows, adversary=adv,
                                                                  coalition=coal), a.warmup, a.repeats)
            t["word"] = f"{coal:#x}"
            t["rows_equal_adv_curve_call"] = bool(torch.equal(rows, ref))
            t["successes"] = int(rows[0, :, 0].sum())
            r["coalitions"][name] = t
        r["adv_curve_call_again"] = _events(parent, a.warmup, a.repeats)
        first, last = r["adv_curve_call"], r["adv_curve_call_again"]
        base = min(first["median_ms"], last["median_ms"])
        r["adv_curve_call_spread_at_median"] = abs(first["median_ms"] - last["median_ms"]) / base
        for t in r["coalitions"].values():
            t["over_adv_curve_call_at_median"] = t["median_ms"] / base
        z = r["coalitions"]["0"]
        lo, hi = min(first["min_ms"], last["min_ms"]), max(first["max_ms"], last["max_ms"])
        # a verdict only for coal = 0 (equal rows), and only where the min-max ranges do not overlap
        r["no_coalition_ranges_overlap"] = not (z["min_ms"] > hi or z["max_ms"] < lo)
        r["no_coalition_slower"] = z["min_ms"] > hi
        r["no_coalition_faster"] = z["max_ms"] < lo
        res["policies"][policy] = r
    return res


def _measure_drop(a, eng, size_l) -> dict:
    """--drop: per policy, the _adv curve call of one checkpoint first and last, the lossy-network call at
    net = 0 (equal rows, or an error) and at each network word between them."""
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, inst = a.parties, a.dishonest, a.instances
    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "instances": inst, "seed": a.seed,
                      "device": torch.cuda.get_device_name(0)}, "policies": {}}
    for policy in a.adversary or ["reference", "reorder_low"]:
        adv = mc.parse_adversary(policy)
        rows = eng.montecarlo_curve_sampled(n, nd, a.seed, inst, [size_l], adversary=adv)
        ref = rows.clone()
        parent = lambda: eng.montecarlo_curve_sampled(n, nd, a.seed, inst, [size_l], rows, adversary=adv)  # noqa: E731
        r = {"word": f"{adv:#x}", "adv_curve_call": _events(parent, a.warmup, a.repeats), "nets": {}}
        r["adv_curve_call"]["successes"] = int(ref[0, :, 0].sum())
        for name in ["0"] + [w for w in a.drop if mc.parse_net(w)]:
            word = mc.parse_net(name)
            t = _events(lambda: eng.montecarlo_curve_sampled_net(n, nd, a.seed, inst, [size_l], rows, adversary=adv,
                                                                 net=word), a.warmup, a.repeats)
            t["word"] = f"{word:#x}"
            t["rows_equal_adv_curve_call"] = bool(torch.equal(rows, ref))
            if not word and not t["rows_equal_adv_curve_call"]:
                raise SystemExit(f"net = 0 does not give the _adv curve call's rows (n={n}, sizeL={size_l}, {policy})")
            t["successes"] = int(rows[0, :, 0].sum())
            t["empty_vi_runs"] = int((rows[0, :, 2] != 0).sum())
            r["nets"][name] = t
        r["adv_curve_call_again"] = _events(parent, a.warmup, a.repeats)
        first, last = r["adv_curve_call"], r["adv_curve_call_again"]
        base = min(first["median_ms"], last["median_ms"])
        r["adv_curve_call_spread_at_median"] = abs(first["median_ms"] - last["median_ms"]) / base
        for t in r["nets"].values():
            t["over_adv_curve_call_at_median"] = t["median_ms"] / base
        z = r["nets"]["0"]
        lo, hi = min(first["min_ms"], last["min_ms"]), max(first["max_ms"], last["max_ms"])
        # a verdict only for net = 0 (equal rows), and only where the min-max ranges do not overlap
        r["perfect_network_ranges_overlap"] = not (z["min_ms"] > hi or z["max_ms"] < lo)
        r["perfect_network_slower"] = z["min_ms"] > hi
        r["perfect_network_faster"] = z["max_ms"] < lo
        res["policies"][policy] = r
    return res


def _measure_noise(a, eng, size_l) -> dict:
    """--noise: per profile, the noise-profile call beside the _adv curve call of one checkpoint at
    flip_q16 = the OR of the profile's rates (the same ladder steps and Philox blocks; 0 for the all-zero and the
    depol-only profiles).  Every baseline is timed first, and again last; a uniform profile without depol must give
    its baseline's rows.  With --noise-split M: the success counts with the total noise (n + 1) * M on all rows, on
    the commander's rows 0 and 1, on the honest parties' rows and on the traitors' rows of each instance (one call
    per instance: the traitors differ from key to key)."""
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, inst = a.parties, a.dishonest, a.instances
    adv = mc.parse_adversary((a.adversary or ["reference"])[0])
    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "instances": inst, "seed": a.seed, "adv": f"{adv:#x}",
                      "device": torch.cuda.get_device_name(0)}, "baselines": {}, "profiles": {}}
    profs = {mc.format_noise_profile(p): p for p in (mc.parse_noise_profile(n, s) for s in a.noise)}
    k_of = lambda p: int(np.bitwise_or.reduce(np.array(p[0])))  # noqa: E731
    rows = eng.montecarlo_curve_sampled(n, nd, a.seed, inst, [size_l], adversary=adv)
    refs = {}

    def base(k):
        return lambda: eng.montecarlo_curve_sampled(n, nd, a.seed, inst, [size_l], rows, flip_q16=k, adversary=adv)
    for k in sorted({k_of(p) for p in profs.values()}):
        t = _events(base(k), a.warmup, a.repeats)
        refs[k] = rows.clone()
        t["successes"] = int(rows[0, :, 0].sum())
        res["baselines"][f"{k:#x}"] = {"first": t}
    for name, p in profs.items():
        k = k_of(p)
        t = _events(lambda: eng.montecarlo_curve_sampled_nprof(n, nd, a.seed, inst, [size_l], rows, adversary=adv,
                                                               noise=p), a.warmup, a.repeats)
        t["baseline_flip_q16"] = f"{k:#x}"
        t["successes"] = int(rows[0, :, 0].sum())
        t["empty_vi_runs"] = int((rows[0, :, 2] != 0).sum())
        if len(set(p[0])) == 1 and not p[1]:
            t["rows_equal_baseline"] = bool(torch.equal(rows, refs[k]))
            if not t["rows_equal_baseline"]:
                raise SystemExit(f"the uniform profile {name} does not give the _adv curve call's rows at "
                                 f"flip_q16={k:#x} (n={n}, sizeL={size_l})")
        res["profiles"][name] = t
    for k in sorted({k_of(p) for p in profs.values()}):
        b = res["baselines"][f"{k:#x}"]
        b["last"] = _events(base(k), a.warmup, a.repeats)
        lo_med = min(b["first"]["median_ms"], b["last"]["median_ms"])
        b["spread_at_median"] = abs(b["first"]["median_ms"] - b["last"]["median_ms"]) / lo_med
        lo, hi = min(b["first"]["min_ms"], b["last"]["min_ms"]), max(b["first"]["max_ms"], b["last"]["max_ms"])
        for t in res["profiles"].values():
            if t["baseline_flip_q16"] == f"{k:#x}":
                t["over_baseline_at_median"] = t["median_ms"] / lo_med
                t["ranges_overlap"] = not (t["min_ms"] > hi or t["max_ms"] < lo)
    if a.noise_split:
        m, total = a.noise_split, (n + 1) * a.noise_split
        clean = eng.montecarlo_curve_sampled(n, nd, a.seed, inst, [size_l], adversary=adv).cpu().numpy()[0]
        owner = [1, 1] + list(range(2, n + 1))  # the party a list row belongs to
        split = {"mean_rate": f"{m:#x}"}

        def count(rows_of):
            one = torch.empty((1, 1, 4 + 5 * (n + 1)), dtype=torch.int32, device=eng.device)
            acc = torch.zeros((), dtype=torch.int64, device=eng.device)
            for i in range(inst):
                pick = rows_of(int(clean[i, 1]))
                rate = min(total // len(pick), 0xFFFF) if pick else 0
                prof = mc.noise_profile(n, 0, {g: rate for g in pick})
                eng.montecarlo_curve_sampled_nprof(n, nd, a.seed + i, 1, [size_l], one, adversary=adv, noise=prof)
                acc += one[0, 0, 0]
            return int(acc.item())
        split["uniform"] = count(lambda dis: list(range(n + 1)))
        split["commander_only"] = count(lambda dis: [0, 1])
        split["honest_only"] = count(lambda dis: [g for g in range(n + 1) if not (dis >> owner[g]) & 1])
        split["traitors_only"] = count(lambda dis: [g for g in range(n + 1) if (dis >> owner[g]) & 1])
        split["noiseless"] = int(clean[:, 0].sum())
        res["split"] = split
    return res


def _measure_trace(a, eng, size_l) -> dict:
    """--trace: the trace call at 16 and at --instances indices beside the
    decision call under the reference word at the same shapes (the yardstick:
    the trace is that call plus the event stores), and trace_host for 16 runs."""
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, cap = a.parties, a.dishonest, 256
    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "seed": a.seed, "cap": cap, "adversary": "0xf",
                      "device": torch.cuda.get_device_name(0)}, "indices": {}}
    for k in sorted({16, a.instances}):
        idx = torch.arange(k, dtype=torch.int64, device=eng.device)
        out = eng.montecarlo_trace_sampled(n, nd, a.seed, idx, size_l, cap=cap)
        rows = eng.montecarlo_sampled(n, nd, a.seed, k, size_l, adversary=0xF)
        t = {"trace": _events(lambda: eng.montecarlo_trace_sampled(n, nd, a.seed, idx, size_l, cap=cap, out=out),
                              a.warmup, a.repeats),
             "decide": _events(lambda: eng.montecarlo_sampled(n, nd, a.seed, k, size_l, rows, adversary=0xF),
                               a.warmup, a.repeats)}
        t["rows_equal"] = bool(torch.equal(out[0], rows))
        t["events_per_instance"] = float(out[1].sum().item()) / k
        t["events_past_cap"] = int((out[1] > cap).sum().item())
        t["trace_over_decide_at_median"] = t["trace"]["median_ms"] / t["decide"]["median_ms"]
        res["indices"][str(k)] = t
    t0 = time.perf_counter()  # the host specification on the engine's own count tables
    host = mc.trace_host(n, size_l, nd, range(16), a.seed, eng)
    res["trace_host_16_runs_wall_s"] = time.perf_counter() - t0
    dev = eng.montecarlo_trace_sampled(n, nd, a.seed, list(range(16)), size_l, cap=cap)
    res["trace_host_rows_equal_device"] = bool((dev[0].cpu().numpy() == host[0]).all())
    return res


def _measure_nettrace(a, eng, size_l) -> dict:
    """--trace --drop: the lossy-network trace call at net = 0 and at each
    network word, at 16 and at --instances indices, beside the lossy-network
    decision call of one checkpoint under the same word and beside the trace
    call on the perfect network."""
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, cap = a.parties, a.dishonest, 256
    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "seed": a.seed, "cap": cap, "adversary": "0xf",
                      "device": torch.cuda.get_device_name(0)}, "indices": {}}
    words = [0] + [w for w in (mc.parse_net(x) for x in a.drop) if w]
    for k in sorted({16, a.instances}):
        idx = torch.arange(k, dtype=torch.int64, device=eng.device)
        ref = eng.montecarlo_trace_sampled(n, nd, a.seed, idx, size_l, cap=cap)
        out = tuple(torch.zeros_like(t) for t in ref)
        rows = eng.montecarlo_curve_sampled_net(n, nd, a.seed, k, [size_l], adversary=0xF)
        r = {"trace": _events(lambda: eng.montecarlo_trace_sampled(n, nd, a.seed, idx, size_l, cap=cap, out=ref),
                              a.warmup, a.repeats), "nets": {}}
        for word in words:
            t = {"nettrace": _events(lambda: eng.montecarlo_trace_sampled_net(n, nd, a.seed, idx, size_l, cap=cap,
                                                                              out=out, net=word),
                                     a.warmup, a.repeats),
                 "decide_net": _events(lambda: eng.montecarlo_curve_sampled_net(n, nd, a.seed, k, [size_l], rows,
                                                                                adversary=0xF, net=word),
                                       a.warmup, a.repeats)}
            t["rows_equal_decide_net"] = bool(torch.equal(out[0], rows[0]))
            if not t["rows_equal_decide_net"]:
                raise SystemExit(f"the traced rows are not the decision call's (n={n}, sizeL={size_l}, net={word:#x})")
            if not word:
                t["equal_trace_call"] = all(bool(torch.equal(x, y)) for x, y in zip(out, ref))
                if not t["equal_trace_call"]:
                    raise SystemExit(f"net = 0 does not give the trace call's outputs (n={n}, sizeL={size_l})")
            t["successes"] = int(out[0][:, 0].sum())
            t["events_per_instance"] = float(out[1].sum().item()) / k
            t["events_past_cap"] = int((out[1] > cap).sum().item())
            t["nettrace_over_decide_net_at_median"] = t["nettrace"]["median_ms"] / t["decide_net"]["median_ms"]
            t["nettrace_over_trace_at_median"] = t["nettrace"]["median_ms"] / r["trace"]["median_ms"]
            for other in ("decide_net", "trace") if not word else ("decide_net",):
                o = t[other] if other == "decide_net" else r["trace"]
                t[f"ranges_overlap_{other}"] = not (t["nettrace"]["min_ms"] > o["max_ms"] or
                                                    t["nettrace"]["max_ms"] < o["min_ms"])
            r["nets"][f"{word:#x}"] = t
        r["trace_again"] = _events(lambda: eng.montecarlo_trace_sampled(n, nd, a.seed, idx, size_l, cap=cap, out=ref),
                                   a.warmup, a.repeats)
        res["indices"][str(k)] = r
    return res


def _measure_flip_tables(a, eng, size_l, k) -> dict:
    """--flip K --tables: the noisy tables path against the noisy fused call."""
    import torch
    n, nd, inst = a.parties, a.dishonest, a.instances
    lists, counts = eng.sample_check_batched(n, a.seed, inst, size_l, packed=True, flip_q16=k)
    out = eng.protocol_batched(n, nd, a.seed, counts)
    fused = eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, flip_q16=k)
    torch.cuda.synchronize()

    def batched():
        return eng.sample_check_batched(n, a.seed, inst, size_l, lists, packed=True, flip_q16=k)

    def both():
        _, c = batched()
        eng.protocol_batched(n, nd, a.seed, c, out)

    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "instances": inst, "seed": a.seed, "flip_q16": k,
                      "noise_blocks_per_entry": 0 if k == 0 else (16 - ((k & -k).bit_length() - 1) + 1) // 2,
                      "device": torch.cuda.get_device_name(0)}}
    res["noisy_batched"] = _events(batched, a.warmup, a.repeats)
    res["noisy_batched_plus_protocol"] = _events(both, a.warmup, a.repeats)
    res["fused_noisy"] = _events(lambda: eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, fused, flip_q16=k),
                                 a.warmup, a.repeats)
    res["rows_equal"] = bool(torch.equal(out, fused))
    t, f = res["noisy_batched_plus_protocol"], res["fused_noisy"]
    res["fused_over_tables_at_median"] = f["median_ms"] / t["median_ms"]
    # faster only where the min-max ranges do not overlap
    res["tables_faster"] = t["max_ms"] < f["min_ms"]
    res["fused_faster"] = f["max_ms"] < t["min_ms"]
    return res


def _walls(fn, warmup, repeats):
    """Host wall time of calls that end synchronised (they read results back)."""
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": repeats}


def _measure_tally(a, eng, size_l) -> dict:
    """--tally: the ending of a Monte-Carlo batch both ways, on the fused path."""
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, inst = a.parties, a.dishonest, a.instances
    rows = eng.montecarlo_sampled(n, nd, a.seed, inst, size_l)
    tally = torch.zeros((1, mc.TALLY_WORDS), dtype=torch.int64, device=eng.device)
    capture = torch.zeros((1, 64), dtype=torch.int64, device=eng.device)

    def decide_and_tally():
        eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, rows)
        eng.montecarlo_tally(n, rows, tally)

    def ending_tally():
        tally.zero_()
        decide_and_tally()
        return mc.summary_from_tally(n, tally.cpu().numpy()[0])

    def ending_rows():
        eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, rows)
        return mc.summarize(n, rows.cpu().numpy())

    want = ending_rows()
    got = ending_tally()
    res = {"config": {"n": n, "sizeL": size_l, "dishonest": nd, "instances": inst, "seed": a.seed,
                      "device": torch.cuda.get_device_name(0), "row_bytes": int(rows.numel()) * 4},
           "result": {k: want[k] for k in ("runs", "successes", "rate", "empty_vi_runs")},
           "summaries_equal": all(got[k] == want[k] for k in want)}
    # device-event times of the asynchronous calls
    res["decision_montecarlo_sampled"] = _events(lambda: eng.montecarlo_sampled(n, nd, a.seed, inst, size_l, rows),
                                                 a.warmup, a.repeats)
    res["tally_alone"] = _events(lambda: eng.montecarlo_tally(n, rows, tally), a.warmup, a.repeats)
    res["tally_alone_capturing_failed"] = _events(
        lambda: eng.montecarlo_tally(n, rows, tally, select=mc.SEL_FAILED, capture=capture), a.warmup, a.repeats)
    res["decision_plus_tally"] = _events(decide_and_tally, a.warmup, a.repeats)
    res["tally_over_decision_at_median"] = (res["tally_alone"]["median_ms"] /
                                            res["decision_montecarlo_sampled"]["median_ms"])
    # host wall times of the two endings, result on the host
    res["wall_decision_tally_summary"] = _walls(ending_tally, a.warmup, a.repeats)
    res["wall_decision_rows_to_host_summarize"] = _walls(ending_rows, a.warmup, a.repeats)
    return res


def _measure(a, eng, size_l) -> dict:
    import torch
    mc = importlib.import_module(f"{PKG}.montecarlo")
    n, nd, inst = a.parties, a.dishonest, a.instances
    a = argparse.Namespace(**{**vars(a), "sizeL": size_l})
    lists, counts = eng.sample_check_batched(n, a.seed, inst, a.sizeL, packed=True)
    out = eng.protocol_batched(n, nd, a.seed, counts)
    torch.cuda.synchronize()

    res = {"config": {"n": n, "sizeL": a.sizeL, "dishonest": nd, "instances": inst, "seed": a.seed,
                      "device": torch.cuda.get_device_name(0)}}
    res["a_sample_check_batched_packed"] = _events(
        lambda: eng.sample_check_batched(n, a.seed, inst, a.sizeL, lists, packed=True), a.warmup, a.repeats)
    res["b_protocol_batched"] = _events(lambda: eng.protocol_batched(n, nd, a.seed, counts, out), a.warmup,
                                        a.repeats)
    table_bytes = 8 * inst * sum(int(t[0].numel()) for t in (counts.H, counts.C, counts.P))
    res["b_protocol_batched"]["table_bytes_read"] = table_bytes
    res["b_protocol_batched"]["table_GBps_at_median"] = table_bytes / res["b_protocol_batched"]["median_ms"] / 1e6
    summary = mc.summarize(n, out.cpu().numpy())
    res["result"] = {k: summary[k] for k in ("runs", "successes", "rate", "empty_vi_runs")}

    def both():
        eng.sample_check_batched(n, a.seed, inst, a.sizeL, lists, packed=True)
        eng.protocol_batched(n, nd, a.seed, counts, out)

    res["a_plus_b"] = _events(both, a.warmup, a.repeats)
    fused = eng.montecarlo_sampled(n, nd, a.seed, inst, a.sizeL)
    res["d_montecarlo_sampled"] = _events(lambda: eng.montecarlo_sampled(n, nd, a.seed, inst, a.sizeL, fused),
                                          a.warmup, a.repeats)
    res["d_montecarlo_sampled"]["rows_equal_tables_path"] = bool(torch.equal(fused, out))
    # faster only where the min-max ranges do not overlap
    res["d_faster_than_a_plus_b"] = res["d_montecarlo_sampled"]["max_ms"] < res["a_plus_b"]["min_ms"]
    res["a_plus_b_faster_than_d"] = res["a_plus_b"]["max_ms"] < res["d_montecarlo_sampled"]["min_ms"]

    k = a.host_instances
    if k <= 0:
        return res
    mc.run_host(n, a.sizeL, nd, 2, a.seed, eng)  # warm
    t0 = time.perf_counter()
    host = mc.run_host(n, a.sizeL, nd, k, a.seed, eng)
    wall = time.perf_counter() - t0
    res["c_run_host_gpu_engine"] = {"instances": k, "wall_s": wall, "per_instance_ms": 1e3 * wall / k,
                                    "extrapolated_to_instances": inst,
                                    "extrapolated_s": wall / k * inst, "extrapolated": True,
                                    "rows_equal_kernel": bool((host == out[:k].cpu().numpy()).all())}
    res["b_below_a"] = res["b_protocol_batched"]["median_ms"] < res["a_sample_check_batched_packed"]["median_ms"]
    return res


if __name__ == "__main__":
    sys.exit(main())
