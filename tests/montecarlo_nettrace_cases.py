"""What tests/test_montecarlo_nettrace.py (CPU) and
tests/test_gpu_montecarlo_nettrace.py (GPU) share: montecarlo.trace_net_host of
the reach sets of tests/montecarlo_net_cases.py and of one more key range,
computed once per process, and the helpers that read its events.  TEST
INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from conftest import sub
from montecarlo_net_cases import REACH
from test_montecarlo_adversary import HostEngine

_SEQ4 = REACH["n15-d8-L96-dup_cmd-sixteenth"]
# The reach sets and one more key range: at loss 1/16 none of the 18 sends with seq >= 4 of the dup_cmd
# set's own 8 keys is lost; under the keys 0x80 further on (the same injected lists) three are.
CASES = {**REACH, "n15-d8-L96-dup_cmd-sixteenth+0x80": _SEQ4[:3] + (_SEQ4[3] + 0x80,) + _SEQ4[4:]}
SAMPLED = [name for name, c in CASES.items() if c[5] is None]   # the four sets without injected lists
LISTS = [name for name, c in CASES.items() if c[5] is not None]  # the hostile ones
DUP = ("n7-d4-L60-dup_all-half", "n15-d8-L96-dup_cmd-sixteenth")
CAP = 1024


@functools.lru_cache(maxsize=None)
def reach_trace(name, flip_q16=0):
    """trace_net_host of all keys of a reach set: (rows, counts, events), read-only."""
    n, nd, sizeL, base, inst, lists, adv, word, _ = CASES[name]
    rows, counts, events = sub("montecarlo").trace_net_host(n, sizeL, nd, range(inst), base, HostEngine(), lists=lists,
                                                            flip_q16=flip_q16, adversary=adv, net=word)
    rows.setflags(write=False)
    counts.setflags(write=False)
    return rows, counts, events


def case_rows(name, party_cls=None):
    """run_host of a case on its network (montecarlo_net_cases.reach_rows, for CASES)"""
    n, nd, sizeL, base, inst, lists, adv, word, _ = CASES[name]
    return sub("montecarlo").run_host(n, sizeL, nd, inst, base, HostEngine(), lists=lists, adversary=adv,
                                      party_cls=party_cls, net=word)


def fields(per_rank):
    """[(fields, pkt)] of one rank's events"""
    mc = sub("montecarlo")
    return [(mc.event_fields(h), p) for h, p in per_rank]


def device_layout(n, counts, events, cap):
    """The host events as the device stores them: uint32 [k, n+1, cap, 2], the
    first ``cap`` of each rank, zeros behind them."""
    dev = np.zeros((len(events), n + 1, cap, 2), np.uint32)
    for j, inst in enumerate(events):
        for r, ev in enumerate(inst):
            if ev:
                dev[j, r, :min(len(ev), cap)] = np.array(ev[:cap], np.uint32).reshape(-1, 2)
    return dev
