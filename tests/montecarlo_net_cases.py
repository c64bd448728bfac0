"""Parameter sets and the observing party shared by tests/test_montecarlo_net.py
(CPU: what the host model montecarlo.NetParty reaches on them) and
tests/test_gpu_montecarlo_net.py (GPU: both lossy-network kernels == the host
model on them).  TEST INFRASTRUCTURE ONLY."""
import threading

import numpy as np

from montecarlo_cases import HOSTILE, hostile_lists
from test_montecarlo_adversary import HostEngine, PRESETS

CMD = 1 << 16
FIVE = 0x1F  # the five-action policy word
_DUP7 = next(c for c in HOSTILE if c["name"] == "n7-d4-L60-dup_all")
_CMD15 = next(c for c in HOSTILE if c["name"] == "n15-d8-L96-dup_cmd")  # six packets in one (source, destination, round)

REACH_BASE, REACH_KEYS = 0x4E47, 24
# name -> (n, n_dishonest, sizeL, seed_base, instances, injected lists or None, policy word, network word,
#          the events of observing() the set was chosen for)
REACH = {
    "n4-d1-L16-half": (4, 1, 16, REACH_BASE, REACH_KEYS, None, 0xF, 0x8000, ("mixed", "broken", "vi_only")),
    "n7-d2-L8-quarter": (7, 2, 8, REACH_BASE, REACH_KEYS, None, 0xF, 0x4000,
                         ("mixed", "vi_only", "mutated_lost")),
    "n7-d4-L60-dup_all-half": (7, 4, 60, _DUP7["base"], _DUP7["keys"], hostile_lists(_DUP7), 0xF, 0x8000,
                               ("mixed", "broken", "mutated_lost")),
    "n15-d8-L96-dup_cmd-sixteenth": (15, 8, 96, _CMD15["base"], _CMD15["keys"], hostile_lists(_CMD15), 0xF, 0x1000,
                                     ("seq4", "mixed")),
    "n7-d2-L8-cmd-half": (7, 2, 8, REACH_BASE, REACH_KEYS, None, 0xF, 0x8000 | CMD,
                          ("cmd_lost", "cmd_relayed", "mixed")),
    "n4-d1-L16-cmd-most": (4, 1, 16, REACH_BASE, REACH_KEYS, None, PRESETS["reorder_low"], 0xC000 | CMD,
                           ("cmd_lost", "cmd_empty", "broken")),
}
# every event the model is asked to reach
EVENTS = ("mixed", "seq4", "broken", "vi_only", "cmd_relayed", "cmd_empty", "mutated_lost")


def reach_rows(mc, name, counts=None, party_cls=None, net=True):
    """run_host (or, with ``counts``, curve_host) of a reach set; ``net=False``: on the perfect network."""
    n, nd, sizeL, base, inst, lists, adv, word, _ = REACH[name]
    kw = {"net": word} if net else {}
    if counts is not None:
        return mc.curve_host(n, counts, nd, inst, base, HostEngine(), lists=lists, adversary=adv, **kw)
    return mc.run_host(n, sizeL, nd, inst, base, HostEngine(), lists=lists, adversary=adv, party_cls=party_cls, **kw)


_LOCK = threading.Lock()  # the ranks of a run are threads


def observing(mc, seen):
    """A NetParty subclass for run_host's party_cls seam that records into
    ``seen`` what the parties of all instances do:

    ``handed``   {(key, rank): packets handed to a link, lost ones included}
    ``links``    {(key, rank, epoch): [handed, lost]}
    ``seq4``     sends on a lossy link with seq >= 4 (the second Philox block)
    ``mutated_lost``  lost packets of a dishonest lieutenant that differ from
                 the packet its broadcast was handed
    ``cmd_lost`` {(key, rank)}: lieutenants whose commander packet was lost
    """
    seen.update({"handed": {}, "links": {}, "seq4": 0, "mutated_lost": 0, "cmd_lost": set()})

    class Observed(mc.NetParty):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self._given = None

        def lieu_broadcast(self, P, v, L):
            self._given = (P.u, int(v), frozenset(L))
            super().lieu_broadcast(P, v, L)

        def send(self, dest, P, v, L):
            key, e = int(self.seed), self._epoch
            with _LOCK:
                seen["handed"][key, self.rank] = seen["handed"].get((key, self.rank), 0) + 1
                seen["links"].setdefault((key, self.rank, e), [0, 0])[0] += 1
                seen["seq4"] += self.lossy(dest) and self._seq.get((e, dest), 0) >= 4
            super().send(dest, P, v, L)

        def lose(self, dest, P, v, L, epoch, seq):
            assert mc.net_lost(self.seed, epoch, self.rank, dest, seq, self.net & 0xFFFF)
            with _LOCK:
                seen["links"][int(self.seed), self.rank, epoch][1] += 1
                if self.rank >= 2 and self.dishonest:
                    seen["mutated_lost"] += (P.u, int(v), frozenset(L)) != self._given
            super().lose(dest, P, v, L, epoch, seq)

        def recv(self, src):
            got = super().recv(src)
            if got[0] is mc.NetLost:
                with _LOCK:
                    seen["cmd_lost"].add((int(self.seed), self.rank))
            return got

    return Observed


def reach_events(n, base, rows, plain, seen):
    """The counts of EVENTS (and ``cmd_lost``) from what observing() recorded
    and the rows of the same keys with (``rows``) and without (``plain``) loss."""
    ev = {"seq4": int(seen["seq4"]), "mutated_lost": int(seen["mutated_lost"]), "cmd_lost": len(seen["cmd_lost"])}
    ev["mixed"] = sum(0 < lost < handed for handed, lost in seen["links"].values())
    ev["broken"] = int(((plain[:, 0] == 1) & (rows[:, 0] == 0)).sum())
    vi = 5 + 5 * np.arange(2, n + 1)
    honest = ((rows[:, 1:2] >> np.arange(2, n + 1)) & 1) == 0
    ev["vi_only"] = int((((rows[:, vi] != plain[:, vi]) & honest).any(axis=1) & (rows[:, 0] == plain[:, 0])).sum())
    ev["cmd_relayed"] = ev["cmd_empty"] = 0
    for key, rank in seen["cmd_lost"]:
        row = rows[key - base]
        if not (row[1] >> rank) & 1:
            ev["cmd_relayed" if row[5 + 5 * rank] else "cmd_empty"] += 1
    return ev
