"""Parameter sets shared by tests/test_montecarlo.py (CPU: what the host
reference reaches on them) and tests/test_gpu_montecarlo.py (GPU: kernel ==
host reference on them).  TEST INFRASTRUCTURE ONLY.

SEED_BASE values were picked on the CPU so that, taken together, the sets
reach every path listed in test_montecarlo.test_parameter_sets_reach_every_path.
The C twin samples n <= 11 only, so the n = 15 host reference takes injected
lists: on the GPU the device-sampled lists themselves, on the CPU lists of the
same law drawn with numpy (tfg_oracle.closed_form_lists).
"""
import json
from pathlib import Path

import numpy as np

import tfg_oracle as orc

# (n, n_dishonest, sizeL) -> (seed_base, instances)
CASES = {
    (3, 1, 60): (1000, 32),
    (4, 1, 60): (1000, 32),
    (7, 2, 200): (3000, 32),
    (11, 3, 400): (4000, 32),
    (15, 2, 400): (5000, 32),
}
IDS = [f"n{n}-d{d}-L{s}" for n, d, s in CASES]

# the injected-list sets: every case of tests/golden/protocol.json (lists with
# Cond3 collisions; the source of rejected commander packets and empty V_i),
# its lists replicated for INJECT_KEYS protocol keys from INJECT_BASE
INJECT_BASE, INJECT_KEYS = 7000, 16


# the hostile sets and the sweep over every n (tests/golden/hostile_lists.npz,
# written by tests/golden/gen_hostile_lists.py, which describes the mutation
# families): lists with duplicated rows, many traitors.  They reach what honest
# lists cannot: descriptor canonicalisation (rep != g), L of 6 and more
# descriptors, rounds 5 and above, several packets per mailbox.
_HOSTILE = np.load(Path(__file__).resolve().parent / "golden" / "hostile_lists.npz")
_META = json.loads(str(_HOSTILE["meta"]))
HOSTILE = _META["hostile"]   # dicts: name, n, nDishonest, sizeL, family, base, keys, rows[, u | src]
SWEEP = _META["sweep"]       # dicts: name, n, nDishonest, sizeL, base, keys
HOSTILE_IDS = [c["name"] for c in HOSTILE]
SWEEP_IDS = [c["name"] for c in SWEEP]
DUP_FAMILIES = ("dup_all", "dup_u", "dup3", "dup_cmd")


def hostile_lists(case):
    """[keys, n+1, sizeL] uint8 of a HOSTILE or SWEEP entry (read-only): a
    hostile set's one list under each of its keys, a sweep entry's own lists."""
    li = _HOSTILE[case["name"]]
    if li.ndim == 2:
        li = np.broadcast_to(li, (case["keys"],) + li.shape)
    assert li.shape == (case["keys"], case["n"] + 1, case["sizeL"]) and li.dtype == np.uint8
    li = li.view()
    li.setflags(write=False)
    return li


def tables_rows(engine, n, nd, base, inst, sizeL, keep_lists=False):
    """The tables path's rows on the GPU: protocol_batched on the tables of
    sample_check_batched.  For sizeL = 0 the batched sampler writes nothing,
    and the rows are defined on all-zero tables."""
    lists, counts = engine.sample_check_batched(n, base, inst, sizeL)
    if sizeL == 0:
        for t in (counts.H, counts.C, counts.P):
            t.zero_()
    rows = engine.protocol_batched(n, nd, base, counts).cpu().numpy()
    rows.setflags(write=False)
    return (rows, lists) if keep_lists else rows


def cpu_lists(n, sizeL, seed_base, n_inst):
    """Injected lists for a host-only evaluation of a set the C twin cannot
    sample (n > 11); None otherwise."""
    if n <= 11:
        return None
    rng = np.random.default_rng(seed_base)
    return np.stack([orc.closed_form_lists(n, sizeL, rng) for _ in range(n_inst)])
