#!/usr/bin/env python3
"""Fixture for the hostile list sets of tests/montecarlo_cases.py: injected
lists in which rows are duplicated, so that the count-mode descriptor
canonicalisation (rep(u, g) = min h with C[u][g][h] == P[u]), long L sets, deep
rounds and full mailboxes are reached, plus a plain sweep over every n.

With Q = {k : L0[k] != L1[k]}, P_u = {k in Q : L1[k] = u} and g < h drawn
lieutenants, a base list of tfg_oracle.closed_form_lists is mutated by one of

    dup_all   row h := row g everywhere
    dup_u     row h := row g on P_u, one u with P_u non-empty
    near      as dup_u on all of P_u but one entry (|P_u| >= 2): no
              canonicalisation, C[u][g][h] = P[u] - 1 is a Cond3 collision
    dup3      rows g < h < k identical: rep is the minimum, not the previous row
    dup_cmd   a lieutenant's row := row 0 or row 1 on Q: rep in {0, 1}

dup_u and near take for u the order of the commander under the set's first
protocol key (ProtocolRng(base, 1).randint(w); the base is advanced until that
key's commander is honest), so the mutated P_u is the P of at least one run;
the list seed is advanced until that P_u is large enough.

The file holds the lists themselves (uint8), because numpy's Generator streams
may change between releases, and a JSON description of every set:

    hostile  one list [n+1, sizeL] per set, run under `keys` protocol keys from `base`
    sweep    `keys` lists [keys, n+1, sizeL] per entry, unmutated

    python tests/golden/gen_hostile_lists.py
"""
import importlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parents[1] / "oracle"))
import tfg_oracle as orc  # noqa: E402

mc = importlib.import_module("tfg---quantum-byzantine-agreement_amd.montecarlo")

OUT = HERE / "hostile_lists.npz"
KEYS = 8
PARAMS = [(2, 1, 24), (3, 2, 30), (4, 2, 40), (7, 4, 60), (8, 7, 64), (12, 6, 80), (15, 8, 96), (15, 14, 96)]
FAMILIES = {"dup_all": 3, "dup_u": 3, "near": 3, "dup3": 4, "dup_cmd": 2}  # family -> smallest n
HOSTILE_BASE, SWEEP_BASE = 20000, 60000   # protocol keys; 100 apart per set
LIST_SEED = 0x7F6                         # list streams; 1000 apart per set


def mutate(li, n, family, rng, u):
    """The mutated copy of `li` and what was done to it, or None when this
    list cannot carry the family (P_u too small)."""
    li = li.copy()
    q = li[0] != li[1]
    pu = np.nonzero(q & (li[1] == u))[0]
    rows = sorted(rng.choice(np.arange(2, n + 1), 3 if family == "dup3" else 2 if family != "dup_cmd" else 1,
                             replace=False).tolist())
    what = {"rows": rows}
    if family == "dup_all":
        li[rows[1]] = li[rows[0]]
    elif family == "dup3":
        li[rows[1]] = li[rows[0]]
        li[rows[2]] = li[rows[0]]
    elif family == "dup_u":
        if len(pu) < 1:
            return None
        li[rows[1], pu] = li[rows[0], pu]
        what["u"] = int(u)
    elif family == "near":
        if len(pu) < 2:
            return None
        keep = int(rng.integers(len(pu)))
        on = np.delete(pu, keep)
        li[rows[1], on] = li[rows[0], on]
        what["u"] = int(u)
    elif family == "dup_cmd":
        src = int(rng.integers(2))
        li[rows[0], q] = li[src, q]
        what["src"] = src
    return li, what


def main():
    arrays, hostile, sweep = {}, [], []
    idx = 0
    for n, nd, sizeL in PARAMS:
        for family, least in FAMILIES.items():
            if n < least:
                continue
            base = HOSTILE_BASE + 100 * idx
            while 1 in mc.ProtocolRng(base, 0).choice(np.arange(1, n + 1), nd, replace=False):
                base += 1  # an honest commander under the first key: its P is P_u
            u = mc.ProtocolRng(base, 1).randint(orc.width(n))
            seed = LIST_SEED + 1000 * idx
            while True:
                rng = np.random.default_rng(seed)
                got = mutate(orc.closed_form_lists(n, sizeL, rng), n, family, rng, u)
                if got is not None:
                    break
                seed += 1
            name = f"n{n}-d{nd}-L{sizeL}-{family}"
            arrays[name] = got[0]
            hostile.append({"name": name, "n": n, "nDishonest": nd, "sizeL": sizeL, "family": family,
                            "base": base, "keys": KEYS, "list_seed": seed, **got[1]})
            idx += 1
    for j, (n, nd) in enumerate((n, min(n, 2)) for n in range(1, 16)):  # n = 1: a dishonest commander alone
        sizeL = 8 * (n + 1)
        rng = np.random.default_rng(LIST_SEED + 500 + 1000 * j)
        name = f"sweep-n{n}-d{nd}-L{sizeL}"
        arrays[name] = np.stack([orc.closed_form_lists(n, sizeL, rng) for _ in range(KEYS)])
        sweep.append({"name": name, "n": n, "nDishonest": nd, "sizeL": sizeL, "base": SWEEP_BASE + 100 * j,
                      "keys": KEYS})
    np.savez_compressed(OUT, meta=np.array(json.dumps({"hostile": hostile, "sweep": sweep})), **arrays)
    print(f"wrote {OUT}: {len(hostile)} hostile sets, {len(sweep)} sweep entries, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
