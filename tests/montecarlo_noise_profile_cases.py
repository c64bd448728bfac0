"""Profiles, the grid, a scalar restatement of the definition and the observing
party shared by tests/test_montecarlo_noise_profile.py (CPU: the definition and
what the host model reaches) and tests/test_gpu_montecarlo_noise_profile.py
(GPU: the noise-profile kernels == the host model).  TEST INFRASTRUCTURE ONLY
(DESIGN.md section 13.14)."""
import threading

import numpy as np

from test_montecarlo_adversary import PRESETS


def _nds(n):
    return sorted({min(max(d, 0), n) for d in (0, 1, n // 3, n - 1)})


NS = [1, 2, 3, 4, 7, 11, 15]
COUNTS = [0, 3, 65, 130]  # 65 and 130 straddle a 64-entry step
INST, GRID_BASE = 67, 0x4E5052
DEPOLS = [0, 1, 0x4000, 0xFFFF]
KINDS = ["zero", "uniform", "commander", "last", "mixed"]
POLICIES = [0xF, PRESETS["reorder_low"], 0x1F]
GRID = [(n, nd) for n in NS for nd in _nds(n)]  # traitors {0, 1, n // 3, n - 1}
MASK64 = (1 << 64) - 1


def rates_of(kind: str, n: int) -> list:
    """The rates of a named profile: all-zero; uniform 0x1000; the commander's
    row alone at 0x8000; the last lieutenant's alone at 1; rates whose lowest
    set bits differ (15, 0, 12, 1, 3, ... from row 0 on) with a zero row."""
    if kind == "zero":
        return [0] * (n + 1)
    if kind == "uniform":
        return [0x1000] * (n + 1)
    if kind == "commander":
        return [0x8000] + [0] * n
    if kind == "last":
        return [0] * n + [1]
    mixed = [0x8000, 0, 0x1000, 0x0002, 0x5558, 0x0001, 0xFFFF, 0x00F0]
    return [mixed[g % len(mixed)] for g in range(n + 1)]


PROFILES = [(kind, depol) for depol in DEPOLS for kind in KINDS]  # 20; index = 5 * (depol index) + kind index


def profiles_at(gi: int) -> list:
    """The five profile indices grid point gi runs: the traitor counts of one n
    (four of them from n = 7 on) take the four blocks of five in turn, shifted
    by n's place so that kinds and depol values also mix below n = 7."""
    n, nd = GRID[gi]
    block = (_nds(n).index(nd) + NS.index(n)) % 4
    return [5 * block + j for j in range(5)]


def policy_at(gi: int, pi: int) -> int:
    return POLICIES[(gi + pi) % 3]


CASES = [(gi, pi) for gi in range(len(GRID)) for pi in profiles_at(gi)]
CASE_IDS = [f"n{GRID[gi][0]}-d{GRID[gi][1]}-{PROFILES[pi][0]}-depol{PROFILES[pi][1]:#x}" for gi, pi in CASES]


def scalar_r(mc, n: int, key: int, e: int, rates, depol: int) -> int:
    """The 64-bit mask r of one entry, word by word from philox4x32: the
    definition of DESIGN.md section 13.14 restated without numpy."""
    key &= MASK64
    ctr = lambda c2: mc.philox4x32((e & 0xFFFFFFFF, e >> 32, c2, 0x4E4F4953), key)  # noqa: E731
    word = lambda t: ctr(t // 4)[t % 4]  # noqa: E731
    r = 0
    nz = [k for k in rates if k]
    if nz:
        j0 = min((k & -k).bit_length() - 1 for k in nz)
        for s in range(16 - j0):
            x = word(2 * s) | word(2 * s + 1) << 32
            m = 0
            for g, k in enumerate(rates):
                if (k >> (j0 + s)) & 1:
                    m |= 0xF << (4 * g)
            r = ((r | x) & m) | ((r & x) & ~m & MASK64)
    if depol:
        d = ctr(8)
        if (d[0] & 0xFFFF) < depol:
            r ^= d[2] | d[3] << 32
    return r


def scalar_masks(mc, n: int, key: int, count: int, rates, depol: int) -> np.ndarray:
    w = 1 << int(n).bit_length()
    out = np.zeros((n + 1, count), np.uint8)
    for e in range(count):
        r = scalar_r(mc, n, key, e, rates, depol)
        for g in range(n + 1):
            out[g, e] = (r >> (4 * g)) & (w - 1)
    return out


def depol_hits(mc, key: int, count: int, depol: int) -> np.ndarray:
    """Whether entry e is depolarised, from the scalar Philox."""
    key &= MASK64
    return np.array([(mc.philox4x32((e, 0, 8, 0x4E4F4953), key)[0] & 0xFFFF) < depol for e in range(count)], bool)


# ---------------------------------------------------------------------------
# reach sets (host model alone)
# ---------------------------------------------------------------------------
REACH_BASE, REACH_KEYS = 0x4E50, 48
MEAN = 0x0800  # the mean rate m of the "where the noise sits" sets
# name -> (n, n_dishonest, sizeL, policy, (rates, depol_q16) or "traitors", the events it was chosen for)
REACH = {
    "n3-d1-L24-uniform": (3, 1, 24, 0xF, ([MEAN] * 4, 0), ("uniform_ok_cmd_fails", "cmd_ok_uniform_fails")),
    "n7-d2-L24-uniform": (7, 2, 24, 0xF, ([MEAN] * 8, 0), ("uniform_ok_cmd_fails", "cmd_ok_uniform_fails")),
    "n7-d2-L40-depol": (7, 2, 40, 0xF, ([0] * 8, 0x2000), ("depol_q_repeat", "notq_read_as_q")),
    "n3-d1-L40-depol": (3, 1, 40, 0xF, ([0] * 4, 0x4000), ("depol_q_repeat", "notq_read_as_q")),
    "n7-d2-L4-traitors": (7, 2, 4, 0xF, "traitors", ("traitor_rows_unseen",)),
    "n7-d2-L24-traitors": (7, 2, 24, 0xF, "traitors", ("traitor_rows_seen",)),
}
EVENTS = ("uniform_ok_cmd_fails", "cmd_ok_uniform_fails", "depol_q_repeat", "notq_read_as_q", "traitor_rows_unseen",
          "traitor_rows_seen")


def commander_only(n: int, mean: int) -> list:
    """The same total noise (n + 1) * mean on the commander's row alone."""
    return [min((n + 1) * mean, 0xFFFF)] + [0] * n


_LOCK = threading.Lock()  # the ranks of a run are threads


def observing(mc, seen):
    """A CountParty subclass for run_host's party_cls seam that records into
    ``seen``, per instance key:

    ``lists``      the lists rank 0 counted (after the noise)
    ``tables``     rank 0's CountTables
    ``consulted``  every tuple an honest or dishonest lieutenant's check looked at, by rank
    """
    seen.update({"lists": {}, "tables": {}, "consulted": {}})
    base = mc.CountParty

    class Observed(base):
        def particle_comm(self):
            super().particle_comm()
            if self.rank == 0:
                with _LOCK:
                    seen["lists"][int(self.seed)] = None if self.inject is None else np.array(self.inject)
                    seen["tables"][int(self.seed)] = self.tables

        def check(self, v, L):
            with _LOCK:
                seen["consulted"].setdefault((int(self.seed), self.rank), set()).update(L)
            return super().check(v, L)

    return Observed


def q_events(n: int, clean: np.ndarray, noisy: np.ndarray, hit: np.ndarray) -> dict:
    """From one instance's clean and noisy lists [n+1, sizeL] and its
    depolarised entries: entries that are Q-correlated after the noise (row 0 !=
    row 1), were depolarised and hold a value twice among rows 1..n (the pair
    walk of mc_entry finds an equal pair); and depolarised entries that were not
    Q-correlated before the noise and are read as Q after it."""
    q_after, q_before = noisy[0] != noisy[1], clean[0] != clean[1]
    rep = np.array([len(set(noisy[1:, e].tolist())) < n for e in range(noisy.shape[1])], bool)
    return {"depol_q_repeat": int((hit & q_after & rep).sum()), "notq_read_as_q": int((hit & ~q_before & q_after).sum())}
