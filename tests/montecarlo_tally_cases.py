"""Inputs and a row-by-row restatement of the tally, shared by
tests/test_montecarlo_tally.py (CPU: montecarlo.tally_host against the loop) and
tests/test_gpu_montecarlo_tally.py (GPU: qba_montecarlo_tally against
tally_host).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

WORDS = 32


def out_words(n):
    return 4 + 5 * (n + 1)


def synthetic_rows(n, count, seed, statuses=(1, 2, 4), status_every=7):
    """Random rows in the layout of montecarlo.py: success in {0, 1}, a
    dishonest mask over ranks 1..n, an empty-V_i mask in one row of five, rank
    0 all zero, decisions in [-1, w), accept near 2^31 - 1.  Every
    `status_every`-th row carries one of `statuses` and -- unlike the kernels'
    own status rows -- keeps its other fields, so a tally that does not skip
    it is wrong in nearly every word."""
    rng = np.random.default_rng(seed)
    w = 1 << int(n).bit_length()
    rows = np.zeros((count, out_words(n)), np.int32)
    rows[:, 0] = rng.integers(0, 2, count)
    rows[:, 1] = rng.integers(0, 1 << n, count) << 1
    rows[:, 2] = np.where(rng.integers(0, 5, count) == 0, rng.integers(1, 1 << n, count) << 1, 0)
    per = rows[:, 4 + 5:].reshape(count, n, 5)
    assert np.shares_memory(per, rows)
    per[:, :, 0] = rng.integers(-1, w, (count, n))
    per[:, :, 1] = rng.integers(0, 1 << w, (count, n))
    per[:, :, 2] = (1 << 31) - 1 - rng.integers(0, 1000, (count, n))
    per[:, :, 3] = rng.integers(0, 1 << 20, (count, n))
    per[:, :, 4] = rng.integers(0, 64, (count, n))
    if statuses and count:
        at = np.arange(status_every // 2, count, status_every)
        rows[at, 3] = np.asarray(statuses, np.int32)[np.arange(len(at)) % len(statuses)]
    return rows


def tally_loop(n, rows, inst_base=0, select=0):
    """The tally words of one slice and its matching indices, one row and one
    rank at a time in plain Python integers."""
    t = [0] * WORDS
    matches = []
    for i, row in enumerate(np.asarray(rows).tolist()):
        ok, dis, empty, st = row[:4]
        t[0] += 1
        if st:
            t[3] += 1
            t[4] |= st & 0xFFFFFFFF
            if select & 4:
                matches.append(inst_base + i)
            continue
        t[1] += ok != 0
        t[2] += empty != 0
        if dis & 2:
            t[5] += 1
            t[6] += ok != 0
        for r in range(1, n + 1):
            d, _v, acc, rej, sent = row[4 + 5 * r:9 + 5 * r]
            t[7] += acc
            t[8] += rej
            t[9] += sent
            if not (dis >> r) & 1:
                if d == -1:
                    t[15] += 1
                elif 0 <= d < 16:
                    t[16 + d] += 1
        if (select & 1 and ok == 0) or (select & 2 and empty != 0):
            matches.append(inst_base + i)
    t[10] = len(matches)
    return t, matches
