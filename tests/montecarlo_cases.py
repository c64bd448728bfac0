"""Parameter sets shared by tests/test_montecarlo.py (CPU: what the host
reference reaches on them) and tests/test_gpu_montecarlo.py (GPU: kernel ==
host reference on them).  TEST INFRASTRUCTURE ONLY.

SEED_BASE values were picked on the CPU so that, taken together, the sets
reach every path listed in test_montecarlo.test_parameter_sets_reach_every_path.
The C twin samples n <= 11 only, so the n = 15 host reference takes injected
lists: on the GPU the device-sampled lists themselves, on the CPU lists of the
same law drawn with numpy (tfg_oracle.closed_form_lists).
"""
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


def cpu_lists(n, sizeL, seed_base, n_inst):
    """Injected lists for a host-only evaluation of a set the C twin cannot
    sample (n > 11); None otherwise."""
    if n <= 11:
        return None
    rng = np.random.default_rng(seed_base)
    return np.stack([orc.closed_form_lists(n, sizeL, rng) for _ in range(n_inst)])
