"""The qubit-flip noise model without a GPU:
montecarlo.noise_masks against the C twin's Philox and the binomial law, the
flip_q16 = 0 identities, the prefix property, what the GPU cases of
tests/test_gpu_montecarlo_noise.py reach (from the reference alone), the static
resources of the noisy kernels and the argument checks of the three calls."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import oracle_lib
from conftest import sub
from kd_util import kernel_descriptors
from oracle_engine import OracleEngine

TAG = 0x4E4F4953
DUMMY = {"nfac": 0, "desc": np.zeros((0, 6), np.int32), "pat": np.zeros(1, np.uint64),
         "apat": np.zeros(1, np.uint64), "thr": np.zeros(1, np.uint64)}
# the shape and seed of the GPU cases (tests/test_gpu_montecarlo_noise.py)
REACH_N, REACH_COUNT, REACH_K, REACH_INST, REACH_BASE = 7, 1000, 0x1000, 67, 0x5EED0


def twin(n, key, count):
    """The closed-form lists of the shipped programs (n <= 11) from the C twin."""
    return oracle_lib.sample(n, key & ((1 << 64) - 1), 0, count, DUMMY, DUMMY, True)


def _r_of(masks):
    """The 4-bit groups of a mask column back into the low bits of r."""
    return sum(int(masks[g]) << (4 * g) for g in range(len(masks)))


@pytest.mark.parametrize("key,e", [(0, 0), (1, 1), (0x5EED, 12345), ((1 << 32) + 7, 99), ((1 << 64) - 3, 5),
                                   (0xDEADBEEFCAFE, (1 << 31) - 1)])
def test_known_answer_at_one_half_is_the_first_philox_block(key, e):
    """k = 0x8000: one step, r = word 0 | word 1 << 32 of block {e, 0, 0, TAG}."""
    mc = sub("montecarlo")
    w = oracle_lib.philox(np.array([[e, 0, 0, TAG]], np.uint32), key)[0]
    r = int(w[0]) | int(w[1]) << 32
    assert tuple(int(x) for x in w) == mc.philox4x32((e, 0, 0, TAG), key)
    got = mc.noise_masks(15, key, e + 1, 0x8000) if e < 1 << 20 else None
    if got is None:  # a far entry: the vectorised helper at that entry alone
        blk = mc._philox4x32_entries(np.array([e], np.uint64), 0, TAG, key)
        assert [int(b[0]) for b in blk] == [int(x) for x in w]
        return
    assert got.shape == (16, e + 1) and got.dtype == np.uint8
    assert _r_of(got[:, e]) == r


def test_two_steps_follow_the_or_and_rule():
    """k = 0xC000 (bits 14 and 15): r = x0 | x1; k = 0x4000: r = x0 alone at
    j0 = 14 then AND with x1 (bit 15 clear)."""
    mc = sub("montecarlo")
    key, e = 77, 3
    w = oracle_lib.philox(np.array([[e, 0, 0, TAG]], np.uint32), key)[0]
    x0, x1 = int(w[0]) | int(w[1]) << 32, int(w[2]) | int(w[3]) << 32
    assert _r_of(mc.noise_masks(15, key, e + 1, 0xC000)[:, e]) == x0 | x1
    assert _r_of(mc.noise_masks(15, key, e + 1, 0x4000)[:, e]) == x0 & x1
    # three steps reach the second block {e, 0, 1, TAG}
    v = oracle_lib.philox(np.array([[e, 0, 1, TAG]], np.uint32), key)[0]
    x2 = int(v[0]) | int(v[1]) << 32
    assert _r_of(mc.noise_masks(15, key, e + 1, 0xA000)[:, e]) == ((x0 & x1) | x2)


@pytest.mark.parametrize("k", [1, 0x0100, 0x1000, 0x5555, 0x8000, 0xFFFF])
def test_flip_rate_is_binomial(k):
    mc = sub("montecarlo")
    n, bits = 11, 12 * 4
    count = -(-(1 << 22) // bits)
    m = mc.noise_masks(n, 0xB10B + k, count, k)
    N, p = bits * count, k / 65536
    assert N >= 1 << 22
    flipped = int(np.unpackbits(m).sum())
    sd = (N * p * (1 - p)) ** 0.5
    print(f"k={k}: {flipped} of {N} bits flipped, expected {N * p:.1f} +- {sd:.1f}")
    assert abs(flipped - N * p) <= 6 * sd


@pytest.mark.parametrize("n", [3, 5])
def test_bits_outside_the_groups_values_are_never_set(n):
    mc = sub("montecarlo")
    w = 1 << n.bit_length()
    m = mc.noise_masks(n, 5, 4096, 0xFFFF)
    assert m.shape == (n + 1, 4096) and int(m.max()) == w - 1  # nearly every bit flips: the full range shows


def test_zero_probability_is_the_identity():
    mc = sub("montecarlo")
    assert not mc.noise_masks(7, 123, 500, 0).any()
    li = twin(7, 9, 64)
    assert np.array_equal(mc.noisy_lists(7, 9, li, 0), li)
    eng = OracleEngine()
    for lists in (None, np.stack([twin(7, 3000 + i, 60) for i in range(4)])):
        want = mc.run_host(7, 60, 2, 4, 3000, eng, lists=lists)
        assert np.array_equal(mc.run_host(7, 60, 2, 4, 3000, eng, lists=lists, flip_q16=0), want)
        wantc = mc.curve_host(7, [5, 60], 2, 4, 3000, eng, lists=lists)
        assert np.array_equal(mc.curve_host(7, [5, 60], 2, 4, 3000, eng, lists=lists, flip_q16=0), wantc)
    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            mc.noise_masks(7, 0, 1, bad)


@pytest.mark.parametrize("k", [1, 0x1000, 0x5555])
def test_masks_of_a_count_are_a_prefix_of_those_of_a_larger_count(k):
    mc = sub("montecarlo")
    big = mc.noise_masks(11, 42, 300, k)
    for c in (0, 1, 63, 64, 65, 299):
        assert np.array_equal(mc.noise_masks(11, 42, c, k), big[:, :c])


def test_curve_host_with_noise_is_the_stack_of_run_host():
    mc = sub("montecarlo")
    lists = np.stack([twin(3, 50 + i, 40) for i in range(3)])
    got = mc.curve_host(3, [1, 7, 40], 1, 3, 50, OracleEngine(), lists=lists, flip_q16=0x2000)
    for j, c in enumerate([1, 7, 40]):
        assert np.array_equal(got[j], mc.run_host(3, c, 1, 3, 50, OracleEngine(), lists=lists[:, :, :c],
                                                  flip_q16=0x2000))


@pytest.fixture(scope="module")
def reach():
    mc = sub("montecarlo")
    clean = [twin(REACH_N, REACH_BASE + i, REACH_COUNT) for i in range(REACH_INST)]
    noisy = [mc.noisy_lists(REACH_N, REACH_BASE + i, li, REACH_K) for i, li in enumerate(clean)]
    return clean, noisy


def test_gpu_cases_reach_new_ground(reach):
    """From the reference alone: what the sampler never produces and the noisy
    kernels therefore run for the first time outside injected fixtures."""
    mc = sub("montecarlo")
    clean, noisy = reach
    g = REACH_N + 1
    turned_q = 0
    for a, b in zip(clean, noisy):
        q = b[0] != b[1]
        distinct = np.array([len(set(col)) == g for col in b.T])
        assert (q & ~distinct).any()  # a Q-correlated entry with a collision (mc_entry's pair walk)
        assert not ((a[0] != a[1]) & np.array([len(set(col)) != g for col in a.T])).any()  # clean ones never collide
        turned_q += int(((a[0] == a[1]) & q).sum())
    assert turned_q > 0  # a not-Q entry turned Q by a flip in group 0 or 1
    differ = 0
    for a, b in zip(clean[:8], noisy[:8]):
        ma, mb = mc.masks_from_lists(REACH_N, a), mc.masks_from_lists(REACH_N, b)
        differ += any(not np.array_equal(ma[k], mb[k]) for k in ("hmask", "czero", "rep"))
    assert differ == 8


def test_noisy_host_rows_differ_from_the_clean_ones(reach):
    mc = sub("montecarlo")
    clean = np.stack(reach[0][:16])
    rows = mc.run_host(REACH_N, REACH_COUNT, 2, 16, REACH_BASE, OracleEngine(), lists=clean)
    noisy = mc.run_host(REACH_N, REACH_COUNT, 2, 16, REACH_BASE, OracleEngine(), lists=clean, flip_q16=REACH_K)
    assert not noisy[:, 3].any()
    assert (rows != noisy).any(axis=1).any()


def test_noisy_kernels_use_no_scratch_no_static_lds_and_at_most_128_vgprs():
    lib = sub("_lib").lib()
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    new = {k: v for k, v in kds.items() if "qba_k_mc_sampled_noisy" in k or "qba_k_mc_curve_sampled_noisy" in k}
    for n in range(1, 16):
        samp = 2 if n <= 11 else 1
        for kernel, shape in ((f"_Z22qba_k_mc_sampled_noisyILi{n}E", lib.qba_montecarlo_shape),
                              (f"_Z28qba_k_mc_curve_sampled_noisyILi{n}E", lib.qba_montecarlo_curve_shape)):
            waves, lds, wgs = C.c_int(), C.c_int64(), C.c_int()
            assert shape(n, C.byref(waves), C.byref(lds), C.byref(wgs)) == 0
            # all samplers of the n, the shipped one at the noiseless kernel's wave count
            assert sum(k.startswith(kernel) for k in new) == (3 if n <= 11 else 2), (n, kernel)
            assert any(k.startswith(f"{kernel}Li{samp}ELi{waves.value}E") for k in new), (n, kernel)
    assert len(new) == 2 * (11 * 3 + 4 * 2)
    for k, v in new.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgprs"] <= 128, (k, v)
    apply = [v for k, v in kds.items() if "qba_k_noise_apply" in k]
    assert len(apply) == 1 and apply[0]["scratch"] == 0 and apply[0]["lds"] == 0


def test_symbols_are_exported_and_flip_is_checked_before_ctx():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    for name in ("qba_montecarlo_sampled_noisy", "qba_montecarlo_curve_sampled_noisy", "qba_noise_apply_batched"):
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES
    eng = sub("engine").Engine
    assert callable(eng.noise_apply)
    counts = (C.c_uint32 * 2)(5, 60)
    calls = {
        "sampled": lambda k: lib.qba_montecarlo_sampled_noisy(None, 7, 2, 0, 4, 60, k, None, None),
        "curve": lambda k: lib.qba_montecarlo_curve_sampled_noisy(None, 7, 2, 0, 4, counts, 2, k, None, None),
        "apply": lambda k: lib.qba_noise_apply_batched(None, 7, 0, 4, 60, k, None, 64, 8 * 64, None),
    }
    for name, f in calls.items():
        for k in (65536, 1 << 20, (1 << 32) - 1):
            assert f(k) == lib_mod.QBA_EINVAL, name
            assert "flip_q16" in lib.qba_last_error().decode(), name
        for k in (0, 1, 65535):  # only the device is missing
            assert f(k) == lib_mod.QBA_EINVAL, name
            assert "ctx is NULL" in lib.qba_last_error().decode(), name
    # the count is still looked at before flip_q16, as before ctx
    assert lib.qba_montecarlo_sampled_noisy(None, 7, 2, 0, 4, 1 << 31, 65536, None, None) == lib_mod.QBA_EINVAL
    assert "count" in lib.qba_last_error().decode()


def test_tables_path_has_no_noisy_sampler():
    mc = sub("montecarlo")
    with pytest.raises(ValueError):
        mc.run(7, 60, 2, 8, 1, None, path="tables", flip_q16=1)
    with pytest.raises(ValueError):
        mc.run(7, 60, 2, 8, 1, None, path="fused", flip_q16=65536)
