"""The noisy batched sampler without a GPU: the two
exports and their flip_q16 envelope, the new path of montecarlo.run, the
argument errors of tfg --tables and the static resources of
qba_k_batched_noisy read from the cross-compiled library."""
import re
from pathlib import Path

import pytest

from conftest import sub
from kd_util import kernel_descriptors

NAMES = ("qba_sample_check_batched_noisy", "qba_sample_check_batched_packed_noisy")


def test_the_two_calls_are_exported():
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in lib_mod.SIGNATURES


@pytest.mark.parametrize("name", NAMES)
def test_flip_is_checked_before_ctx(name):
    lib_mod = sub("_lib")
    lib = lib_mod.lib()
    f = lambda k: getattr(lib, name)(None, 7, 0, 4, 60, k, None, 64, 8 * 64, None, None, None, None)  # noqa: E731
    for k in (65536, (1 << 32) - 1):
        assert f(k) == lib_mod.QBA_EINVAL
        assert "flip_q16" in lib.qba_last_error().decode() and name in lib.qba_last_error().decode()
    for k in (0, 1, 65535):  # only the device is missing
        assert f(k) == lib_mod.QBA_EINVAL
        assert "ctx is NULL" in lib.qba_last_error().decode()


def test_run_knows_the_path_and_checks_flip():
    mc = sub("montecarlo")
    with pytest.raises(ValueError, match="flip_q16"):
        mc.run(7, 60, 2, 8, 1, None, path="tables_noisy", flip_q16=65536)
    with pytest.raises(ValueError, match="tables_noisy"):  # the refusal of the plain tables path names the new one
        mc.run(7, 60, 2, 8, 1, None, path="tables", flip_q16=1)
    with pytest.raises(ValueError, match="tables_noisy"):
        mc.run(7, 60, 2, 8, 1, None, path="no such path")


@pytest.mark.parametrize("argv,msg", [
    (["200", "2", "--runs", "8", "--tables", "--curve", "100"], "--tables: not with --curve or --fused"),
    (["200", "2", "--runs", "8", "--tables", "--fused"], "--tables: not with --curve or --fused"),
    (["200", "2", "--runs", "8", "--tables", "--fused", "--flip", "4096"], "--tables: not with --curve or --fused"),
    (["200", "2", "--tables"], "--tables needs --runs"),
])
def test_tfg_tables_argument_errors(argv, msg, capsys):
    tfg = sub("tfg")
    with pytest.raises(SystemExit) as e:
        tfg._args(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_tfg_tables_keeps_flip_from_implying_fused():
    tfg = sub("tfg")
    a = tfg._args(["200", "2", "--runs", "8", "--tables", "--flip", "4096"])
    assert a.tables and not a.fused and a.flip == 4096
    b = tfg._args(["200", "2", "--runs", "8", "--flip", "4096"])  # as before
    assert b.fused and not b.tables


def test_noisy_batched_kernels_use_no_scratch_and_no_static_lds():
    kds = kernel_descriptors(Path(sub("_lib").LIB_PATH))
    new = {k: v for k, v in kds.items() if "qba_k_batched_noisy" in k}
    # <NP, SAMP, QPT, PK>: every sampler of the n (closed form up to n = 11); byte rows with one-quad and wide
    # steps, nibble rows with the wide step alone (the calls refuse rows the one-quad step would be for)
    assert len(new) == 3 * (11 * 3 + 4 * 2)
    assert not any(re.match(r"_Z19qba_k_batched_noisyILi\d+ELi\dELi1ELi1EE", k) for k in new)
    for n in (3, 7, 11, 15):
        for pk in (0, 1):
            mine = {k: v for k, v in new.items() if re.match(rf"_Z19qba_k_batched_noisyILi{n}ELi\dELi\dELi{pk}EE", k)}
            assert len(mine) == (1 if pk else 2) * (3 if n <= 11 else 2), (n, pk)
            for k, v in mine.items():
                assert v["scratch"] == 0 and v["lds"] == 0, (k, v)
    for k, v in new.items():  # and every other n
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)
