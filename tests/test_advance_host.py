"""PG_KERNEL_ADVANCE (the opt-in closed-form frame advance of k_relu, k_relu2
and k_sig2: serve delays and periodic rallies) without a GPU:
the ABI value, the kernel names, and pg_eval_population's handling of the
modifier bit for an empty launch (n_genomes = 0: argument checks only, no
device touched)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


def test_bit_value_matches_header_and_names():
    from pong_amd import _lib, device
    text = open(HEADER).read()
    got = int(re.search(r"\bPG_KERNEL_ADVANCE\s*=\s*(0x[0-9a-fA-F]+|\d+)", text).group(1), 0)
    assert got == 0x100 == _lib.PG_KERNEL_ADVANCE
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    for name in ("relu", "relu2", "sig2", "auto"):
        assert device.KERNELS[name + "+advance"] == device.KERNELS[name] | 0x100
    assert sorted(k for k in device.KERNELS if "+" in k) == ["auto+advance", "relu+advance", "relu2+advance",
                                                            "sig2+advance"]


def _args(_lib, shape, kernel, activation, n_genomes=0, **fields):
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes, a.kernel = 6, n_genomes, kernel
    a.net = _lib.make_net(shape, True, _lib.PG_F64, activation=activation)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_empty_launch_accepts_and_refuses(lib):
    from pong_amd import _lib
    ADV, RELU, SIG = _lib.PG_KERNEL_ADVANCE, _lib.PG_ACT_RELU, _lib.PG_ACT_SIGMOID

    def run(shape, kernel, activation, **fields):
        return lib.pg_eval_population(ctypes.byref(_args(_lib, shape, kernel, activation, **fields)), None)

    # the accepted combinations, each in its base kernel's scope; AUTO wherever it resolves
    for shape, kernel, act in (([6, 64, 3], _lib.PG_KERNEL_RELU, RELU), ([6, 16, 16, 3], _lib.PG_KERNEL_RELU2, RELU),
                               ([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, SIG), ([6, 64, 3], _lib.PG_KERNEL_AUTO, RELU),
                               ([6, 16, 16, 3], _lib.PG_KERNEL_AUTO, RELU), ([6, 64, 3], _lib.PG_KERNEL_AUTO, SIG),
                               ([6, 64, 64, 3], _lib.PG_KERNEL_AUTO, SIG), ([6, 16, 16, 3], _lib.PG_KERNEL_AUTO, SIG),
                               ([6, 4, 4, 4, 2], _lib.PG_KERNEL_AUTO, RELU)):
        assert run(shape, kernel, act) == _lib.PG_OK, (shape, kernel, act)
        assert run(shape, kernel | ADV, act) == _lib.PG_OK, (shape, kernel, act)
    # every other explicit kernel with the bit: the retired ones included
    for shape, kernel, act in (([6, 64, 3], _lib.PG_KERNEL_GENERAL, SIG), ([6, 64, 3], _lib.PG_KERNEL_GENERAL, RELU),
                               ([6, 64, 3], _lib.PG_KERNEL_SPLIT, SIG), ([6, 64, 64, 3], _lib.PG_KERNEL_WIDE, SIG),
                               ([6, 64, 64, 3], _lib.PG_KERNEL_RELU_WIDE, RELU),
                               ([6, 64, 3], _lib.PG_KERNEL_RESIDENT, SIG), ([6, 64, 3], _lib.PG_KERNEL_STAGED, SIG)):
        assert run(shape, kernel | ADV, act) == _lib.PG_ERR_UNSUPPORTED, (shape, kernel)
        assert b"advance" in lib.pg_last_error(), lib.pg_last_error()
    # the base kernel's own refusals, word for word, with the bit set
    for shape, kernel, act, fields in (([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, RELU, {}),
                                       ([6, 64, 3], _lib.PG_KERNEL_SIG2, SIG, {}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, SIG, {"horizon": 1000}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, SIG, {"precision": _lib.PG_PREC_F64}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_RELU2, SIG, {}),
                                       ([6, 65, 16, 3], _lib.PG_KERNEL_RELU2, RELU, {})):
        assert run(shape, kernel, act, **fields) == _lib.PG_ERR_UNSUPPORTED
        want = lib.pg_last_error()
        assert run(shape, kernel | ADV, act, **fields) == _lib.PG_ERR_UNSUPPORTED
        assert lib.pg_last_error() == want and b"advance" not in want, want
    assert run([6, 16, 16, 3], _lib.PG_KERNEL_SIG2 | ADV, RELU) == _lib.PG_ERR_UNSUPPORTED
    assert b"sigmoid" in lib.pg_last_error()
    hard = (ctypes.c_uint32 * 32)()  # (never written: the call is refused)
    assert run([6, 16, 16, 3], _lib.PG_KERNEL_SIG2 | ADV, SIG, hard_log=ctypes.addressof(hard),
               hard_cap=4) == _lib.PG_ERR_UNSUPPORTED
    assert b"hard" in lib.pg_last_error()
    # any other bit above the low byte
    for kernel in (0x200, 0x200 | ADV, _lib.PG_KERNEL_RELU | 0x200, _lib.PG_KERNEL_RELU | 0x400 | ADV, 0x10000, -1):
        assert run([6, 64, 3], kernel, RELU) == _lib.PG_ERR_INVALID, hex(kernel)
        assert b"kernel" in lib.pg_last_error()


def test_workspace_is_the_base_kernels(lib):
    from pong_amd import _lib
    ADV = _lib.PG_KERNEL_ADVANCE
    cases = (([6, 64, 3], _lib.PG_KERNEL_RELU, _lib.PG_ACT_RELU), ([6, 16, 16, 3], _lib.PG_KERNEL_RELU2, _lib.PG_ACT_RELU),
             ([6, 64, 64, 3], _lib.PG_KERNEL_SIG2, _lib.PG_ACT_SIGMOID), ([6, 64, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_RELU),
             ([6, 64, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_SIGMOID),      # AUTO -> SPLIT: the lane records
             ([6, 64, 64, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_SIGMOID),  # AUTO -> WIDE: its scratch
             ([6, 16, 16, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_SIGMOID))
    sizes = []
    for shape, kernel, act in cases:
        plain = lib.pg_eval_workspace_bytes(ctypes.byref(_args(_lib, shape, kernel, act, n_genomes=4096)))
        with_bit = lib.pg_eval_workspace_bytes(ctypes.byref(_args(_lib, shape, kernel | ADV, act, n_genomes=4096)))
        assert plain == with_bit > 0, (shape, kernel)
        sizes.append(plain)
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    assert sizes[0] == sizes[1] == sizes[2] == sizes[3] == base and sizes[4] > base and sizes[5] > base
