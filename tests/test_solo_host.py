"""PG_KERNEL_SOLO (scripted-opponent games of k_relu, k_relu2 and k_sig2 on half
a lane group) without a GPU: the ABI value, the kernel names
(device.kernel_code), and pg_eval_population's handling of the modifier bit for
an empty launch (n_genomes = 0: argument checks only, no device touched)."""
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


def test_bit_value_matches_header():
    from pong_amd import _lib
    text = open(HEADER).read()
    got = int(re.search(r"\bPG_KERNEL_SOLO\s*=\s*(0x[0-9a-fA-F]+|\d+)", text).group(1), 0)
    assert got == 0x800 == _lib.PG_KERNEL_SOLO
    assert _lib.PG_KERNEL_SOLO & (0xff | _lib.PG_KERNEL_ADVANCE) == 0
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13


def test_kernel_code_names():
    from pong_amd import _lib, device
    ADV, SOLO = _lib.PG_KERNEL_ADVANCE, _lib.PG_KERNEL_SOLO
    plain = {"auto": 0, "general": 1, "split": 3, "wide": 4, "relu": 6, "relu2": 7, "relu_wide": 8, "sig2": 9}
    for name, code in plain.items():
        assert device.kernel_code(name) == code == device.KERNELS[name]
    for name in ("relu", "relu2", "sig2", "auto"):
        assert device.kernel_code(name + "+advance") == plain[name] | ADV == device.KERNELS[name + "+advance"]
        assert device.kernel_code(name + "+solo") == plain[name] | SOLO
        assert device.kernel_code(name + "+advance+solo") == plain[name] | ADV | SOLO
        assert device.kernel_code(name + "+solo+advance") == plain[name] | ADV | SOLO
    for bad in ("general+solo", "split+solo", "wide+solo", "relu_wide+solo", "general+advance", "relu+solo+solo",
                "relu+advance+advance", "relu+advance+solo+solo", "relu+fast", "relu+", "+solo", "solo", "", "resident"):
        with pytest.raises(KeyError) as err:
            device.kernel_code(bad)
        assert "+solo" in str(err.value) and "+advance" in str(err.value), bad
    # KERNELS itself is what it was: the plain names and the four advance ones
    assert sorted(device.KERNELS) == sorted(list(plain) + [n + "+advance" for n in ("relu", "relu2", "sig2", "auto")])


def _args(_lib, shape, kernel, activation, n_genomes=0, **fields):
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes, a.kernel = 6, n_genomes, kernel
    a.net = _lib.make_net(shape, True, _lib.PG_F64, activation=activation)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_empty_launch_accepts_and_refuses(lib):
    from pong_amd import _lib
    ADV, SOLO, RELU, SIG = _lib.PG_KERNEL_ADVANCE, _lib.PG_KERNEL_SOLO, _lib.PG_ACT_RELU, _lib.PG_ACT_SIGMOID

    def run(shape, kernel, activation, **fields):
        return lib.pg_eval_population(ctypes.byref(_args(_lib, shape, kernel, activation, **fields)), None)

    # the accepted combinations, each in its base kernel's scope; AUTO wherever it resolves
    for shape, kernel, act in (([6, 64, 3], _lib.PG_KERNEL_RELU, RELU), ([6, 16, 16, 3], _lib.PG_KERNEL_RELU2, RELU),
                               ([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, SIG), ([6, 64, 3], _lib.PG_KERNEL_AUTO, RELU),
                               ([6, 16, 16, 3], _lib.PG_KERNEL_AUTO, RELU), ([6, 64, 3], _lib.PG_KERNEL_AUTO, SIG),
                               ([6, 64, 64, 3], _lib.PG_KERNEL_AUTO, SIG), ([6, 16, 16, 3], _lib.PG_KERNEL_AUTO, SIG),
                               ([6, 4, 4, 4, 2], _lib.PG_KERNEL_AUTO, RELU)):
        assert run(shape, kernel | SOLO, act) == _lib.PG_OK, (shape, kernel, act, lib.pg_last_error())
        assert run(shape, kernel | SOLO | ADV, act) == _lib.PG_OK, (shape, kernel, act, lib.pg_last_error())
    # every other explicit kernel with the bit: the retired ones included
    for shape, kernel, act in (([6, 64, 3], _lib.PG_KERNEL_GENERAL, SIG), ([6, 64, 3], _lib.PG_KERNEL_GENERAL, RELU),
                               ([6, 64, 3], _lib.PG_KERNEL_SPLIT, SIG), ([6, 64, 64, 3], _lib.PG_KERNEL_WIDE, SIG),
                               ([6, 64, 64, 3], _lib.PG_KERNEL_RELU_WIDE, RELU),
                               ([6, 64, 3], _lib.PG_KERNEL_RESIDENT, SIG), ([6, 64, 3], _lib.PG_KERNEL_STAGED, SIG)):
        assert run(shape, kernel | SOLO, act) == _lib.PG_ERR_UNSUPPORTED, (shape, kernel)
        assert b"solo" in lib.pg_last_error() and b"advance" not in lib.pg_last_error(), lib.pg_last_error()
        # with both bits the advance bit's refusal comes first
        assert run(shape, kernel | SOLO | ADV, act) == _lib.PG_ERR_UNSUPPORTED, (shape, kernel)
        assert b"advance" in lib.pg_last_error() and b"solo" not in lib.pg_last_error(), lib.pg_last_error()
    # the base kernel's own refusals, word for word, with the bit set
    hard = (ctypes.c_uint32 * 32)()  # (never written: the calls are refused)
    for shape, kernel, act, fields in (([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, RELU, {}),
                                       ([6, 64, 3], _lib.PG_KERNEL_SIG2, SIG, {}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, SIG, {"horizon": 1000}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, SIG, {"precision": _lib.PG_PREC_F64}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_SIG2, SIG,
                                        {"hard_log": ctypes.addressof(hard), "hard_cap": 4}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_RELU2, SIG, {}),
                                       ([6, 65, 16, 3], _lib.PG_KERNEL_RELU2, RELU, {}),
                                       ([6, 16, 16, 3], _lib.PG_KERNEL_RELU2, RELU, {"precision": _lib.PG_PREC_F64})):
        assert run(shape, kernel, act, **fields) == _lib.PG_ERR_UNSUPPORTED
        want = lib.pg_last_error()
        for bits in (SOLO, SOLO | ADV):
            assert run(shape, kernel | bits, act, **fields) == _lib.PG_ERR_UNSUPPORTED
            assert lib.pg_last_error() == want and b"solo" not in want, want
    # any other bit above the low byte
    for kernel in (0x200, 0x400, 0x1000, _lib.PG_KERNEL_RELU | 0x200 | SOLO, 0x200 | SOLO | ADV, 0x10000 | SOLO, -1):
        assert run([6, 64, 3], kernel, RELU) == _lib.PG_ERR_INVALID, hex(kernel)
        assert b"kernel" in lib.pg_last_error()


def test_workspace_is_the_base_kernels(lib):
    from pong_amd import _lib
    ADV, SOLO = _lib.PG_KERNEL_ADVANCE, _lib.PG_KERNEL_SOLO
    cases = (([6, 64, 3], _lib.PG_KERNEL_RELU, _lib.PG_ACT_RELU), ([6, 16, 16, 3], _lib.PG_KERNEL_RELU2, _lib.PG_ACT_RELU),
             ([6, 64, 64, 3], _lib.PG_KERNEL_SIG2, _lib.PG_ACT_SIGMOID), ([6, 64, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_RELU),
             ([6, 64, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_SIGMOID),      # AUTO -> SPLIT: the lane records
             ([6, 64, 64, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_SIGMOID),  # AUTO -> WIDE: its scratch
             ([6, 16, 16, 3], _lib.PG_KERNEL_AUTO, _lib.PG_ACT_SIGMOID))
    sizes = []
    for shape, kernel, act in cases:
        plain = lib.pg_eval_workspace_bytes(ctypes.byref(_args(_lib, shape, kernel, act, n_genomes=4096)))
        for bits in (SOLO, SOLO | ADV):
            with_bit = lib.pg_eval_workspace_bytes(ctypes.byref(_args(_lib, shape, kernel | bits, act, n_genomes=4096)))
            assert plain == with_bit > 0, (shape, kernel, bits)
        sizes.append(plain)
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256  # (both game counters live in the 256-byte header)
    assert sizes[0] == sizes[1] == sizes[2] == sizes[3] == base and sizes[4] > base and sizes[5] > base
