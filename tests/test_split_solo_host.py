"""pg_eval_resolve without a GPU: the kernel pg_eval_population launches for a
set of arguments and the modifier bits in effect on it (PG_KERNEL_SOLO on
k_service's [6, 33..64, O] layout under PG_KERNEL_AUTO), its
refusals, the workspace with and without the bit, Evaluator.resolved_kernel."""
import ctypes
import itertools

import pytest

SHAPES = ([6, 32, 3], [6, 33, 2], [6, 64, 4], [6, 65, 3], [6, 16, 16, 3], [6, 4, 4, 4, 2])


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


def _args(_lib, shape, kernel, activation, n_genomes=0, dtype=None, **fields):
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes, a.kernel = 6, n_genomes, kernel
    a.net = _lib.make_net(shape, True, _lib.PG_F64 if dtype is None else dtype, activation=activation)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _expected(_lib, shape, activation, kernel, bits, traced, horizon, hard_log, lanes):
    """The rules of pong_ga.h, written out: AUTO's choice, then where each bit takes effect."""
    K = _lib
    hidden = shape[1:-1]
    if kernel != K.PG_KERNEL_AUTO:
        base = kernel
    elif activation == K.PG_ACT_RELU:
        base = K.PG_KERNEL_RELU if len(hidden) == 1 else (K.PG_KERNEL_RELU2 if len(hidden) == 2 else K.PG_KERNEL_GENERAL)
    else:
        base = K.PG_KERNEL_SPLIT if len(hidden) == 1 else K.PG_KERNEL_GENERAL  # (no shape here is WIDE's: H1, H2 < 64)
    cert = base in (K.PG_KERNEL_RELU, K.PG_KERNEL_RELU2, K.PG_KERNEL_SIG2)
    out = base
    if bits & K.PG_KERNEL_ADVANCE and cert and not traced:
        out |= K.PG_KERNEL_ADVANCE
    if bits & K.PG_KERNEL_SOLO:
        split_solo = (base == K.PG_KERNEL_SPLIT and 33 <= shape[1] <= 64 and lanes in (0, 8) and not traced
                      and not horizon and not hard_log)
        if cert or split_solo:
            out |= K.PG_KERNEL_SOLO
    return out


def test_symbol_and_examples(lib):
    """The header's examples."""
    from pong_amd import _lib as K
    ADV, SOLO = K.PG_KERNEL_ADVANCE, K.PG_KERNEL_SOLO
    buf = (ctypes.c_uint8 * 8)()  # (never followed: the query reads whether trace is set)
    tr = {"trace": ctypes.addressof(buf), "trace_games": 1, "trace_cap": 1}

    def ask(shape, kernel, act, **f):
        return lib.pg_eval_resolve(ctypes.byref(_args(K, shape, kernel, act, **f)))

    assert ask([6, 64, 3], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID) == K.PG_KERNEL_SPLIT | SOLO
    assert ask([6, 64, 3], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID, **tr) == K.PG_KERNEL_SPLIT
    assert ask([6, 64, 3], K.PG_KERNEL_AUTO | ADV | SOLO, K.PG_ACT_RELU) == K.PG_KERNEL_RELU | ADV | SOLO
    assert ask([6, 64, 3], K.PG_KERNEL_AUTO | ADV | SOLO, K.PG_ACT_RELU, **tr) == K.PG_KERNEL_RELU | SOLO
    assert ask([6, 16, 16, 3], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID) == K.PG_KERNEL_GENERAL
    assert ask([6, 64, 3], K.PG_KERNEL_AUTO | ADV, K.PG_ACT_SIGMOID) == K.PG_KERNEL_SPLIT  # SPLIT always advances
    assert ask([6, 64, 64, 3], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID) == K.PG_KERNEL_WIDE
    assert ask([6, 64, 3], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID, precision=K.PG_PREC_F64) == K.PG_KERNEL_GENERAL
    # every routed (O, genome type), and a played launch resolves as an empty one
    for O, dtype, n in itertools.product((2, 3, 4), (K.PG_F32, K.PG_F64), (0, 4096)):
        assert ask([6, 48, O], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID, dtype=dtype, n_genomes=n) == K.PG_KERNEL_SPLIT | SOLO


def test_resolve_table(lib):
    from pong_amd import _lib as K
    ADV, SOLO = K.PG_KERNEL_ADVANCE, K.PG_KERNEL_SOLO
    buf = (ctypes.c_uint8 * 32)()
    modes = {"plain": {}, "traced": {"trace": ctypes.addressof(buf), "trace_games": 1, "trace_cap": 1},
             "horizon": {"horizon": 37}, "hard_log": {"hard_log": ctypes.addressof(buf), "hard_cap": 1},
             "lanes16": {"group_lanes": 16}}
    named = {K.PG_ACT_SIGMOID: (K.PG_KERNEL_AUTO, K.PG_KERNEL_SPLIT, K.PG_KERNEL_GENERAL, K.PG_KERNEL_SIG2),
             K.PG_ACT_RELU: (K.PG_KERNEL_AUTO, K.PG_KERNEL_RELU, K.PG_KERNEL_RELU2, K.PG_KERNEL_GENERAL)}
    seen = set()
    for act, shape, bits, (mode, fields) in itertools.product(named, SHAPES, (0, ADV, SOLO, ADV | SOLO), modes.items()):
        for kernel in named[act]:
            a = _args(K, shape, kernel | bits, act, **fields)
            got = lib.pg_eval_resolve(ctypes.byref(a))
            # the same call as an empty launch: pg_eval_population's own verdict on entry
            rc = lib.pg_eval_population(ctypes.byref(a), None)
            msg = lib.pg_last_error()
            if rc != K.PG_OK:
                assert got == rc, (act, shape, kernel, bits, mode)
                assert lib.pg_eval_resolve(ctypes.byref(a)) == rc and lib.pg_last_error() == msg
                continue
            want = _expected(K, shape, act, kernel, bits, mode == "traced", mode == "horizon", mode == "hard_log",
                             16 if mode == "lanes16" else 0)
            assert got == want, (act, shape, kernel, hex(bits), mode, hex(got), hex(want))
            seen.add(got)
    # the table met the solo instance, the base under the bit, and both bits on a certified family
    assert {K.PG_KERNEL_SPLIT | SOLO, K.PG_KERNEL_SPLIT, K.PG_KERNEL_RELU | ADV | SOLO, K.PG_KERNEL_RELU2 | SOLO,
            K.PG_KERNEL_SIG2 | ADV, K.PG_KERNEL_GENERAL} <= seen
    # the widths at the scope's edges, spelled out
    for H, solo in ((32, False), (33, True), (64, True), (65, False)):
        got = lib.pg_eval_resolve(ctypes.byref(_args(K, [6, H, 3], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID)))
        assert got == K.PG_KERNEL_SPLIT | (SOLO if solo else 0), H
    got = lib.pg_eval_resolve(ctypes.byref(_args(K, [6, 64, 3], K.PG_KERNEL_AUTO | SOLO, K.PG_ACT_SIGMOID, group_lanes=8)))
    assert got == K.PG_KERNEL_SPLIT | SOLO


def test_refusals_are_pg_eval_populations(lib):
    from pong_amd import _lib as K
    ADV, SOLO, SIG = K.PG_KERNEL_ADVANCE, K.PG_KERNEL_SOLO, K.PG_ACT_SIGMOID
    assert lib.pg_eval_resolve(None) == K.PG_ERR_INVALID and b"NULL" in lib.pg_last_error()
    cases = (([6, 64, 3], K.PG_KERNEL_SPLIT | SOLO, SIG, {}, K.PG_ERR_UNSUPPORTED, b"PG_KERNEL_SOLO"),
             ([6, 64, 3], K.PG_KERNEL_SPLIT | SOLO | ADV, SIG, {}, K.PG_ERR_UNSUPPORTED, b"PG_KERNEL_ADVANCE"),
             ([6, 64, 3], K.PG_KERNEL_GENERAL | SOLO, SIG, {}, K.PG_ERR_UNSUPPORTED, b"PG_KERNEL_SOLO"),
             ([6, 64, 3], K.PG_KERNEL_AUTO | 0x200, SIG, {}, K.PG_ERR_INVALID, b"unknown bits"),
             ([6, 64, 3], K.PG_KERNEL_AUTO | SOLO, SIG, {"n_games": 0}, K.PG_ERR_INVALID, b"n_games"),
             ([6, 64, 3], K.PG_KERNEL_AUTO | SOLO, SIG, {"horizon": -1}, K.PG_ERR_INVALID, b"horizon"),
             ([6, 64, 3], K.PG_KERNEL_AUTO | SOLO, SIG, {"struct_size": 8}, K.PG_ERR_INVALID, b"struct_size"),
             ([5, 64, 3], K.PG_KERNEL_AUTO | SOLO, SIG, {}, K.PG_ERR_INVALID, b"6 inputs"),
             ([6, 64, 3], K.PG_KERNEL_SIG2 | SOLO, SIG, {}, K.PG_ERR_UNSUPPORTED, b""),
             ([6, 16, 16, 3], K.PG_KERNEL_RELU2 | SOLO, SIG, {}, K.PG_ERR_UNSUPPORTED, b""),
             ([6, 64, 64, 3], K.PG_KERNEL_RELU_WIDE, SIG, {}, K.PG_ERR_UNSUPPORTED, b""))
    for shape, kernel, act, fields, code, word in cases:
        a = _args(K, shape, kernel, act, **fields)
        assert lib.pg_eval_population(ctypes.byref(a), None) == code, (shape, hex(kernel))
        want = lib.pg_last_error()
        assert word in want and want, want
        assert lib.pg_eval_resolve(ctypes.byref(a)) == code and lib.pg_last_error() == want, (shape, hex(kernel))


def test_workspace_with_and_without_the_bit(lib):
    """The solo instance plays the base's lane records and keeps its second cursor in the work header."""
    from pong_amd import _lib as K
    for shape, dtype in itertools.product(([6, 32, 3], [6, 33, 2], [6, 64, 3], [6, 64, 4], [6, 65, 3]), (K.PG_F32, K.PG_F64)):
        sizes = {bits: lib.pg_eval_workspace_bytes(ctypes.byref(_args(K, shape, K.PG_KERNEL_AUTO | bits, K.PG_ACT_SIGMOID,
                                                                        n_genomes=4096, dtype=dtype)))
                 for bits in (0, K.PG_KERNEL_SOLO, K.PG_KERNEL_SOLO | K.PG_KERNEL_ADVANCE)}
        named = lib.pg_eval_workspace_bytes(ctypes.byref(_args(K, shape, K.PG_KERNEL_SPLIT, K.PG_ACT_SIGMOID, n_genomes=4096,
                                                               dtype=dtype)))
        assert len(set(sizes.values())) == 1 and sizes[0] == named > 256 + 4096 * 6 * 4, (shape, sizes)


def test_evaluator_resolved_kernel(lib, monkeypatch):
    """Evaluator.resolved_kernel touches no device: built here as on a GPU machine, it only asks the library."""
    import torch
    from pong_amd import _lib as K
    from pong_amd import device
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    ev = device.Evaluator([6, 64, 3], device="cuda:0", kernel="auto+solo")
    assert ev.resolved_kernel() == "split+solo"
    assert ev.resolved_kernel("auto") == "split" == ev.resolved_kernel("split")
    assert ev.resolved_kernel(traced=True) == "split" == ev.resolved_kernel(hard_log=True) == ev.resolved_kernel(horizon=37)
    assert ev.resolved_kernel(group_lanes=16) == "split" and ev.resolved_kernel(group_lanes=8) == "split+solo"
    assert ev.resolved_kernel("auto+advance+solo") == "split+solo" and ev.resolved_kernel("general") == "general"
    assert ev.resolved_kernel(precision="f64") == "general"
    with pytest.raises(KeyError):
        ev.resolved_kernel("split+solo")  # a reported name only: kernel_code still refuses it
    relu = device.Evaluator([6, 64, 3], device="cuda:0", activation="relu")
    assert relu.resolved_kernel("auto+advance+solo") == "relu+advance+solo"
    assert relu.resolved_kernel("auto+advance+solo", traced=True) == "relu+solo"
    assert relu.resolved_kernel("relu+solo") == "relu+solo" and relu.resolved_kernel() == "relu"
    with pytest.raises(K.PongGAError) as err:
        relu.resolved_kernel("sig2")
    assert err.value.code == K.PG_ERR_UNSUPPORTED
    assert device.Evaluator([6, 16, 16, 3], device="cuda:0").resolved_kernel("auto+solo") == "general"
    # kernel_name is kernel_code's inverse on every name it accepts
    for name in ("auto", "general", "split", "wide", "relu", "relu2", "relu_wide", "sig2", "relu+advance", "sig2+solo",
                 "relu2+advance+solo"):
        assert device.kernel_name(device.kernel_code(name)) == name
