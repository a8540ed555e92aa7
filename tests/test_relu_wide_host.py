"""PG_KERNEL_RELU_WIDE (k_wide's ReLU instances: [6, 2..512, 2..512, 2..4] ReLU
networks) without a GPU: the ABI values and signatures, the workspace sizes,
pg_eval_population's scope checks on an empty launch, the config knob, and
the committed fixture's own consistency."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


def test_kernel_value_and_signatures_match_header():
    from pong_amd import _lib, device
    text = open(HEADER).read()
    got = int(re.search(r"\bPG_KERNEL_RELU_WIDE\s*=\s*(\d+)", text).group(1))
    assert got == 8 == _lib.PG_KERNEL_RELU_WIDE
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    assert device.KERNELS["relu_wide"] == 8
    for name in ("pg_relu_wide_decide", "pg_relu_wide_decide_workspace_bytes"):
        assert re.search(rf"\b{name}\(const pg_wide_decide_args \*", text), name
    # the same argument struct as pg_wide_decide
    assert _lib.SIGNATURES["pg_relu_wide_decide"] == _lib.SIGNATURES["pg_wide_decide"]
    assert _lib.SIGNATURES["pg_relu_wide_decide_workspace_bytes"] == _lib.SIGNATURES["pg_wide_decide_workspace_bytes"]
    assert hasattr(device.Evaluator, "relu_wide_decide")


def test_workspace_bytes(lib):
    """RELU_WIDE on a ReLU [6,512,512,3] f32: the base plus k_wide's W2 copies --
    the sigmoid WIDE's byte count exactly; AUTO on the same net: the base."""
    from pong_amd import _lib
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes = 6, 4096
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    a.net = _lib.make_net([6, 512, 512, 3], True, _lib.PG_F32, activation=_lib.PG_ACT_RELU)
    a.kernel = _lib.PG_KERNEL_RELU_WIDE
    relu_wide = lib.pg_eval_workspace_bytes(ctypes.byref(a))
    a.kernel = _lib.PG_KERNEL_AUTO
    assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) == base
    a.net = _lib.make_net([6, 512, 512, 3], True, _lib.PG_F32, activation=_lib.PG_ACT_SIGMOID)
    a.kernel = _lib.PG_KERNEL_WIDE
    wide = lib.pg_eval_workspace_bytes(ctypes.byref(a))
    assert relu_wide > base
    assert relu_wide == wide


def _empty_launch(lib, shape, bias=True, activation=None, precision=None, dtype=None):
    from pong_amd import _lib
    e = _lib.PgEvalArgs()
    e.n_games, e.n_genomes, e.kernel = 6, 0, _lib.PG_KERNEL_RELU_WIDE
    e.precision = _lib.PG_PREC_CERTIFIED if precision is None else precision
    e.net = _lib.make_net(shape, bias, _lib.PG_F32 if dtype is None else dtype,
                          activation=_lib.PG_ACT_RELU if activation is None else activation)
    return lib.pg_eval_population(ctypes.byref(e), None)


@pytest.mark.parametrize("shape", [[6, 512, 512, 3], [6, 2, 2, 2], [6, 100, 130, 4]])
def test_empty_launch_accepts_the_scope(lib, shape):
    from pong_amd import _lib
    for dtype in (_lib.PG_F32, _lib.PG_F64):
        for bias in (True, False):
            for precision in (_lib.PG_PREC_CERTIFIED, _lib.PG_PREC_F64):
                rc = _empty_launch(lib, shape, bias=bias, precision=precision, dtype=dtype)
                assert rc == _lib.PG_OK, (shape, dtype, bias, precision, lib.pg_last_error())


def test_empty_launch_refuses_a_sigmoid_net(lib):
    from pong_amd import _lib
    assert _empty_launch(lib, [6, 512, 512, 3], activation=_lib.PG_ACT_SIGMOID) == _lib.PG_ERR_UNSUPPORTED
    assert b"sigmoid" in lib.pg_last_error()


@pytest.mark.parametrize("shape", [[6, 64, 3], [6, 513, 64, 3], [6, 64, 513, 3], [6, 1, 64, 3], [6, 64, 1, 3],
                                   [6, 64, 64, 5], [6, 8, 8, 8, 2]])
def test_empty_launch_refuses_shapes_outside_the_scope(lib, shape):
    from pong_amd import _lib
    assert _empty_launch(lib, shape) == _lib.PG_ERR_UNSUPPORTED
    assert b"relu_wide" in lib.pg_last_error()


def test_config_kernel_knob():
    import config
    assert config.KERNEL == "auto"
    import inspect

    from pong_amd import runtime
    assert inspect.signature(runtime.evaluator).parameters["kernel"].default == "auto"


def test_fixture_is_consistent(golden):
    """relu_forward_wide.npz: data only, both shapes, 32 grid inputs per network,
    the stored argmax and run() agree with the stored activations, and the
    [6,512,512,2] genes regenerate from their seeds."""
    g = golden("relu_forward_wide.npz")
    for key, n_genomes in (("6x100x130x2", 4), ("6x512x512x2", 2)):
        shape = [int(v) for v in g[f"{key}__shape"]]
        assert "x".join(map(str, shape)) == key
        k, x, act, idx, run = (g[f"{key}__{f}"] for f in ("k", "x", "act", "idx", "run"))
        assert k.shape == (32 * n_genomes, 6) and k.min() >= 0 and k.max() <= 320
        np.testing.assert_array_equal(x, k / 320.0)
        np.testing.assert_array_equal(np.bincount(g[f"{key}__gidx"]), [32] * n_genomes)
        assert act.shape == (32 * n_genomes, 2) and (act >= 0).all()
        np.testing.assert_array_equal(idx, np.argmax(act, axis=1))
        np.testing.assert_array_equal(run, np.eye(2, dtype=np.int8)[idx])
    assert g["6x100x130x2__genes"].shape == (4, 7 * 100 + 101 * 130 + 131 * 2)
    G = 7 * 512 + 513 * 512 + 513 * 2
    for seed, dist, sha in zip(g["6x512x512x2__seed"], g["6x512x512x2__dist"], g["6x512x512x2__genes_sha256"]):
        rng = np.random.default_rng(int(seed))
        genes = rng.random(G) if str(dist) == "init" else rng.standard_normal(G)
        genes = genes.astype(np.float32).astype(np.float64)
        assert hashlib.sha256(genes.tobytes()).hexdigest() == str(sha)
