"""k_relu2 (ReLU networks with two hidden layers, [6, 2..64, 2..64, 2..4] with
bias) without a GPU: the ABI values, the validation and kernel resolution of
pg_eval_population, and the static f32 error bound (csrc/pg_relu2_bound.h,
compiled for the host with gcc) against an f32 emulation of the kernel's chain
(tests/_relu2_model.py, on tests/_relu_model.py's once-rounded fma)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _relu2_model as M
from _relu_model import RELU_CAP, U32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


# ------------------------------------------------------------------- ABI ----
def test_kernel_value_matches_header():
    from pong_amd import _lib, device
    text = open(HEADER).read()
    got = int(re.search(r"\bPG_KERNEL_RELU2\s*=\s*(\d+)", text).group(1))
    assert got == 7 == _lib.PG_KERNEL_RELU2
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    assert "pg_relu2_decide" in _lib.SIGNATURES
    assert _lib.SIGNATURES["pg_relu2_decide"] == _lib.SIGNATURES["pg_relu_decide"]  # the same argument struct
    assert device.KERNELS["relu2"] == 7


def test_workspace_bytes_and_scope(lib):
    """AUTO and RELU2 on a ReLU [6,64,64,3] need only the base workspace; an
    empty launch accepts RELU2 for an in-scope net and refuses everything
    outside the kernel's scope."""
    from pong_amd import _lib
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes = 6, 4096
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    a.net = _lib.make_net([6, 64, 64, 3], True, _lib.PG_F32, activation=_lib.PG_ACT_RELU)
    for kernel in (_lib.PG_KERNEL_AUTO, _lib.PG_KERNEL_RELU2):
        a.kernel = kernel
        assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) == base

    def run(shape, bias=True, activation=_lib.PG_ACT_RELU, precision=_lib.PG_PREC_CERTIFIED, dtype=_lib.PG_F32):
        e = _lib.PgEvalArgs()
        e.n_games, e.n_genomes, e.kernel, e.precision = 6, 0, _lib.PG_KERNEL_RELU2, precision
        e.net = _lib.make_net(shape, bias, dtype, activation=activation)
        return lib.pg_eval_population(ctypes.byref(e), None)

    for shape in ([6, 64, 64, 3], [6, 2, 2, 2], [6, 17, 33, 4]):
        for dtype in (_lib.PG_F32, _lib.PG_F64):
            assert run(shape, dtype=dtype) == _lib.PG_OK
    assert run([6, 64, 64, 3], activation=_lib.PG_ACT_SIGMOID) == _lib.PG_ERR_UNSUPPORTED
    assert b"sigmoid" in lib.pg_last_error()
    for shape in ([6, 64, 3], [6, 65, 64, 3], [6, 64, 65, 3], [6, 1, 64, 3], [6, 64, 1, 3], [6, 64, 64, 5],
                  [6, 8, 8, 8, 2]):
        assert run(shape) == _lib.PG_ERR_UNSUPPORTED, shape
        assert b"relu2" in lib.pg_last_error()
    assert run([6, 64, 64, 3], bias=False) == _lib.PG_ERR_UNSUPPORTED
    assert run([6, 64, 64, 3], precision=_lib.PG_PREC_F64) == _lib.PG_ERR_UNSUPPORTED
    assert b"certified" in lib.pg_last_error()


# ----------------------------------------------------------------- bound ----
CELLS = [(2, 2), (16, 16), (17, 33), (64, 64)]


def test_bound_covers_the_f32_chain(tmp_path):
    """2 000 random networks x 8 inputs: the emulated f32 outputs lie within the
    bound of numpy's own np.dot chain, and the bound is at most 2 K u max_o S_o."""
    rng = np.random.default_rng(13)
    worst, total = 0.0, 0
    for c, (H1, H2) in enumerate(CELLS):
        for O in (2, 3, 4):
            shape = [6, H1, H2, O]
            n = 167 if (c, O) != (0, 2) else 163  # 11 x 167 + 163 = 2 000
            G = M.genes(shape)
            g = rng.random((n, G))
            g[n // 3:2 * n // 3] = rng.standard_normal((2 * n // 3 - n // 3, G))
            g[2 * n // 3:] = rng.standard_normal((n - 2 * n // 3, G)) * 30.0
            e = M.bounds(tmp_path, shape, g)
            assert e.shape == (n,) and np.isfinite(e).all() and (e > 0).all()
            k = rng.integers(0, 321, size=(n, 8, 6))
            err = np.abs(M.z32(shape, g, k).astype(np.float64) - M.z64(shape, g, k)).max(axis=(1, 2))
            s = M.s_max(shape, g)
            assert (err <= e).all(), (shape, (err / e).max())
            assert (e <= 2 * M.RELU2_K * U32 * s).all(), shape
            worst = max(worst, float((err / (U32 * s)).max()))
            total += n
    assert total == 2000
    print(f"largest |z32 - z64| / (u max S_o) over 16 000 passes: {worst:.3f} (the bound: K = {M.RELU2_K:.0f})")


def _positions(shape):
    """One gene of each of the six blocks: W1, b1, W2, b2, W3, b3."""
    _, H1, H2, O = shape
    a, b = H1 * 7, H1 * 7 + H2 * (H1 + 1)
    return [0, 6, a, a + H1, b, b + H2]


def test_bound_is_inf_for_genes_f32_sums_cannot_hold(tmp_path):
    rng = np.random.default_rng(14)
    for shape in ([6, 2, 2, 2], [6, 17, 33, 4], [6, 64, 64, 3]):
        G = M.genes(shape)
        nets, finite = [], []
        for pos in _positions(shape):
            for bad in (1e30, -1e30, np.nan, np.inf):
                g = rng.standard_normal(G)
                g[pos] = bad
                nets.append(g)
                finite.append(False)
        nets.append(rng.standard_normal(G))
        finite.append(True)
        e = M.bounds(tmp_path, shape, np.array(nets))
        np.testing.assert_array_equal(np.isfinite(e), finite)


def test_bound_at_the_cap(tmp_path):
    """max_o S_o just above PG_RELU_CAP: inf.  Just below: finite, z32 finite
    and still within the bound of numpy's chain."""
    rng = np.random.default_rng(15)
    for H1, H2 in CELLS:
        for O in (2, 3, 4):
            shape = [6, H1, H2, O]
            above, below = M.cap_net(shape, RELU_CAP * (1 + 1e-3)), M.cap_net(shape, RELU_CAP * (1 - 1e-3))
            assert np.isfinite(above.astype(np.float32)).all()
            assert M.s_max(shape, above) > RELU_CAP > M.s_max(shape, below) > RELU_CAP * (1 - 2e-3)
            e = M.bounds(tmp_path, shape, np.array([above, below]))
            assert np.isinf(e[0]) and np.isfinite(e[1])
            k = np.concatenate([np.zeros((1, 6), np.int64), np.full((1, 6), 320), rng.integers(0, 321, size=(14, 6))])[None]
            z = M.z32(shape, below[None], k)
            assert np.isfinite(z).all()
            err = np.abs(z.astype(np.float64) - M.z64(shape, below[None], k)).max()
            assert err <= e[1], (shape, err, e[1])


def test_bound_covers_subnormal_genes(tmp_path):
    """Genes of 1e-36 .. 1e-60 (f32 subnormals, or zero in f32): u max S_o says
    nothing there, the underflow term covers the chain."""
    rng = np.random.default_rng(16)
    for H1, H2 in CELLS:
        shape = [6, H1, H2, 3]
        g = np.array([M.tiny_net(shape, rng) for _ in range(4)])
        e = M.bounds(tmp_path, shape, g)
        assert np.isfinite(e).all() and (e > 0).all() and (M.s_max(shape, g) < 1e-30).all()
        k = rng.integers(0, 321, size=(4, 16, 6))
        err = np.abs(M.z32(shape, g, k).astype(np.float64) - M.z64(shape, g, k)).max(axis=(1, 2))
        assert (err <= e).all(), (shape, err, e)
        assert (e >= 2.0 ** -126).all()  # the underflow term, not K u S
