"""The two-hidden-layer ReLU kernels without a GPU -- k_relu2 ([6, 2..64, 2..64,
2..4] with bias, a network on the lanes of a wave) and k_relu2_block (up to
128 x 128, a 256-thread block per game): the ABI values and the names, the
validation and kernel resolution of pg_eval_population with workspace = NULL,
and the static f32 error bound (csrc/pg_relu2_bound.h, compiled for the host
with gcc) under both layouts against its numpy restatement and against an f32
emulation of each kernel's chain (tests/_relu2_model.py, on
tests/_relu_model.py's once-rounded fma)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _relu2_model as M
from _relu2_model import BLOCK, LANES
from _relu_model import RELU_CAP, U32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")
LAYOUTS = pytest.mark.parametrize("layout", [LANES, BLOCK], ids=lambda l: l.name)


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


# ---------------------------------------------------------- k_relu2: ABI ----
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


# ------------------------------------------- k_relu2_block: ABI and naming ----
def test_kernel_value_and_names():
    from pong_amd import _lib, device
    text = open(HEADER).read()
    got = int(re.search(r"\bPG_KERNEL_RELU2_BLOCK\s*=\s*(\d+)", text).group(1))
    assert got == 10 == _lib.PG_KERNEL_RELU2_BLOCK
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    assert _lib.SIGNATURES["pg_relu2_block_decide"] == _lib.SIGNATURES["pg_relu_decide"]  # the same argument struct
    assert device.kernel_code("relu2_block") == 10 and device.kernel_name(10) == "relu2_block"
    # KERNELS itself is unchanged: the name lives in a second mapping
    plain = ["auto", "general", "split", "wide", "relu", "relu2", "relu_wide", "sig2"]
    assert sorted(device.KERNELS) == sorted(plain + [n + "+advance" for n in ("relu", "relu2", "sig2", "auto")])
    assert "relu2_block" not in device.KERNELS and device.MORE_KERNELS == {"relu2_block": 10}
    for bad in ("relu2_block+advance", "relu2_block+solo", "relu2_block+advance+solo", "relu2_block+"):
        with pytest.raises(KeyError) as err:
            device.kernel_code(bad)
        assert "+solo" in str(err.value) and "+advance" in str(err.value) and "relu2_block" in str(err.value), bad
    assert hasattr(device.Evaluator, "relu2_block_decide")


def _args(_lib, shape, kernel=None, activation=None, bias=True, dtype=None, n_genomes=0, **fields):
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes = 6, n_genomes
    a.kernel = _lib.PG_KERNEL_RELU2_BLOCK if kernel is None else kernel
    a.net = _lib.make_net(shape, bias, _lib.PG_F32 if dtype is None else dtype,
                          activation=_lib.PG_ACT_RELU if activation is None else activation)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_scope_without_a_gpu(lib):
    """The refusals in the family's words, for an empty launch (workspace =
    NULL, nothing allocated); the launch in scope is accepted; the workspace is
    the base one; pg_eval_resolve names the kernel; AUTO is where it was."""
    from pong_amd import _lib as K

    def run(*a, **kw):
        return lib.pg_eval_population(ctypes.byref(_args(K, *a, **kw)), None)

    def refused(word, *a, **kw):
        assert run(*a, **kw) == K.PG_ERR_UNSUPPORTED, (a, kw)
        msg = lib.pg_last_error()
        assert word in msg, msg
        args = _args(K, *a, **kw)
        assert lib.pg_eval_resolve(ctypes.byref(args)) == K.PG_ERR_UNSUPPORTED and lib.pg_last_error() == msg

    for shape in BLOCK.SHAPES + [[6, 64, 64, 3], [6, 16, 16, 2]]:
        for dtype in (K.PG_F32, K.PG_F64):
            assert run(shape, dtype=dtype) == K.PG_OK, shape
            assert lib.pg_eval_resolve(ctypes.byref(_args(K, shape, dtype=dtype))) == 10
    top = [6, 128, 128, 3]
    refused(b"sigmoid", top, activation=K.PG_ACT_SIGMOID)
    for shape in ([6, 128, 3], [6, 129, 128, 3], [6, 128, 129, 3], [6, 1, 128, 3], [6, 128, 1, 3], [6, 128, 128, 5],
                  [6, 128, 128, 1], [6, 8, 8, 8, 2]):
        refused(b"relu2_block kernel needs NETWORK_SHAPE [6, 2..128, 2..128, 2..4] with bias", shape)
    refused(b"bias", top, bias=False)
    refused(b"relu2_block kernel is the certified-precision path", top, precision=K.PG_PREC_F64)
    refused(b"relu2_block kernel plays whole episodes", top, horizon=1000)
    buf = (ctypes.c_uint32 * 8)()
    refused(b"relu2_block kernel keeps no hard-case log", top, hard_log=ctypes.cast(buf, ctypes.c_void_p), hard_cap=1)
    # the modifier bits, as on every explicit kernel outside the three certified families: advance first, then solo
    ADV, SOLO = K.PG_KERNEL_ADVANCE, K.PG_KERNEL_SOLO
    refused(b"PG_KERNEL_ADVANCE: kernel=10", top, kernel=10 | ADV)
    refused(b"PG_KERNEL_ADVANCE: kernel=10", top, kernel=10 | ADV | SOLO)
    refused(b"PG_KERNEL_SOLO: kernel=10", top, kernel=10 | SOLO)
    # the workspace: the base size, relu2's
    a = _args(K, [6, 64, 64, 3], n_genomes=4096)
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) == base
    a.kernel = K.PG_KERNEL_RELU2
    assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) == base
    assert lib.pg_eval_workspace_bytes(ctypes.byref(_args(K, top, n_genomes=4096))) == base
    # PG_KERNEL_AUTO is unchanged: such networks still resolve to the general kernel
    for shape in ([6, 100, 100, 3], [6, 128, 128, 3], [6, 65, 2, 2]):
        assert lib.pg_eval_resolve(ctypes.byref(_args(K, shape, kernel=K.PG_KERNEL_AUTO))) == K.PG_KERNEL_GENERAL
    assert lib.pg_eval_resolve(ctypes.byref(_args(K, [6, 64, 64, 3], kernel=K.PG_KERNEL_AUTO))) == K.PG_KERNEL_RELU2


# ------------------------------------------------- the bound, both layouts ----
@LAYOUTS
def test_bound_header_equals_numpy_restatement(tmp_path, layout):
    """The gcc-compiled pg_relu2_bound_genome against the same sums in numpy, in
    the same order: equal as f32 values, inf included."""
    rng = np.random.default_rng(21)
    for shape in layout.SHAPES:
        G = M.genes(shape)
        g = np.concatenate([rng.random((3, G)), rng.standard_normal((3, G)), rng.standard_normal((3, G)) * 30.0,
                            M.cap_net(shape, RELU_CAP * (1 + 1e-3))[None], M.cap_net(shape, RELU_CAP * (1 - 1e-3))[None],
                            M.tiny_net(shape, rng)[None], M.systematic_net(shape)[None], np.zeros((1, G))])
        g[0, rng.integers(0, G)] = np.nan
        g[3, rng.integers(0, G)] = 1e30
        got = M.bounds(tmp_path, layout, shape, g).astype(np.float32)
        want = M.bound_numpy(layout, shape, g)
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg=str(shape))
        assert np.isinf(got[[0, 3, 9]]).all() and np.isfinite(got[[1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13]]).all()


CELLS = [(2, 2), (16, 16), (17, 33), (64, 64)]
# each layout's draw of 2 000 networks: the seed, (shape, networks) in order, inputs per network
_DRAWS = {"lanes": (13, [([6, H1, H2, O], 167 if (c, O) != (0, 2) else 163)  # 11 x 167 + 163 = 2 000
                         for c, (H1, H2) in enumerate(CELLS) for O in (2, 3, 4)], 8),
          "block": (23, [(shape, 200) for shape in BLOCK.SHAPES], 4)}


@LAYOUTS
def test_bound_covers_the_f32_chain(tmp_path, layout):
    """2 000 random networks across the layout's shapes, with U[0,1), N(0,1) and
    N(0,30) genes, x 8 (lanes) or 4 (block) inputs: the emulated f32 outputs lie
    within the bound of numpy's own np.dot chain, the bound is at most
    2 K u max_o S_o, and |z32 - z64| / (u max_o S_o) stays below K."""
    seed, cases, m = _DRAWS[layout.name]
    rng = np.random.default_rng(seed)
    worst, total = 0.0, 0
    for shape, n in cases:
        G = M.genes(shape)
        g = rng.random((n, G))
        g[n // 3:2 * n // 3] = rng.standard_normal((2 * n // 3 - n // 3, G))
        g[2 * n // 3:] = rng.standard_normal((n - 2 * n // 3, G)) * 30.0
        e = M.bounds(tmp_path, layout, shape, g)
        assert e.shape == (n,) and np.isfinite(e).all() and (e > 0).all()
        k = rng.integers(0, 321, size=(n, m, 6))
        err = np.abs(M.z32(layout, shape, g, k).astype(np.float64) - M.z64(shape, g, k)).max(axis=(1, 2))
        s = M.s_max(shape, g)
        assert (err <= e).all(), (shape, (err / e).max())
        assert (e <= 2 * layout.K * U32 * s).all(), shape
        ratio = float((err / (U32 * s)).max())
        assert ratio < layout.K, (shape, ratio)
        worst = max(worst, ratio)
        total += n
    assert total == 2000
    print(f"largest |z32 - z64| / (u max S_o) over {total * m} passes: {worst:.3f} (the bound: K = {layout.K:.0f})")


# ---------------------------------------------- the bound, the lane layout ----
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
        e = M.bounds(tmp_path, LANES, shape, np.array(nets))
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
            e = M.bounds(tmp_path, LANES, shape, np.array([above, below]))
            assert np.isinf(e[0]) and np.isfinite(e[1])
            k = np.concatenate([np.zeros((1, 6), np.int64), np.full((1, 6), 320), rng.integers(0, 321, size=(14, 6))])[None]
            z = M.z32(LANES, shape, below[None], k)
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
        e = M.bounds(tmp_path, LANES, shape, g)
        assert np.isfinite(e).all() and (e > 0).all() and (M.s_max(shape, g) < 1e-30).all()
        k = rng.integers(0, 321, size=(4, 16, 6))
        err = np.abs(M.z32(LANES, shape, g, k).astype(np.float64) - M.z64(shape, g, k)).max(axis=(1, 2))
        assert (err <= e).all(), (shape, err, e)
        assert (e >= 2.0 ** -126).all()  # the underflow term, not K u S


# --------------------------------------------- the bound, the block layout ----
def test_bound_on_built_networks(tmp_path):
    """cap_net on both sides of PG_RELU_CAP (inf above; finite below, with z32
    finite and within the bound), tiny_net (f32-subnormal genes: the underflow
    term covers the chain) and an all-positive systematic network on k = 320
    (every rounding the same way: the largest ratio a network reaches)."""
    rng = np.random.default_rng(25)
    worst = 0.0
    for shape in BLOCK.SHAPES:
        above, below = M.cap_net(shape, RELU_CAP * (1 + 1e-3)), M.cap_net(shape, RELU_CAP * (1 - 1e-3))
        assert np.isfinite(above.astype(np.float32)).all()
        assert M.s_max(shape, above) > RELU_CAP > M.s_max(shape, below) > RELU_CAP * (1 - 2e-3)
        tiny, syst = M.tiny_net(shape, rng), M.systematic_net(shape)
        e = M.bounds(tmp_path, BLOCK, shape, np.array([above, below, tiny, syst]))
        assert np.isinf(e[0]) and np.isfinite(e[1:]).all() and (e[1:] > 0).all()
        k = np.concatenate([np.zeros((1, 6), np.int64), np.full((1, 6), 320), rng.integers(0, 321, size=(6, 6))])
        g3 = np.array([below, tiny, syst])
        z = M.z32(BLOCK, shape, g3, np.broadcast_to(k, (3,) + k.shape))
        assert np.isfinite(z).all()
        err = np.abs(z.astype(np.float64) - M.z64(shape, g3, np.broadcast_to(k, (3,) + k.shape))).max(axis=(1, 2))
        assert (err <= e[1:]).all(), (shape, err, e[1:])
        assert M.s_max(shape, tiny) < 1e-30 and e[2] >= 2.0 ** -126  # the underflow term, not K u S
        ratio = err[2] / (U32 * M.s_max(shape, syst))
        assert ratio < BLOCK.K, (shape, ratio)
        worst = max(worst, float(ratio))
    print(f"largest |z32 - z64| / (u max S_o) of the systematic networks: {worst:.3f} (K = {BLOCK.K:.0f})")
