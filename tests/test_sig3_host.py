"""k_sig3 without a GPU -- [6, 2..32, 2..32, 2..32, 2..4] sigmoid networks with
bias, three hidden layers on the lanes of a wave: the ABI value and the names,
the validation and kernel resolution of pg_eval_population with workspace =
NULL, the static f32 error bound (csrc/pg_sig3_bound.h, compiled for the host
with gcc) against its numpy restatement and against an f32 emulation of the
kernel's chain (tests/_sig3_model.py), the CPU oracle at depth 3 against plain
numpy, and the seeds of the populations that tests/test_gpu_sig3.py plays."""
import ctypes
import os
import re

import numpy as np
import pytest

import _sig3_cells as C
import _sig3_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")
CAP, U32, ETA = M.CAP, M.U32, M.ETA


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


# ------------------------------------------------------------ ABI and names ----
def test_kernel_value_and_names():
    from pong_amd import _lib, device
    text = open(HEADER).read()
    got = int(re.search(r"\bPG_KERNEL_SIG3\s*=\s*(\d+)", text).group(1))
    assert got == 13 == _lib.PG_KERNEL_SIG3 == device.DEEP_KERNELS["sig3"]
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    assert re.search(r"int32_t pg_sig3_decide\(const pg_relu_decide_args \*args, void \*stream\);", text)
    assert _lib.SIGNATURES["pg_sig3_decide"] == _lib.SIGNATURES["pg_relu_decide"]  # the same argument struct
    ADV, SOLO = _lib.PG_KERNEL_ADVANCE, _lib.PG_KERNEL_SOLO
    for name, code in (("sig3", 13), ("sig3+advance", 13 | ADV), ("sig3+solo", 13 | SOLO),
                       ("sig3+advance+solo", 13 | ADV | SOLO)):
        assert device.kernel_code(name) == code and device.kernel_name(code) == name
    assert device.kernel_code("sig3+solo+advance") == 13 | ADV | SOLO
    for bad in ("sig3+advance+advance", "sig3+", "sig3+fast", "sig3_block", "sig"):
        with pytest.raises(KeyError):
            device.kernel_code(bad)
    # the three pinned mappings are unchanged, and relu3 is where it was: the name lives next to it
    plain = ["auto", "general", "split", "wide", "relu", "relu2", "relu_wide", "sig2"]
    assert sorted(device.KERNELS) == sorted(plain + [n + "+advance" for n in ("relu", "relu2", "sig2", "auto")])
    assert device.MORE_KERNELS == {"relu2_block": 10} and device.BLOCK_KERNELS == {"sig2_block": 11}
    assert device.DEEP_KERNELS["relu3"] == 12 and sorted(device.DEEP_KERNELS) == ["relu3", "sig3"]
    assert hasattr(device.Evaluator, "sig3_decide")


def _args(_lib, shape, kernel=13, activation=None, bias=True, dtype=None, n_genomes=0, **fields):
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes = 6, n_genomes
    a.kernel = kernel
    a.net = _lib.make_net(shape, bias, _lib.PG_F32 if dtype is None else dtype,
                          activation=_lib.PG_ACT_SIGMOID if activation is None else activation)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_scope_without_a_gpu(lib):
    """Empty launches (workspace = NULL): every model shape is accepted with and without the modifier bits and
    pg_eval_resolve names what was asked; the refusals come in the family's words and pg_eval_resolve agrees; the
    workspace is the base one; AUTO is where it was."""
    from pong_amd import _lib as K
    ADV, SOLO = K.PG_KERNEL_ADVANCE, K.PG_KERNEL_SOLO

    def run(*a, **kw):
        return lib.pg_eval_population(ctypes.byref(_args(K, *a, **kw)), None)

    def refused(word, *a, **kw):
        assert run(*a, **kw) == K.PG_ERR_UNSUPPORTED, (a, kw)
        msg = lib.pg_last_error()
        assert word in msg, msg
        assert lib.pg_eval_resolve(ctypes.byref(_args(K, *a, **kw))) == K.PG_ERR_UNSUPPORTED
        assert lib.pg_last_error() == msg

    for shape in M.SHAPES:
        for dtype in (K.PG_F32, K.PG_F64):
            for bits in (0, ADV, SOLO, ADV | SOLO):
                assert run(shape, kernel=13 | bits, dtype=dtype) == K.PG_OK, (shape, bits)
                assert lib.pg_eval_resolve(ctypes.byref(_args(K, shape, kernel=13 | bits, dtype=dtype))) == 13 | bits
    for n_games in (1, 64):
        assert run([6, 16, 16, 16, 3], n_games=n_games) == K.PG_OK
    top = [6, 32, 32, 32, 3]
    refused(b"activation relu: the sig3 kernel evaluates sigmoid networks only (use RELU3)", top,
            activation=K.PG_ACT_RELU)
    for shape in ([6, 33, 2, 2, 2], [6, 2, 33, 2, 2], [6, 2, 2, 33, 2], [6, 1, 2, 2, 2], [6, 2, 2, 2, 5],
                  [6, 2, 2, 2, 1], [6, 8, 8, 3], [6, 8, 8, 8, 8, 3]):
        for bits in (0, ADV | SOLO):
            refused(b"sig3 kernel needs NETWORK_SHAPE [6, 2..32, 2..32, 2..32, 2..4]", shape, kernel=13 | bits)
    refused(b"sig3 kernel needs a network with bias", top, bias=False)
    refused(b"sig3 kernel is the certified-precision path", top, precision=K.PG_PREC_F64)
    refused(b"sig3 kernel: no fixed-horizon mode (horizon must be 0)", top, horizon=1000)
    refused(b"sig3 kernel: no hard-case log (hard_log must be NULL)", top, hard_log=1 << 20, hard_cap=8)
    # the workspace: the base size
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    for bits in (0, ADV, SOLO):
        assert lib.pg_eval_workspace_bytes(ctypes.byref(_args(K, top, kernel=13 | bits, n_genomes=4096))) == base
    # PG_KERNEL_AUTO does not pick it, with or without a modifier bit
    for bits in (0, ADV, SOLO, ADV | SOLO):
        a = _args(K, [6, 16, 16, 16, 3], kernel=K.PG_KERNEL_AUTO | bits)
        assert lib.pg_eval_resolve(ctypes.byref(a)) == K.PG_KERNEL_GENERAL


# ------------------------------------------------------------------ the bound ----
BOUND_SHAPES = [[6, 2, 2, 2, 2], [6, 16, 16, 16, 3], [6, 9, 32, 5, 3], [6, 32, 32, 32, 4]]


def test_bound_header_equals_numpy_restatement(tmp_path):
    """The gcc-compiled pg_sig3_bound_genome (which also pins the header's macros) against the same sums in
    numpy, in the same order: equal to one f32 ulp, inf included."""
    rng = np.random.default_rng(41)
    for shape in M.SHAPES:
        G = M.genes(shape)
        g = np.concatenate([rng.random((3, G)), rng.standard_normal((3, G)), rng.standard_normal((3, G)) * 30.0,
                            M.cap_net(shape, CAP * (1 + 1e-3))[None], M.cap_net(shape, CAP * (1 - 1e-3))[None],
                            M.tiny_net(shape, rng)[None], M.systematic_net(shape)[None], np.zeros((1, G))])
        g[0, rng.integers(0, G)] = np.nan
        g[3, rng.integers(0, G)] = 1e30
        g[6, rng.integers(0, G)] = np.inf
        got = M.bounds(tmp_path, shape, g)
        want = M.bound_np(shape, g)
        fin = np.isfinite(want)
        np.testing.assert_array_equal(np.isfinite(got), fin, err_msg=str(shape))
        assert (np.abs(got[fin].view(np.int32) - want[fin].view(np.int32)) <= 1).all(), shape
        assert np.isinf(got[[0, 3, 6, 9]]).all() and np.isfinite(got[[1, 2, 4, 5, 7, 8, 10, 11, 12, 13]]).all(), shape
        assert got[13] == np.float32(ETA * M.UNDER[3] * (1 + 2.0 ** -10))  # the zero genome: the underflow constant


def test_bound_covers_the_f32_chain(tmp_path):
    """2 000 random networks over four shapes, with U[0,1), N(0,1) and N(0,30) genes, x 8 inputs: the emulated
    f32 outputs lie within the bound of numpy's own np.dot chain's last pre-activations -- with every sigmoid
    as the rounded f64 one (sign = 0) and with every sigmoid displaced by its full allowance of 4.5 u towards
    and away from each output in turn (sign = +-1)."""
    rng = np.random.default_rng(43)
    worst, worst_adv, total = 0.0, 0.0, 0
    for shape in BOUND_SHAPES:
        n, G, O = 500, M.genes(shape), shape[-1]
        g = rng.random((n, G))
        g[n // 3:2 * n // 3] = rng.standard_normal((2 * n // 3 - n // 3, G))
        g[2 * n // 3:] = rng.standard_normal((n - 2 * n // 3, G)) * 30.0
        e = M.bounds(tmp_path, shape, g).astype(np.float64)
        assert e.shape == (n,) and np.isfinite(e).all() and (e > 0).all()
        k = rng.integers(0, 321, size=(n, 8, 6))
        ref = M.z64(shape, g, k)
        s = M.s_max(shape, g)
        err = np.abs(M.z32(shape, g, k).astype(np.float64) - ref).max(axis=(1, 2))
        assert (err <= e).all(), (shape, (err / e).max())
        worst = max(worst, float((err / (U32 * s)).max()))
        for out in range(O):
            for sign in (1.0, -1.0):
                z = M.z32(shape, g, k, out=out, sign=sign).astype(np.float64)
                err = np.abs(z - ref).max(axis=(1, 2))
                assert (err <= e).all(), (shape, out, sign, (err / e).max())
                worst_adv = max(worst_adv, float((err / (U32 * s)).max()))
        total += n
    assert total == 2000
    print(f"largest |z32 - z64| / (u max S_o) over {total * 8} passes: {worst:.4f} with rounded sigmoids, "
          f"{worst_adv:.4f} with every sigmoid displaced by 4.5 u (the bound: 1)")


def test_bound_on_built_networks(tmp_path):
    """cap_net on both sides of PG_SIG2_CAP (inf above; finite below, with z32 finite and within the bound),
    tiny_net (f32-subnormal genes: the underflow term governs and covers the chain), an all-positive systematic
    network on k = 320 (every conversion rounds the same way), and a bad gene in each of the eight blocks (inf)."""
    rng = np.random.default_rng(45)
    for shape in BOUND_SHAPES:
        above, below = M.cap_net(shape, CAP * (1 + 1e-3)), M.cap_net(shape, CAP * (1 - 1e-3))
        with np.errstate(all="ignore"):
            assert np.isfinite(above.astype(np.float32)).all()
        assert M.s_max(shape, above[None])[0] > CAP > M.s_max(shape, below[None])[0] > CAP * (1 - 2e-3)
        tiny, syst = M.tiny_net(shape, rng), M.systematic_net(shape)
        e = M.bounds(tmp_path, shape, np.array([above, below, tiny, syst])).astype(np.float64)
        assert np.isinf(e[0]) and np.isfinite(e[1:]).all() and (e[1:] > 0).all()
        k = np.concatenate([np.zeros((1, 6), np.int64), np.full((1, 6), 320), rng.integers(0, 321, size=(6, 6))])
        g3 = np.array([below, tiny, syst])
        kk = np.broadcast_to(k, (3,) + k.shape)
        z = M.z32(shape, g3, kk)
        assert np.isfinite(z).all()
        err = np.abs(z.astype(np.float64) - M.z64(shape, g3, kk)).max(axis=(1, 2))
        assert (err <= e[1:]).all(), (shape, err, e[1:])
        # tiny: u max S_o is far below eta, the underflow term is the bound
        assert U32 * M.s_max(shape, tiny[None])[0] < 1e-3 * ETA and ETA * M.UNDER[3] <= e[2] < ETA * (M.UNDER[3] + 1)
        # one bad gene in each of the eight blocks W1, b1, .., W4, b4
        at, nets = 0, []
        for a, b in zip(shape[:-1], shape[1:]):
            for pos in (at, at + a):
                for bad in (1e30, -1e30, np.nan, np.inf):
                    g = rng.standard_normal(M.genes(shape))
                    g[pos] = bad
                    nets.append(g)
            at += (a + 1) * b
        assert len(nets) == 32 and np.isinf(M.bounds(tmp_path, shape, np.array(nets))).all(), shape


# ------------------------------------------------------- the oracle at depth 3 ----
@pytest.mark.parametrize("shape", [[6, 5, 4, 3, 2], [6, 32, 32, 32, 4]], ids=str)
def test_oracle_depth_3_equals_numpy(oracle, shape):
    """oracle.nn_run with the sigmoid against np.dot, 1 / (1 + np.e ** -z) and np.argmax on N(0, sigma) networks,
    sigma in 0.3, 1, 3, 10, and on NaN / +-inf genes: the same index; the activations to 1e-15 (numpy's ** is
    not correctly rounded everywhere, the oracle's sigmoid is: the last bits may differ), NaN where numpy's are."""
    rng = np.random.default_rng(sum(shape))
    G = M.genes(shape)
    nets = [rng.standard_normal(G) * sigma for sigma in (0.3, 1.0, 3.0, 10.0) for _ in range(4)]
    for bad in (np.nan, np.inf, -np.inf):
        for _ in range(4):
            g = rng.standard_normal(G)
            g[rng.integers(0, G)] = bad
            nets.append(g)
    worst = 0.0
    for g in nets:
        ws = M.split(shape, g)
        for _ in range(8):
            k = rng.integers(0, 321, size=6)
            x = (k / 2) / 160
            with np.errstate(all="ignore"):
                a = np.append(x, 1.0)
                for w in ws:
                    h = 1 / (1 + np.e ** -np.dot(w, a))
                    a = np.append(h, 1.0)
            idx, act = oracle.nn_run(g, shape, x)
            assert idx == int(np.argmax(h))
            np.testing.assert_array_equal(np.isnan(act), np.isnan(h))
            ok = ~np.isnan(h)
            if ok.any():
                worst = max(worst, float(np.abs(act[ok] - h[ok]).max()))
    assert worst <= 1e-15
    print(f"{shape}: largest |oracle - numpy| over the activations {worst:.3g}")


# -------------------------------------------------- the game populations' seeds ----
@pytest.mark.parametrize("cell", C.CELLS, ids=C.cell_id)
def test_cell_population_meets_its_conditions(oracle, cell):
    """>= 6 % of the games timed out, >= 50 % ended by score, >= 1.5 % timed out after a point; the solo games
    differ in length."""
    from test_gpu_modifier_instances import check_cell_population, oracle_result
    pop = C.cell_population(cell)
    shares = check_cell_population(oracle, cell, pop, oracle_result(oracle, cell, pop), floors=C.FLOORS)
    print(f"{C.cell_id(cell)}: seed {C.SEEDS[cell[1]]}, timed out {shares[0]:.3f}, by score {shares[1]:.3f}, "
          f"timed out after a point {shares[2]:.3f}")
