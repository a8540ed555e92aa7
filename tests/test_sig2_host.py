"""k_sig2 (sigmoid networks with two hidden layers, [6, 2..64, 2..64, 2..4] with
bias) without a GPU: the ABI values, the scope checks of pg_eval_population, and
the static f32 error bound (csrc/pg_sig2_bound.h, compiled for the host with
gcc) against its numpy restatement and against an f32 emulation of the kernel's
chain whose every sigmoid is displaced adversarially by the full allowance
(tests/_sig2_model.py, on tests/_relu_model.py's once-rounded fma)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _sig2_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")
CELLS = [(2, 2), (16, 16), (17, 33), (64, 64)]


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
    got = int(re.search(r"\bPG_KERNEL_SIG2\s*=\s*(\d+)", text).group(1))
    assert got == 9 == _lib.PG_KERNEL_SIG2 == device.KERNELS["sig2"]
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    assert _lib.SIGNATURES["pg_sig2_decide"] == _lib.SIGNATURES["pg_relu_decide"]  # the same argument struct
    assert re.search(r"\bpg_sig2_decide\(const pg_relu_decide_args \*", text)


def test_scope_refusals_hold_for_an_empty_launch(lib):
    """PG_KERNEL_SIG2 with n_genomes = 0: PG_OK inside the scope, and each
    refusal with its word outside it; the workspace is the base alone."""
    from pong_amd import _lib
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes, a.kernel = 6, 4096, _lib.PG_KERNEL_SIG2
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    for shape in ([6, 64, 64, 3], [6, 16, 16, 3]):
        a.net = _lib.make_net(shape, True, _lib.PG_F64)
        assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) == base

    def run(shape, bias=True, activation=_lib.PG_ACT_SIGMOID, precision=_lib.PG_PREC_CERTIFIED, dtype=_lib.PG_F32,
            horizon=0, hard_log=None):
        e = _lib.PgEvalArgs()
        e.n_games, e.n_genomes, e.kernel, e.precision, e.horizon = 6, 0, _lib.PG_KERNEL_SIG2, precision, horizon
        if hard_log is not None:
            e.hard_log, e.hard_cap = ctypes.addressof(hard_log), 4  # (never written: the call is refused)
        e.net = _lib.make_net(shape, bias, dtype, activation=activation)
        return lib.pg_eval_population(ctypes.byref(e), None)

    def refused(word, *args, **kw):
        assert run(*args, **kw) == _lib.PG_ERR_UNSUPPORTED, (args, kw)
        assert word in lib.pg_last_error(), lib.pg_last_error()

    for shape in ([6, 64, 64, 3], [6, 2, 2, 2], [6, 17, 33, 4]):
        for dtype in (_lib.PG_F32, _lib.PG_F64):
            assert run(shape, dtype=dtype) == _lib.PG_OK
    refused(b"sigmoid", [6, 64, 64, 3], activation=_lib.PG_ACT_RELU)
    for shape in ([6, 64, 3], [6, 65, 64, 3], [6, 64, 65, 3], [6, 1, 64, 3], [6, 64, 1, 3], [6, 64, 64, 5],
                  [6, 8, 8, 8, 2]):
        refused(b"sig2", shape)
    refused(b"bias", [6, 64, 64, 3], bias=False)
    refused(b"certified", [6, 64, 64, 3], precision=_lib.PG_PREC_F64)
    refused(b"horizon", [6, 64, 64, 3], horizon=1000)
    refused(b"hard", [6, 64, 64, 3], hard_log=(ctypes.c_uint32 * 32)())


# ----------------------------------------------------------------- bound ----
def _positions(shape):
    """One gene of each of the six blocks: W1, b1, W2, b2, W3, b3."""
    _, H1, H2, O = shape
    a, b = H1 * 7, H1 * 7 + H2 * (H1 + 1)
    return [0, 6, a, a + H1, b, b + H2]


def _ulp_equal(a, b):
    """Equal to one f32 ulp (both inf counts as equal)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both_inf = np.isinf(a) & np.isinf(b)
    with np.errstate(all="ignore"):
        near = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.minimum(a, b))
    return both_inf | (np.isfinite(a) & np.isfinite(b) & near)


def test_bound_equals_its_numpy_restatement(tmp_path):
    rng = np.random.default_rng(21)
    for H1, H2 in CELLS + [(64, 2), (5, 4)]:
        for O in (2, 3, 4):
            shape = [6, H1, H2, O]
            G = M.genes(shape)
            g = np.concatenate([rng.random((8, G)), rng.standard_normal((8, G)), rng.standard_normal((8, G)) * 30.0,
                                rng.standard_normal((4, G)) * 1e-38])
            e = M.bounds(tmp_path, shape, g)
            assert np.isfinite(e).all() and (e > 0).all()
            assert _ulp_equal(e, M.bound_np(shape, g)).all(), shape


def test_bound_is_inf_for_genes_f32_sums_cannot_hold(tmp_path):
    """A NaN gene, an inf gene and a gene of 1e30 in any of the six blocks: e = inf, in C and in the restatement."""
    rng = np.random.default_rng(22)
    for shape in ([6, 2, 2, 2], [6, 17, 33, 4], [6, 64, 64, 3]):
        G = M.genes(shape)
        nets, finite = [], []
        for pos in _positions(shape):
            for bad in (1e30, -1e30, np.nan, np.inf, -np.inf):
                g = rng.standard_normal(G)
                g[pos] = bad
                nets.append(g)
                finite.append(False)
        nets.append(rng.standard_normal(G))
        finite.append(True)
        e = M.bounds(tmp_path, shape, np.array(nets))
        np.testing.assert_array_equal(np.isfinite(e), finite)
        np.testing.assert_array_equal(np.isfinite(M.bound_np(shape, np.array(nets))), finite)


def _scaled(shape, g, which, target):
    """g with one block scaled so that one capped sum of pg_sig2_bound.h equals target while the others stay far
    below it: 'A' scales W1 (sum_j A_j) and 'B' W2's bias column (sum_k B_k), both under small W2 and W3 weights;
    'S_bias' sets the output biases (S_o through 11 |b3_o|), 'S_w3' scales W3's weights under zero output biases."""
    _, H1, H2, O = shape
    w1, w2, w3 = (w.copy() for w in M.split(shape, g))
    if which in ("A", "B"):
        w2[:, :H1] *= 1e-3
        w3[:, :H2] *= 1e-4
    if which == "A":
        w1 *= target / np.abs(w1).sum()
    elif which == "B":
        w2[:, H1] *= (target - np.abs(w2[:, :H1]).sum()) / np.abs(w2[:, H1]).sum()
    elif which == "S_bias":
        w3[:, :H2] = 0.0
        w3[:, H2] = target / M.CHAIN3 * np.sign(w3[:, H2])
    else:
        w3[:, H2] = 0.0
        w3[:, :H2] *= target / M.sums(shape, M.pack(w1, w2, w3))[0].max()
    return M.pack(w1, w2, w3)


def test_bound_at_the_cap(tmp_path):
    """Each capped sum just above PG_SIG2_CAP: inf.  Just below: finite, the
    emulated z32 finite and within the bound of numpy's chain."""
    rng = np.random.default_rng(23)
    for H1, H2 in CELLS:
        shape = [6, H1, H2, 3]
        base = rng.standard_normal(M.genes(shape)) * 0.1
        for which in ("A", "B", "S_bias", "S_w3"):
            above, below = (_scaled(shape, base, which, M.CAP * f) for f in (1 + 1e-3, 1 - 1e-3))
            assert np.isfinite(above.astype(np.float32)).all()
            e = M.bounds(tmp_path, shape, np.array([above, below]))
            assert np.isinf(e[0]) and np.isfinite(e[1]), (shape, which, e)
            assert _ulp_equal(e, M.bound_np(shape, np.array([above, below]))).all()
            k = np.concatenate([np.zeros((1, 6), np.int64), np.full((1, 6), 320), rng.integers(0, 321, size=(6, 6))])[None]
            z = M.z32(shape, below[None], k)
            assert np.isfinite(z).all()
            err = np.abs(z.astype(np.float64) - M.z64(shape, below[None], k)).max()
            assert err <= e[1], (shape, which, err, e[1])


# ------------------------------------------------------------- soundness ----
def _families(rng, shape, n):
    """n networks in five families: U[0,1), N(0,1), N(0,3), N(0,30), all-positive systematic."""
    G = M.genes(shape)
    q = n // 5
    sysnet = (0.05 + 0.9 * ((np.arange(G)[None, :] * 7 + np.arange(n - 4 * q)[:, None] * 13) % 31) / 31.0)
    return {"U[0,1)": rng.random((q, G)), "N(0,1)": rng.standard_normal((q, G)),
            "N(0,3)": rng.standard_normal((q, G)) * 3.0, "N(0,30)": rng.standard_normal((q, G)) * 30.0,
            "positive": sysnet}


def test_bound_covers_the_adversarial_f32_chain(tmp_path):
    """2 000 networks x 8 inputs: with every emulated f32 sigmoid displaced by
    the full 4.5 u towards, then away from, one output, that output's emulated
    z32 stays within e of numpy's own np.dot chain.  Prints the largest ratio,
    and per shape the share of the N(0,1) passes the restated certificate decides."""
    rng = np.random.default_rng(24)
    worst, total = 0.0, 0
    shares = {}
    for c, (H1, H2) in enumerate(CELLS):
        for O in (2, 3, 4):
            shape = [6, H1, H2, O]
            n = 167 if (c, O) != (0, 2) else 163  # 11 x 167 + 163 = 2 000
            for name, g in _families(rng, shape, n).items():
                e = M.bounds(tmp_path, shape, g)
                assert np.isfinite(e).all() and (e > 0).all()
                k = rng.integers(0, 321, size=(len(g), 8, 6))
                ref = M.z64(shape, g, k)
                out = int(rng.integers(0, O))
                for sign in (1.0, -1.0, 0.0):
                    z = M.z32(shape, g, k, out=out, sign=sign).astype(np.float64)
                    err = np.abs(z - ref)[:, :, out] if sign else np.abs(z - ref).max(axis=2)
                    ratio = float((err.max(axis=1) / e).max())
                    assert ratio <= 1.0, (shape, name, sign, ratio)
                    worst = max(worst, ratio)
                    if name == "N(0,1)" and sign == 0.0:
                        shares.setdefault((H1, H2), []).append(M.certify_np(z.astype(np.float32), e[:, None]).ravel())
                total += len(g)
    assert total == 2000
    print(f"largest |z32 - z64| / e over 2 000 networks x 8 inputs x 3 displacements: {worst:.4f}")
    for cell, parts in shares.items():
        print(f"  {cell}: the certificate decides {np.concatenate(parts).mean():.4f} of the N(0,1) passes")


def test_certificate_share_on_the_shared_passes():
    """The shares tests/test_gpu_sig2.py compares the device against (printed for DESIGN)."""
    for shape in M.SHAPES:
        s = M.host_share(shape)
        print(f"  {shape}: host-model stage-0 share {s:.4f}")
        assert 0.0 <= s <= 1.0
