"""k_sig2_block (sigmoid networks with two hidden layers of up to 128 units,
[6, 2..128, 2..128, 2..4] with bias, a 256-thread block per game) without a GPU:
the ABI value and the Python names, the scope checks of pg_eval_population and
pg_eval_resolve, and the static f32 error bound under the block layout
(csrc/pg_sig2_bound.h, compiled for the host with gcc) against its numpy
restatement and against an f32 emulation of the block's chain whose every
sigmoid is displaced adversarially by the full allowance
(tests/_sig2_block_model.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _sig2_block_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")
CELLS = [(2, 2), (65, 2), (2, 65), (100, 100), (128, 128)]


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


# ------------------------------------------------------------------- ABI ----
def test_kernel_value_and_names():
    from pong_amd import _lib, device
    text = open(HEADER).read()
    got = int(re.search(r"\bPG_KERNEL_SIG2_BLOCK\s*=\s*(\d+)", text).group(1))
    assert got == 11 == _lib.PG_KERNEL_SIG2_BLOCK == device.BLOCK_KERNELS["sig2_block"]
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    assert _lib.SIGNATURES["pg_sig2_block_decide"] == _lib.SIGNATURES["pg_relu_decide"]  # the same argument struct
    assert re.search(r"\bpg_sig2_block_decide\(const pg_relu_decide_args \*", text)
    assert device.kernel_code("sig2_block") == 11 and device.kernel_name(11) == "sig2_block"
    # KERNELS and MORE_KERNELS are unchanged: the name lives in a third mapping
    plain = ["auto", "general", "split", "wide", "relu", "relu2", "relu_wide", "sig2"]
    assert sorted(device.KERNELS) == sorted(plain + [n + "+advance" for n in ("relu", "relu2", "sig2", "auto")])
    assert device.MORE_KERNELS == {"relu2_block": 10}
    assert device.kernel_code("relu2_block") == 10 and device.kernel_name(10) == "relu2_block"
    for bad in ("sig2_block+advance", "sig2_block+solo", "sig2_block+advance+solo", "sig2_block+"):
        with pytest.raises(KeyError) as err:
            device.kernel_code(bad)
        assert "+solo" in str(err.value) and "+advance" in str(err.value) and "sig2_block" in str(err.value), bad
    assert hasattr(device.Evaluator, "sig2_block_decide")


def _args(_lib, shape, kernel=None, activation=None, bias=True, dtype=None, n_genomes=0, **fields):
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes = 6, n_genomes
    a.kernel = _lib.PG_KERNEL_SIG2_BLOCK if kernel is None else kernel
    a.net = _lib.make_net(shape, bias, _lib.PG_F32 if dtype is None else dtype,
                          activation=_lib.PG_ACT_SIGMOID if activation is None else activation)
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

    for shape in ([6, 2, 2, 2], [6, 65, 2, 2], [6, 64, 64, 3], [6, 128, 128, 4]) + tuple(M.BLOCK_SHAPES):
        for dtype in (K.PG_F32, K.PG_F64):
            assert run(shape, dtype=dtype) == K.PG_OK, shape
            assert lib.pg_eval_resolve(ctypes.byref(_args(K, shape, dtype=dtype))) == 11
    top = [6, 64, 64, 3]
    refused(b"sigmoid", top, activation=K.PG_ACT_RELU)  # activation first: also for a shape out of scope
    refused(b"sigmoid", [6, 64, 3], activation=K.PG_ACT_RELU)
    for shape in ([6, 64, 3], [6, 129, 64, 3], [6, 64, 129, 3], [6, 1, 64, 3], [6, 64, 1, 3], [6, 64, 64, 5],
                  [6, 8, 8, 8, 2]):
        refused(b"sig2_block kernel needs NETWORK_SHAPE [6, 2..128, 2..128, 2..4] with bias", shape)
    refused(b"bias", top, bias=False)
    refused(b"sig2_block kernel is the certified-precision path", top, precision=K.PG_PREC_F64)
    refused(b"horizon", top, horizon=1000)
    buf = (ctypes.c_uint32 * 8)()
    refused(b"hard", top, hard_log=ctypes.cast(buf, ctypes.c_void_p), hard_cap=1)
    # the modifier bits, as on every explicit kernel outside the three certified families: advance first, then solo
    ADV, SOLO = K.PG_KERNEL_ADVANCE, K.PG_KERNEL_SOLO
    refused(b"PG_KERNEL_ADVANCE: kernel=11", top, kernel=11 | ADV)
    refused(b"PG_KERNEL_ADVANCE: kernel=11", top, kernel=11 | ADV | SOLO)
    refused(b"PG_KERNEL_SOLO: kernel=11", top, kernel=11 | SOLO)
    # the workspace: the base size alone
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    for shape in (top, [6, 128, 128, 3]):
        assert lib.pg_eval_workspace_bytes(ctypes.byref(_args(K, shape, n_genomes=4096))) == base
    # PG_KERNEL_AUTO is unchanged: WIDE from 64 units up, else GENERAL
    for shape, want in (([6, 100, 100, 3], K.PG_KERNEL_WIDE), ([6, 128, 128, 3], K.PG_KERNEL_WIDE),
                        ([6, 64, 64, 3], K.PG_KERNEL_WIDE), ([6, 16, 16, 3], K.PG_KERNEL_GENERAL)):
        assert lib.pg_eval_resolve(ctypes.byref(_args(K, shape, kernel=K.PG_KERNEL_AUTO))) == want


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


def _laws(rng, G, n):
    return np.concatenate([rng.random((n, G)), rng.standard_normal((n, G)), rng.standard_normal((n, G)) * 30.0,
                           rng.standard_normal((n, G)) * 1e-38])


def test_block_bound_equals_its_numpy_restatement(tmp_path):
    """The gcc-compiled bound under the block layout against the restatement, to one f32 ulp, on every block shape;
    a network wider than the lane layout holds has no bound there."""
    rng = np.random.default_rng(31)
    for shape in M.BLOCK_SHAPES:
        g = _laws(rng, M.genes(shape), 4)
        e = M.bounds(tmp_path, shape, g)
        assert np.isfinite(e).all() and (e > 0).all()
        assert _ulp_equal(e, M.bound_np(shape, g)).all(), shape
        if max(shape[1:3]) > 64:
            assert np.isinf(M.bounds(tmp_path, shape, g[:2], which="lanes")).all()


def test_lane_layout_is_what_it_was(tmp_path):
    """pg_sig2_bound_genome (the lane layout's earlier entry) and pg_sig2_bound_genome_l under
    pg_sig2_layout_lanes print the same %a strings; they are the restatement's under 9 / 65 / 11 with 2, 36, 80."""
    rng = np.random.default_rng(32)
    for shape in ([6, 2, 2, 2], [6, 17, 33, 4], [6, 64, 2, 2], [6, 64, 64, 3]):
        g = _laws(rng, M.genes(shape), 6)
        old, new = M.bound_strings(tmp_path, "old", shape, g), M.bound_strings(tmp_path, "lanes", shape, g)
        assert old == new and len(old) == len(g)
        e = np.array([float.fromhex(v) for v in new]).astype(np.float32)
        assert _ulp_equal(e, M.bound_np(shape, g, M.LANE_CHAIN, M.LANE_UNDER)).all()
        assert (M.bounds(tmp_path, shape, g) > e).all()  # the block layout's chain is the longer one


def test_bound_is_inf_for_genes_f32_sums_cannot_hold(tmp_path):
    """A NaN gene, an inf gene and a gene of 1e30 in any of the six blocks: e = inf, in C and in the restatement."""
    rng = np.random.default_rng(33)
    for shape in ([6, 2, 2, 2], [6, 65, 64, 4], [6, 128, 128, 3]):
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
    below it (tests/test_sig2_host.py's, with the block layout's chain lengths)."""
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
        w3[:, H2] = target / M.CHAIN[2] * np.sign(w3[:, H2])
    else:
        w3[:, H2] = 0.0
        w3[:, :H2] *= target / M.sums(shape, M.pack(w1, w2, w3))[0].max()
    return M.pack(w1, w2, w3)


def test_bound_at_the_cap(tmp_path):
    """Each capped sum just above PG_SIG2_CAP: inf.  Just below: finite, the
    emulated z32 finite and within the bound of numpy's chain."""
    rng = np.random.default_rng(34)
    for H1, H2 in CELLS:
        shape = [6, H1, H2, 3]
        base = rng.standard_normal(M.genes(shape)) * 0.1
        for which in ("A", "B", "S_bias", "S_w3"):
            above, below = (_scaled(shape, base, which, M.CAP * f) for f in (1 + 1e-3, 1 - 1e-3))
            assert np.isfinite(above.astype(np.float32)).all()
            e = M.bounds(tmp_path, shape, np.array([above, below]))
            assert np.isinf(e[0]) and np.isfinite(e[1]), (shape, which, e)
            assert _ulp_equal(e, M.bound_np(shape, np.array([above, below]))).all()
            k = np.concatenate([np.zeros((1, 6), np.int64), np.full((1, 6), 320), rng.integers(0, 321, size=(2, 6))])[None]
            z = M.z32(shape, below[None], k)
            assert np.isfinite(z).all()
            err = np.abs(z.astype(np.float64) - M.z64(shape, below[None], k)).max()
            assert err <= e[1], (shape, which, err, e[1])


# ------------------------------------------------------------- soundness ----
def _families(rng, shape, q):
    """q networks in each of five families: U[0,1), N(0,1), N(0,3), N(0,30), all-positive systematic."""
    G = M.genes(shape)
    sysnet = (0.05 + 0.9 * ((np.arange(G)[None, :] * 7 + np.arange(q)[:, None] * 13) % 31) / 31.0)
    return {"U[0,1)": rng.random((q, G)), "N(0,1)": rng.standard_normal((q, G)),
            "N(0,3)": rng.standard_normal((q, G)) * 3.0, "N(0,30)": rng.standard_normal((q, G)) * 30.0,
            "positive": sysnet}


def test_bound_covers_the_adversarial_f32_chain(tmp_path):
    """Per shape 5 families x 16 networks x 8 inputs: with every emulated f32
    sigmoid displaced by the full 4.5 u towards, then away from, one output,
    that output's emulated z32 stays within e of numpy's own np.dot chain: the
    bound's claim, so the threshold is 1.  Prints the largest ratio."""
    rng = np.random.default_rng(35)
    worst = 0.0
    for H1, H2 in CELLS:
        O = 2 + (H1 + H2) % 3
        shape = [6, H1, H2, O]
        for name, g in _families(rng, shape, 16).items():
            e = M.bounds(tmp_path, shape, g)
            assert np.isfinite(e).all() and (e > 0).all()
            k = rng.integers(0, 321, size=(len(g), 8, 6))
            k[:, 0] = 320  # the largest inputs: nothing of the all-positive networks cancels
            ref = M.z64(shape, g, k)
            out = int(rng.integers(0, O))
            for sign in (1.0, -1.0, 0.0):
                z = M.z32(shape, g, k, out=out, sign=sign).astype(np.float64)
                err = np.abs(z - ref)[:, :, out] if sign else np.abs(z - ref).max(axis=2)
                ratio = float((err.max(axis=1) / e).max())
                assert ratio <= 1.0, (shape, name, sign, ratio)
                worst = max(worst, ratio)
    print(f"largest |z32 - z64| / e over 5 shapes x 80 networks x 8 inputs x 3 displacements: {worst:.4f}")


def test_tiny_genes_stay_within_the_bound(tmp_path):
    """Signed genes of magnitude 1e-36 .. 1e-60 (subnormal in f32, or flushed to zero): the emulated chain stays
    within e of numpy's -- the underflow term, which is all of e here."""
    rng = np.random.default_rng(36)
    for H1, H2 in CELLS:
        shape = [6, H1, H2, 3]
        G = M.genes(shape)
        g = np.where(rng.random((6, G)) < 0.5, -1.0, 1.0) * 10.0 ** -rng.uniform(36.0, 60.0, (6, G))
        e = M.bounds(tmp_path, shape, g)
        assert np.isfinite(e).all() and (e > 0).all() and (e < 1e-34).all()
        k = rng.integers(0, 321, size=(6, 8, 6))
        err = np.abs(M.z32(shape, g, k).astype(np.float64) - M.z64(shape, g, k)).max(axis=(1, 2))
        assert (err <= e).all(), (shape, (err / e).max())


def test_certificate_share_on_the_shared_passes():
    """The shares tests/test_gpu_sig2_block.py compares the device against (printed for DESIGN)."""
    for shape in ([6, 65, 2, 2], [6, 100, 100, 3], [6, 128, 128, 3]):
        s = M.host_share(shape)
        print(f"  {shape}: host-model stage-0 share {s:.4f}")
        assert 0.0 <= s <= 1.0
