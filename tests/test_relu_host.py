"""ReLU policy networks (ABI 13, activation_function = ReLU numpy_nn.py:6-9, 26)
without a GPU: the ABI values, the validation and kernel resolution of
pg_eval_population, k_relu's static f32 error bound (csrc/pg_relu_bound.h,
compiled for the host with gcc) against an f32 emulation of the kernel's chain
(tests/_relu_model.py: its once-rounded fma, the networks built to use up the
bound, the tie networks the GPU tests decide by np.dot's last bit),
the drop-in numpy_nn's activation switch and the checkpoint configuration."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from _relu_model import (RELU_CAP, TIE_CELLS, U32, _bounds, _fma32, _fma32_twice, _s_max, _z32, _z64, cap_net,
                         systematic_net, tie_case, tie_sensitivity, tiny_net)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")


@pytest.fixture(scope="module")
def lib():
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib.lib()


# ------------------------------------------------------------------- ABI ----
def test_activation_values_match_header():
    from pong_amd import _lib
    text = open(HEADER).read()
    for name, want in (("PG_ACT_SIGMOID", 0), ("PG_ACT_RELU", 1), ("PG_KERNEL_RELU", 6)):
        got = int(re.search(rf"\b{name}\s*=\s*(\d+)", text).group(1))
        assert got == want == getattr(_lib, name)
    assert int(re.search(r"#define PG_ABI_VERSION (\d+)", text).group(1)) == _lib.PG_ABI_VERSION == 13
    assert _lib.make_net([6, 64, 3]).activation == _lib.PG_ACT_SIGMOID  # the default is what a zeroed net means
    net = _lib.make_net([6, 64, 3], True, _lib.PG_F32, activation=_lib.PG_ACT_RELU)
    assert (net.activation, net.dtype, net.bias) == (_lib.PG_ACT_RELU, _lib.PG_F32, 1)
    assert _lib.PgNet.activation.offset == _lib.PgNet.dtype.offset + 4
    assert "pg_relu_decide" in _lib.SIGNATURES


def test_gene_count_ignores_the_activation(lib):
    from pong_amd import _lib
    for shape in ([6, 2, 2], [6, 64, 3], [6, 64, 64, 2]):
        counts = [lib.pg_gene_count(ctypes.byref(_lib.make_net(shape, activation=a)))
                  for a in (_lib.PG_ACT_SIGMOID, _lib.PG_ACT_RELU)]
        assert counts[0] == counts[1] > 0


def test_eval_accepts_relu_and_rejects_other_activations(lib):
    from pong_amd import _lib
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes = 6, 0
    a.net = _lib.make_net([6, 64, 3], activation=_lib.PG_ACT_RELU)
    assert lib.pg_eval_population(ctypes.byref(a), None) == _lib.PG_OK
    a.net.activation = 2
    assert lib.pg_eval_population(ctypes.byref(a), None) == _lib.PG_ERR_INVALID
    assert b"activation" in lib.pg_last_error()
    assert lib.pg_gene_count(ctypes.byref(a.net)) == _lib.PG_ERR_INVALID


def test_workspace_bytes_of_relu_calls(lib):
    """AUTO with a ReLU net: k_relu for [6, H<=256, 2..4] certified with bias,
    else the general kernel; both need only the base workspace (k_relu keeps
    no lane records), never the split kernel's records or the wide kernel's copies."""
    from pong_amd import _lib
    a = _lib.PgEvalArgs()
    a.n_games, a.n_genomes = 6, 4096
    base = 256 + (4096 * 6 * 4 + 255) // 256 * 256
    a.net = _lib.make_net([6, 64, 3])
    split = lib.pg_eval_workspace_bytes(ctypes.byref(a))
    assert split > base  # the sigmoid net: the split kernel's records
    for kernel in (_lib.PG_KERNEL_AUTO, _lib.PG_KERNEL_RELU, _lib.PG_KERNEL_GENERAL):
        a.kernel = kernel
        a.net = _lib.make_net([6, 64, 3], activation=_lib.PG_ACT_RELU)
        assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) == base
    a.kernel = _lib.PG_KERNEL_AUTO
    a.net = _lib.make_net([6, 512, 512, 3], True, _lib.PG_F32, activation=_lib.PG_ACT_RELU)
    assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) == base
    a.net.activation = _lib.PG_ACT_SIGMOID
    assert lib.pg_eval_workspace_bytes(ctypes.byref(a)) > base  # the same sigmoid net: k_wide's copies


# ----------------------------------------------------------------- bound ----
def test_bound_covers_the_f32_chain(tmp_path):
    """2 000 random networks: the emulated f32 outputs lie within the bound of
    numpy's f64 np.dot chain, and the bound is a small multiple of u max_o S_o."""
    rng = np.random.default_rng(13)
    nets = []
    for t in range(2000):
        H = (2, 16, 64, 256)[t % 4]
        O = int(rng.integers(2, 5))
        G = H * 7 + O * (H + 1)
        dist = (t // 4) % 3
        g = rng.random(G) if dist == 0 else rng.standard_normal(G) * (1.0 if dist == 1 else 30.0)
        nets.append((H, O, g))
    e = _bounds(tmp_path, nets)
    assert e.shape == (2000,) and np.isfinite(e).all() and (e > 0).all()
    worst = 0.0
    for (H, O, g), bound in zip(nets, e):
        k = rng.integers(0, 321, size=(8, 6))
        err = np.abs(_z32(H, O, g, k).astype(np.float64) - _z64(H, O, g, k)).max()
        s = _s_max(H, O, g)
        assert err <= bound, (H, O, err, bound)
        assert bound <= 64 * U32 * s, (H, O, bound, s)
        worst = max(worst, err / (U32 * s))
    print(f"largest |z32 - z64| / (u max S_o) over 16 000 passes: {worst:.3f} (the bound: 33)")


def test_bound_is_inf_for_weights_f32_cannot_hold(tmp_path):
    rng = np.random.default_rng(14)
    nets = []
    for H, O in ((2, 2), (64, 3), (256, 4)):
        G = H * 7 + O * (H + 1)
        for pos in (0, H * 7 - 1, H * 7, G - 1):  # a W1 weight, a hidden bias, a W2 weight, an output bias
            g = rng.standard_normal(G)
            g[pos] = 1e30
            nets.append((H, O, g))
        for bad in (np.inf, np.nan):
            g = rng.standard_normal(G)
            g[3] = bad
            nets.append((H, O, g))
        nets.append((H, O, rng.standard_normal(G)))
    e = _bounds(tmp_path, nets)
    for (H, O, g), bound in zip(nets, e):
        assert np.isinf(bound) == (not np.isfinite(g).all() or np.abs(g).max() >= 1e30)


# ------------------------------------------------- the model's exact fma ----
def _midpoint_cases(rng, n):
    """a * b an odd 25-bit integer (exact in f64, half-way between the two f32
    neighbours p - 1 and p + 1) plus a c far below f64's last bit of it: the
    f64 sum rounds to p itself, and the second rounding to f32 then goes to the
    even neighbour whatever the sign of c."""
    a = (rng.integers(1 << 11, 1 << 12, n) | 1).astype(np.float32)
    b = (rng.integers(1 << 12, 1 << 13, n) | 1).astype(np.float32)
    keep = a.astype(np.int64) * b.astype(np.int64) >= 1 << 24
    a, b = a[keep], b[keep]
    c = (np.where(rng.random(len(a)) < 0.5, -1.0, 1.0) * 2.0 ** -rng.integers(40, 100, len(a))).astype(np.float32)
    want = (a.astype(np.int64) * b.astype(np.int64) + np.sign(c).astype(np.int64)).astype(np.float32)
    return a, b, c, want


def test_model_fma_is_rounded_once(tmp_path):
    rng = np.random.default_rng(21)
    a, b, c, want = _midpoint_cases(rng, 4000)
    assert len(a) > 1000
    np.testing.assert_array_equal(_fma32(a, b, c), want)
    wrong = _fma32_twice(a, b, c) != want
    assert 0.25 < wrong.mean() < 0.75, wrong.mean()  # the twice-rounded formula: wrong whenever c points away from even
    # the same, scaled into f32's subnormals (the last rounding is coarser there, not finer)
    tiny = np.float32(2.0 ** -140)
    sub = _fma32(a * np.float32(2.0 ** -12), b * tiny, np.float32(2.0 ** -149))
    np.testing.assert_array_equal(sub, ((a.astype(np.float64) * b.astype(np.float64) * 2.0 ** -152 + 2.0 ** -149)
                                        .astype(np.float32)))  # (that f64 sum is exact: < 53 bits)
    # against the C library's fmaf on the hard cases and on random operands of every scale, inf and NaN included
    ra = (rng.standard_normal(20000) * 2.0 ** rng.integers(-60, 60, 20000)).astype(np.float32)
    rb = (rng.standard_normal(20000) * 2.0 ** rng.integers(-60, 60, 20000)).astype(np.float32)
    rc = np.where(rng.random(20000) < 0.5, -(ra.astype(np.float64) * rb.astype(np.float64)) * (1 + 2.0 ** -rng.integers(1, 40, 20000)),
                  rng.standard_normal(20000) * 2.0 ** rng.integers(-120, 120, 20000)).astype(np.float32)
    ra[:4], rb[:4], rc[:4] = [np.inf, np.inf, np.nan, 0.0], [1.0, 0.0, 1.0, -1.0], [-np.inf, 1.0, 1.0, 0.0]
    A, B, C = (np.concatenate(v) for v in ((a, ra), (b, rb), (c, rc)))
    src = tmp_path / "f.c"
    src.write_text("#include <math.h>\n#include <stdio.h>\n"
                   "int main(int argc, char **argv){ FILE *f = fopen(argv[1], \"rb\"), *o = fopen(argv[2], \"wb\"); float v[3];\n"
                   " while (fread(v, sizeof(float), 3, f) == 3) { volatile float r = fmaf(v[0], v[1], v[2]);\n"
                   "  float w = r; fwrite(&w, sizeof(float), 1, o); }\n fclose(o); return 0; }\n")
    exe = tmp_path / "f"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    np.stack([A, B, C], axis=1).astype(np.float32).tofile(tmp_path / "in.bin")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    ref = np.fromfile(tmp_path / "out.bin", np.float32)
    got = _fma32(A, B, C)
    assert len(ref) == len(got)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.int32), ref[~nan].view(np.int32))
    assert (_fma32_twice(A, B, C)[~nan] != ref[~nan]).any()


# ------------------------------------ the bound on adversarial networks ----
BOUND_H = (1, 64, 65, 128, 129, 256)


def _family_nets():
    """(family, H, O, genes) of the networks built to use up the bound."""
    rng = np.random.default_rng(31)
    for H in BOUND_H:
        for O in (2, 3, 4):
            yield "systematic", H, O, systematic_net(H, O)
            yield "cap", H, O, cap_net(H, O, RELU_CAP * (1 - 1e-3))
            yield "tiny", H, O, tiny_net(H, O, rng)


def test_bound_covers_the_chain_on_adversarial_networks(tmp_path):
    """The exact-fma model on networks whose roundings all point one way
    (systematic_net), that sit just below PG_RELU_CAP, and whose genes are f32
    subnormals or flush to zero: |z32 - z64| <= bound on all-0, all-320 and
    random inputs, and z32 is finite whenever the bound is.  The printed ratio
    err / (u max_o S_o) is the slack the derivation's 33 leaves (a measurement,
    not a condition)."""
    rng = np.random.default_rng(32)
    fam = list(_family_nets())
    e = _bounds(tmp_path, [(H, O, g) for _, H, O, g in fam])
    assert np.isfinite(e).all() and (e > 0).all()
    worst = {}
    for (name, H, O, g), bound in zip(fam, e):
        k = np.concatenate([np.zeros((1, 6), np.int64), np.full((1, 6), 320), rng.integers(0, 321, size=(14, 6))])
        z32, z64 = _z32(H, O, g, k), _z64(H, O, g, k)
        assert np.isfinite(z32).all(), (name, H, O)
        err = np.abs(z32.astype(np.float64) - z64).max()
        assert err <= bound, (name, H, O, err, bound)
        s = _s_max(H, O, g)
        if name == "cap":
            assert RELU_CAP * (1 - 2e-3) < s < RELU_CAP
        else:
            assert (g > 0).all() if name == "systematic" else s < 1e-30
        w = worst.setdefault(name, [0.0, 0.0])
        w[0], w[1] = max(w[0], err / (U32 * s)), max(w[1], err / bound)
    assert set(worst) == {"systematic", "cap", "tiny"}
    for name, w in worst.items():  # (tiny_net's bound is its underflow term: u max S_o says nothing there)
        print(f"largest |z32 - z64| / (u max S_o), {name}_net: {w[0]:.3f} (the bound: 33); / bound: {w[1]:.4f}")


def test_bound_is_inf_just_above_the_cap(tmp_path):
    nets = [(H, O, cap_net(H, O, RELU_CAP * (1 + d))) for H in BOUND_H for O in (2, 3, 4) for d in (1e-3, -1e-3)]
    e = _bounds(tmp_path, nets)
    for (H, O, g), bound in zip(nets, e):
        assert np.isfinite(g.astype(np.float32)).all()
        assert np.isinf(bound) == (_s_max(H, O, g) > RELU_CAP), (H, O, bound)
    assert np.isinf(e[0::2]).all() and np.isfinite(e[1::2]).all()


# ------------------------------------------------------- the tie networks ----
@pytest.mark.parametrize("H,O", TIE_CELLS)
def test_tie_net_is_sensitive_to_the_summation_order(H, O):
    """numpy's own np.dot on the tie network of each cell the GPU test uses: the
    exactly equal outputs come out bitwise different in at least 8 of 256
    passes and np.argmax is non-zero at least once -- an f64 fallback that sums
    in another order than np.dot cannot reproduce these decisions by luck."""
    g, k = tie_case(H, O)
    w1, w2 = g[: H * 7].reshape(H, 7), g[H * 7:].reshape(O, H + 1)
    assert (w1[1::2] == w1[0:2 * (H // 2):2]).all() and (w2 >= 0).all() and (w2[:, H] > 0).all()
    assert all((np.sort(w2[o]) == np.sort(w2[0])).all() and (w2[o] != w2[0]).any() for o in range(1, O))
    assert (g.astype(np.float32) == g).all()
    differ, nonzero = tie_sensitivity(H, O, g, k)
    assert differ >= 8 and nonzero >= 1, (differ, nonzero)


# --------------------------------------------------------------- drop-in ----
def test_numpy_nn_resolves_the_activation_at_call_time(monkeypatch):
    import config
    import numpy_nn
    assert config.ACTIVATION == "sigmoid"
    assert numpy_nn.activation_function is numpy_nn._ACTIVATIONS[config.ACTIVATION] is numpy_nn.sigmoid
    assert numpy_nn.activation() == "sigmoid"
    np.testing.assert_array_equal(numpy_nn.ReLU([-1.5, -0.0, 0.25]), [0.0, 0.0, 0.25])
    monkeypatch.setattr(numpy_nn, "activation_function", numpy_nn.ReLU)  # the reference's one-line switch
    assert numpy_nn.activation() == "relu"
    monkeypatch.setattr(numpy_nn, "activation_function", np.tanh)
    with pytest.raises(NotImplementedError, match="sigmoid.*ReLU"):
        numpy_nn.activation()


def test_runtime_evaluator_keys_on_the_activation():
    from pong_amd import runtime
    sig = inspect.signature(runtime.evaluator)
    assert sig.parameters["activation"].default == "sigmoid"


class _StandInGA:
    """What checkpoint._config reads of a DeviceGA."""
    nodes, P, H, tournsize, bias, n_games, schedule = [6, 16, 3], 8, 2, 2, True, 6, "selfplay"
    cxpb = mutpb = alpha = sigma = indpb = 0.9
    mu, seed, physics_seed, precision, kernel, hof_block_rows = 0.0, 1, 0, "certified", "auto", 0

    def __init__(self, activation=None):
        import torch
        self.dtype = torch.float64
        if activation is not None:
            self.activation = activation


def test_checkpoint_config_names_the_activation_only_when_set(tmp_path, monkeypatch):
    import torch

    from pong_amd import checkpoint, evolve
    assert "activation" not in checkpoint._config(_StandInGA())           # a GA from before this field
    assert "activation" not in checkpoint._config(_StandInGA("sigmoid"))  # the default: the config is unchanged
    assert checkpoint._config(_StandInGA("relu"))["activation"] == "relu"
    assert inspect.signature(evolve.DeviceGA.__init__).parameters["activation"].default == "sigmoid"

    made = []

    class FakeGA:
        def __init__(self, nodes, P, **kw):
            made.append(kw)

        def set_population(self, *a):
            pass

        def set_hall_of_fame(self, *a):
            pass

    monkeypatch.setattr(evolve, "DeviceGA", FakeGA)
    tensors = {"population": torch.zeros((8, 4), dtype=torch.float64), "fitness": torch.zeros(8, dtype=torch.float64),
               "valid": torch.zeros(8, dtype=torch.uint8), "hall_of_fame": torch.zeros((2, 4), dtype=torch.float64),
               "hof_fitness": torch.zeros(2, dtype=torch.float64)}
    for act in (None, "relu"):
        cfg = checkpoint._config(_StandInGA(act))
        path = str(tmp_path / f"c_{act}.safetensors")
        checkpoint.write_tensors(path, tensors, {"format": checkpoint.FORMAT, "config": json.dumps(cfg),
                                                 "generation": 3, "logbook": "[]"})
        checkpoint.load(path)
    assert "activation" not in made[0]  # an old (sigmoid) checkpoint: DeviceGA's default applies
    assert made[1]["activation"] == "relu"
