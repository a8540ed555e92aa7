"""ReLU policy networks (ABI 13, activation_function = ReLU numpy_nn.py:6-9, 26)
without a GPU: the ABI values, the validation and kernel resolution of
pg_eval_population, k_relu's static f32 error bound (csrc/pg_relu_bound.h,
compiled for the host with gcc) against an f32 emulation of the kernel's chain,
the drop-in numpy_nn's activation switch and the checkpoint configuration."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pong_ga.h")
BOUND_HDR = os.path.join(REPO, "neuro-genetic-pong-self-play_amd", "csrc", "pg_relu_bound.h")
U32 = 2.0 ** -24


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
def _relu_lanes(H):
    return 4 if H <= 64 else (8 if H <= 128 else 16)


def _bounds(tmp_path, nets):
    """pg_relu_bound_genome of each (H, O, genes) through a stand-alone gcc program."""
    src = tmp_path / "b.c"
    src.write_text(f'#include <stdio.h>\n#include <stdlib.h>\n#include "{BOUND_HDR}"\n'
                   "int main(int argc, char **argv){ FILE *f = fopen(argv[1], \"rb\"); int hdr[3];\n"
                   " while (fread(hdr, sizeof(int), 3, f) == 3) { int H = hdr[0], O = hdr[1];\n"
                   "  size_t G = (size_t)H * 7 + (size_t)O * (H + 1); double *g = malloc(G * sizeof(double));\n"
                   "  if (fread(g, sizeof(double), G, f) != G) return 1;\n"
                   "  printf(\"%a\\n\", (double)pg_relu_bound_genome(g, H, O, hdr[2])); free(g); }\n"
                   " return 0; }\n")
    exe = tmp_path / "b"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    data = tmp_path / "nets.bin"
    with open(data, "wb") as fh:
        for H, O, g in nets:
            fh.write(np.array([H, O, _relu_lanes(H) * 16], np.int32).tobytes())
            fh.write(np.ascontiguousarray(g, np.float64).tobytes())
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(v) for v in out])


def _fma32(a, b, c):
    """fl32(a * b + c): the product of two f32 is exact in f64, the sum is rounded to f64, then to f32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _z32(H, O, g, k):
    """k_relu's f32 chain (pg_relu.hpp relu_z32) on doubled centroids k [m, 6]:
    unit j = hl + LN u on lane hl, 16 units per lane in order, a pairwise tree
    over the lanes (group_sum), then the output bias."""
    LN, U = _relu_lanes(H), 16
    w1 = g[: H * 7].reshape(H, 7).astype(np.float32)
    w2 = g[H * 7:].reshape(O, H + 1).astype(np.float32)
    x = k.astype(np.float32) * np.float32(0.003125)  # feat32
    a = np.broadcast_to(w1[:, 6], (len(k), H)).copy()
    for i in range(6):
        a = _fma32(w1[None, :, i], x[:, i:i + 1], a)
    h = np.zeros((len(k), LN * U), np.float32)
    h[:, :H] = np.maximum(a, np.float32(0))
    w2p = np.zeros((O, LN * U), np.float32)
    w2p[:, :H] = w2[:, :H]
    h, w2p = h.reshape(len(k), U, LN), w2p.reshape(O, U, LN)
    z = np.empty((len(k), O), np.float32)
    for o in range(O):
        acc = np.zeros((len(k), LN), np.float32)
        for u in range(U):
            acc = _fma32(w2p[o, u][None, :], h[:, u, :], acc)
        while acc.shape[1] > 1:
            acc = acc[:, 0::2] + acc[:, 1::2]
        z[:, o] = acc[:, 0] + w2[o, H]
    return z


def _z64(H, O, g, k):
    """numpy_nn's f64 pre-activations (NeuralNetwork.run numpy_nn.py:126-131 with ReLU)."""
    w1, w2 = g[: H * 7].reshape(H, 7), g[H * 7:].reshape(O, H + 1)
    z = np.empty((len(k), O))
    for t in range(len(k)):
        a0 = np.ones(7)
        a0[:6] = (k[t] / 2) / 160
        a1 = np.ones(H + 1)
        a1[:-1] = np.maximum(0.0, np.dot(w1, a0))
        z[t] = np.dot(w2, a1)
    return z


def _s_max(H, O, g):
    w1, w2 = np.abs(g[: H * 7].reshape(H, 7)), np.abs(g[H * 7:].reshape(O, H + 1))
    return float((w2[:, :H] @ w1.sum(axis=1) + w2[:, H]).max())


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
