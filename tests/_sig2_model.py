"""The host model of k_sig2's decision (csrc/pg_hidden2.hpp, pg_sig2_bound.h) in
plain numpy, shared by tests/test_sig2_host.py and tests/test_gpu_sig2.py: the
f32 chain of a [6, H1, H2, O] sigmoid network on tests/_relu_model.py's
once-rounded fused multiply-add with an emulated f32 sigmoid, numpy_nn's f64
chain, the bound restated in numpy and compiled with gcc, certify's rule
(pg_cascade.hpp) restated, and the passes both test files draw.  Everything is
vectorised over a leading axis of networks."""
import os
import subprocess

import numpy as np

from _relu_model import _fma32
from _relu2_model import SHAPES, genes, lanes, pack, split  # noqa: F401  (the layout is k_relu2's)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_HDR = os.path.join(REPO, "neuro-genetic-pong-self-play_amd", "csrc", "pg_sig2_bound.h")
U32 = 2.0 ** -24
ETA = 2.0 ** -126
CAP = 1e25                            # PG_SIG2_CAP
CHAIN1, CHAIN2, CHAIN3 = 9, 65, 11    # PG_SIG2_CHAIN1..3
SIG = 4.5                             # PG_SIG2_SIG: sigmoid_f32's own absolute error, in u
SLOPE = 0.25                          # PG_SIG2_SLOPE


def sums(shape, g):
    """The sums of pg_sig2_bound.h for genomes g [.., G]: S_o (with the output
    bias's share), T_o, sum_k |W3_ok| per output; sum_j A_j, sum_k B_k, sum_k P_k."""
    _, H1, H2, O = shape
    w1, w2, w3 = (np.abs(w) for w in split(shape, np.asarray(g, np.float64)))
    with np.errstate(all="ignore"):
        A = w1.sum(axis=-1)
        W = w2[..., :H1].sum(axis=-1)
        P = np.einsum("...kj,...j->...k", w2[..., :H1], A)
        B = W + w2[..., H1]
        Q = (SLOPE * CHAIN1) * P + (SIG + CHAIN2) * B
        t = SLOPE * Q + (SIG + CHAIN3)
        S = np.einsum("...ok,...k->...o", w3[..., :H2], t) + CHAIN3 * w3[..., H2]
        T = np.einsum("...ok,...k->...o", w3[..., :H2], W)
        return S, T, w3[..., :H2].sum(axis=-1), A.sum(axis=-1), B.sum(axis=-1), P.sum(axis=-1)


def bound_np(shape, g):
    """pg_sig2_bound_genome restated: e = (u max_o S_o + eta (2 max_o T_o + 36 max_o sum_k |W3_ok| + 80)) (1 + 2^-10)
    as f32, inf when a sum exceeds the cap or is not a number."""
    S, T, W3, a, b, p = sums(shape, g)
    with np.errstate(all="ignore"):
        ok = (a <= CAP) & (b <= CAP) & (p <= CAP) & (S <= CAP).all(axis=-1) & (T <= CAP).all(axis=-1) & \
            (W3 <= CAP).all(axis=-1)
        e = (U32 * S.max(axis=-1) + ETA * (2.0 * T.max(axis=-1) + 36.0 * W3.max(axis=-1) + 80.0)) * (1.0 + 2.0 ** -10)
        return np.where(ok, e, np.inf).astype(np.float32)


def bounds(tmp_path, shape, nets):
    """pg_sig2_bound_genome of each genome of nets [N, G] through a stand-alone gcc program."""
    exe = tmp_path / "bs2"
    if not exe.exists():
        src = tmp_path / "bs2.c"
        src.write_text(f'#include <stdio.h>\n#include <stdlib.h>\n#include "{BOUND_HDR}"\n'
                       "int main(int argc, char **argv){ FILE *f = fopen(argv[1], \"rb\"); int hdr[4];\n"
                       " if (PG_SIG2_CHAIN1 != 9 || PG_SIG2_CHAIN2 != 65 || PG_SIG2_CHAIN3 != 11 || PG_SIG2_SIG != 4.5 ||\n"
                       "     PG_SIG2_SLOPE != 0.25 || PG_SIG2_CAP != 1e25 || PG_SIG2_MAX_H != 64) return 2;\n"
                       " while (fread(hdr, sizeof(int), 4, f) == 4) { int H1 = hdr[0], H2 = hdr[1], O = hdr[2];\n"
                       "  size_t G = (size_t)hdr[3]; double *g = malloc(G * sizeof(double));\n"
                       "  if (fread(g, sizeof(double), G, f) != G) return 1;\n"
                       "  printf(\"%a\\n\", (double)pg_sig2_bound_genome(g, H1, H2, O)); free(g); }\n"
                       " return 0; }\n")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    data = tmp_path / "nets_s2.bin"
    nets = np.atleast_2d(np.ascontiguousarray(nets, np.float64))
    assert nets.shape[1] == genes(shape)
    with open(data, "wb") as fh:
        for g in nets:
            fh.write(np.array([shape[1], shape[2], shape[3], len(g)], np.int32).tobytes())
            fh.write(g.tobytes())
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(v) for v in out]).astype(np.float32)


def sigmoid64(z):
    """numpy_nn.sigmoid (numpy_nn.py:22-23)."""
    with np.errstate(all="ignore"):
        return 1 / (1 + np.e ** -np.asarray(z, np.float64))


def _sig32(a, d):
    """The emulated f32 sigmoid: the f64 sigmoid of the f32 pre-activation
    rounded to f32, then displaced by d (in u; per unit) and rounded again."""
    s = sigmoid64(a.astype(np.float64)).astype(np.float32)
    return (s.astype(np.float64) + d * U32).astype(np.float32)


def z32(shape, g, k, out=None, sign=0.0):
    """k_sig2's f32 chain (pg_hidden2.hpp hidden2_z32) for genomes g [N, G] on doubled
    centroids k [N, m, 6] -> [N, m, O]: layer 1 as six fmas onto the bias; layer
    2 one fma per padded layer-1 unit, in order, onto the bias; layer 3 a lane's
    units hl U + v in order from 0, a pairwise tree over the lanes (group_sum),
    then the output bias.  Padding units have activation 0.5 and zero outgoing
    weights.  sign = 0: every sigmoid as the rounded f64 one.  sign = +-1: every
    sigmoid displaced by the full allowance of 4.5 u towards (+1) or away from
    (-1) raising output `out`: a layer-2 unit by the sign of its weight into
    that output, a layer-1 unit by the sign of sum_k W3[out, k] W2[k, j]."""
    _, H1, H2, O = shape
    LN, U = lanes(H1, H2)
    P = LN * U
    with np.errstate(all="ignore"):
        w1, w2, w3 = (w.astype(np.float32) for w in split(shape, g))
        N, m = k.shape[0], k.shape[1]
        d1, d2 = np.zeros((N, 1, H1)), np.zeros((N, 1, H2))
        if sign:
            d2 = sign * SIG * np.sign(w3[:, out, :H2].astype(np.float64))[:, None, :]
            d1 = sign * SIG * np.sign(np.einsum("nk,nkj->nj", w3[:, out, :H2].astype(np.float64),
                                                w2[:, :, :H1].astype(np.float64)))[:, None, :]
        x = k.astype(np.float32) * np.float32(0.003125)  # feat32
        a = np.broadcast_to(w1[:, None, :, 6], (N, m, H1)).copy()
        for i in range(6):
            a = _fma32(w1[:, None, :, i], x[:, :, i:i + 1], a)
        h1 = np.full((N, m, P), 0.5, np.float32)
        h1[:, :, :H1] = _sig32(a, d1)
        w2p = np.zeros((N, P, P), np.float32)
        w2p[:, :H2, :H1] = w2[:, :, :H1]
        a2 = np.zeros((N, m, P), np.float32)
        a2[:, :, :H2] = w2[:, None, :, H1]
        for j in range(P):
            a2 = _fma32(w2p[:, None, :, j], h1[:, :, j:j + 1], a2)
        h2 = np.full((N, m, P), 0.5, np.float32)
        h2[:, :, :H2] = _sig32(a2[:, :, :H2], d2)
        h2 = h2.reshape(N, m, LN, U)
        w3p = np.zeros((N, O, P), np.float32)
        w3p[:, :, :H2] = w3[:, :, :H2]
        w3p = w3p.reshape(N, O, LN, U)
        z = np.empty((N, m, O), np.float32)
        for o in range(O):
            acc = np.zeros((N, m, LN), np.float32)
            for v in range(U):
                acc = _fma32(w3p[:, None, o, :, v], h2[:, :, :, v], acc)
            while acc.shape[2] > 1:
                acc = acc[:, :, 0::2] + acc[:, :, 1::2]
            z[:, :, o] = acc[:, :, 0] + w3[:, None, o, H2]
    return z


def z64(shape, g, k):
    """numpy_nn's f64 output pre-activations (NeuralNetwork.run numpy_nn.py:126-131 with the sigmoid), np.dot per pass."""
    _, H1, H2, O = shape
    w1, w2, w3 = split(shape, np.asarray(g, np.float64))
    N, m = k.shape[0], k.shape[1]
    z = np.empty((N, m, O))
    with np.errstate(all="ignore"):
        for n in range(N):
            for t in range(m):
                a0 = np.ones(7)
                a0[:6] = (k[n, t] / 2) / 160
                a1 = np.ones(H1 + 1)
                a1[:-1] = sigmoid64(np.dot(w1[n], a0))
                a2 = np.ones(H2 + 1)
                a2[:-1] = sigmoid64(np.dot(w2[n], a1))
                z[n, t] = np.dot(w3[n], a2)
    return z


def run64(shape, g, k):
    """np.argmax of NeuralNetwork.run's output activations for genome g on doubled centroids k [m, 6]."""
    return np.argmax(sigmoid64(z64(shape, np.asarray(g)[None], np.asarray(k)[None])[0]), axis=-1)


def certify_np(z, e):
    """certify (pg_cascade.hpp) restated in f32 numpy: True where the rule decides.  z [.., O] f32, e [..] f32."""
    f = np.float32
    z = np.asarray(z, f)
    e = np.asarray(e, f)
    O = z.shape[-1]
    with np.errstate(all="ignore"):
        tlo, thi = f(36.7367) - e, f(36.7369) + e
        sat = z[..., O - 1] > thi
        for o in range(O - 2, -1, -1):
            sat = np.where(z[..., o] > thi, True, np.where(z[..., o] >= tlo, False, sat))
        top = -np.sort(-z, axis=-1)
        top1, top2 = top[..., 0], top[..., 1]
        tw = f(8.8817842e-16) * (np.exp((top1 + e).astype(f)).astype(f) + f(1.0))
        uns = (top1 - top2 > f(2.0) * e + tw) & (top1 > f(-708.0) + e)
        return np.where(top1 >= tlo, sat, uns) & np.isfinite(e)


def n01_passes(shape, dtype_f32=False):
    """The N(0, 1) networks and inputs on which the host and the GPU test compare
    the certificate's share: 32 genomes [32, G], doubled centroids [32, 64, 6]."""
    rng = np.random.default_rng([11] + list(shape))
    g = rng.standard_normal((32, genes(shape)))
    if dtype_f32:
        g = g.astype(np.float32).astype(np.float64)
    return g, rng.integers(0, 321, size=(32, 64, 6))


def host_share(shape, dtype_f32=False):
    """The share of n01_passes the restated certificate decides on the emulated chain."""
    g, k = n01_passes(shape, dtype_f32)
    return float(certify_np(z32(shape, g, k), bound_np(shape, g)[:, None]).mean())
