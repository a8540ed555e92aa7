"""The host model of the three-hidden-layer ReLU certificate (csrc/pg_relu3_bound.h,
k_relu3: csrc/pg_hidden3.hpp) in plain numpy, shared by tests/test_relu3_host.py
and tests/test_gpu_relu3.py: the f32 chain of a network in the kernel's
documented order, on the once-rounded fused multiply-add of
tests/_relu_model.py; numpy_nn's f64 chain and its decision; the gcc-compiled
bound and its numpy restatement; builders of the networks a random draw does
not reach.  Everything is vectorised over a leading axis of networks."""
import os
import subprocess

import numpy as np

from _relu2_model import certify  # noqa: F401  (relu_certify: the same certificate)
from _relu_model import RELU_CAP, U32, _fma32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_HDR = os.path.join(REPO, "neuro-genetic-pong-self-play_amd", "csrc", "pg_relu3_bound.h")

# all padding; the 8-lane layout full; each layer alone forcing the 16-lane layout; mixed padding; full
SHAPES = [[6, 2, 2, 2, 2], [6, 16, 16, 16, 3], [6, 16, 16, 16, 4], [6, 17, 2, 2, 2], [6, 2, 17, 2, 3],
          [6, 2, 2, 17, 4], [6, 9, 32, 5, 3], [6, 32, 32, 32, 2], [6, 32, 32, 32, 3], [6, 32, 32, 32, 4]]
CHAIN = (9, 33, 33, 8)  # roundings a term of layer 1, 2, 3, 4 passes through (PG_RELU3_CHAIN1..4)
K = float(sum(CHAIN) + 2)
MAX_H = 32
UNITS = 2


def lanes(shape):
    """hidden3_lanes (pg_hidden3.hpp): lanes per network; two units of each layer per lane."""
    return 8 if max(shape[1:4]) <= 16 else 16


def genes(shape):
    return sum((shape[i] + 1) * shape[i + 1] for i in range(len(shape) - 1))


def split(shape, g):
    """W1 [.., H1, 7], W2 [.., H2, H1 + 1], W3 [.., H3, H2 + 1], W4 [.., O, H3 + 1] of genomes g [.., G]
    (numpy_nn.py:52-69)."""
    g = np.asarray(g)
    lead, out, at = g.shape[:-1], [], 0
    for a, b in zip(shape[:-1], shape[1:]):
        out.append(g[..., at:at + (a + 1) * b].reshape(lead + (b, a + 1)))
        at += (a + 1) * b
    assert at == g.shape[-1]
    return out


def pack(*ws):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in ws])


def bounds(tmp_path, shape, nets):
    """pg_relu3_bound_genome of each genome of nets [N, G] through a stand-alone gcc program (exit status 2: one
    of the header's macros is not what this model says)."""
    exe = tmp_path / "b3"
    if not exe.exists():
        pins = " || ".join(f"PG_RELU3_{n} != {v}" for n, v in
                           zip(("CHAIN1", "CHAIN2", "CHAIN3", "CHAIN4", "MAX_H", "K"), CHAIN + (MAX_H, K)))
        src = tmp_path / "b3.c"
        src.write_text(f'#include <stdio.h>\n#include <stdlib.h>\n#include "{BOUND_HDR}"\n'
                       "int main(int argc, char **argv){ FILE *f = fopen(argv[1], \"rb\"); int hdr[5];\n"
                       f" if ({pins}) return 2;\n"
                       " while (fread(hdr, sizeof(int), 5, f) == 5) { size_t G = (size_t)hdr[4];\n"
                       "  double *g = malloc(G * sizeof(double));\n"
                       "  if (fread(g, sizeof(double), G, f) != G) return 1;\n"
                       "  printf(\"%a\\n\", (double)pg_relu3_bound_genome(g, hdr[0], hdr[1], hdr[2], hdr[3])); free(g); }\n"
                       " return 0; }\n")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    data = tmp_path / "nets3.bin"
    nets = np.atleast_2d(np.ascontiguousarray(nets, np.float64))
    assert nets.shape[1] == genes(shape)
    with open(data, "wb") as fh:
        for g in nets:
            fh.write(np.array(list(shape[1:]) + [len(g)], np.int32).tobytes())
            fh.write(g.tobytes())
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(v) for v in out])


def _abs_sums(shape, g):
    """A [N, H1], B [N, H2], V2 [N, H2], C [N, H3], T3 [N, H3], V3 [N, H3] of pg_relu3_bound.h, every sum in the
    header's serial order."""
    _, H1, H2, H3, O = shape
    w1, w2, w3, w4 = (np.abs(w) for w in split(shape, np.atleast_2d(np.asarray(g, np.float64))))
    N = w1.shape[0]
    A = np.zeros((N, H1))
    for i in range(7):
        A = A + w1[:, :, i]
    B, V2 = np.zeros((N, H2)), np.zeros((N, H2))
    for j in range(H1):
        B = B + w2[:, :, j] * A[:, j:j + 1]
        V2 = V2 + w2[:, :, j]
    B = B + w2[:, :, H1]
    C, T3, V3 = np.zeros((N, H3)), np.zeros((N, H3)), np.zeros((N, H3))
    for k in range(H2):
        C = C + w3[:, :, k] * B[:, k:k + 1]
        T3 = T3 + w3[:, :, k] * V2[:, k:k + 1]
        V3 = V3 + w3[:, :, k]
    C = C + w3[:, :, H2]
    return A, B, V2, C, T3, V3, w4


def _serial(v):
    s = np.zeros(v.shape[0])
    for i in range(v.shape[1]):
        s = s + v[:, i]
    return s


def bound_numpy(shape, g):
    """pg_relu3_bound_genome restated: e of genomes g [N, G] as f32 (inf past PG_RELU_CAP or for NaN)."""
    _, H1, H2, H3, O = shape
    with np.errstate(all="ignore"):
        A, B, V2, C, T3, V3, w4 = _abs_sums(shape, g)
        N = A.shape[0]
        S, Q, R, W4 = (np.zeros((N, O)) for _ in range(4))
        for l in range(H3):
            S = S + w4[:, :, l] * C[:, l:l + 1]
            Q = Q + w4[:, :, l] * T3[:, l:l + 1]
            R = R + w4[:, :, l] * V3[:, l:l + 1]
            W4 = W4 + w4[:, :, l]
        S = S + w4[:, :, H3]
        asum, bsum, csum, w2s, w3s = _serial(A), _serial(B), _serial(C), _serial(V2), _serial(V3)
        ok = (asum <= RELU_CAP) & (bsum <= RELU_CAP) & (csum <= RELU_CAP) & (w2s <= RELU_CAP) & (w3s <= RELU_CAP)
        ok &= ((S <= RELU_CAP) & (Q <= RELU_CAP) & (R <= RELU_CAP) & (W4 <= RELU_CAP)).all(axis=-1)
        smax, qmax, rmax, w4max = (np.where(np.isnan(v), 0.0, v).max(axis=-1) for v in (S, Q, R, W4))
        under = 2.0 ** -126 * (16.0 * qmax + (3.0 * asum + (CHAIN[1] + 4.0)) * rmax
                               + (3.0 * bsum + (CHAIN[2] + 3.0)) * w4max + 2.0 * csum + 16.0)
        e = ((K * U32) * smax + under) * (1.0 + 2.0 ** -20)
        return np.where(ok, e, np.inf).astype(np.float32)


def s_max(shape, g):
    """max_o S_o of genomes g [.., G] (pg_relu3_bound.h)."""
    ws = [np.abs(w) for w in split(shape, np.asarray(g, np.float64))]
    with np.errstate(all="ignore"):
        a = ws[0].sum(axis=-1)
        for w in ws[1:]:
            a = np.einsum("...kj,...j->...k", w[..., :-1], a) + w[..., -1]
        return a.max(axis=-1)


def _layer32(w, h, P):
    """One hidden layer of hidden3_z32: w [N, H, Hin + 1] f32, h [N, m, P] (padded) -> max(0, .) [N, m, P]: one
    fma per padded input unit, in ascending order, onto the bias."""
    N, H, Hin = w.shape[0], w.shape[1], w.shape[2] - 1
    wp = np.zeros((N, P, P), np.float32)
    wp[:, :H, :Hin] = w[:, :, :Hin]
    a = np.zeros(h.shape[:2] + (P,), np.float32)
    a[:, :, :H] = w[:, None, :, Hin]
    for j in range(P):
        a = _fma32(wp[:, None, :, j], h[:, :, j:j + 1], a)
    return np.maximum(a, np.float32(0))


def z32(shape, g, k):
    """The kernel's f32 chain (pg_hidden3.hpp hidden3_z32) for genomes g [N, G] on doubled centroids k [N, m, 6]
    -> [N, m, O]: layer 1 as six fmas onto the bias; layers 2 and 3 one fma per padded unit of the layer before,
    in ascending order, onto the bias; layer 4 lane hl's units 2 hl, 2 hl + 1 in order by fmas from 0, a pairwise
    tree over the LN lanes (group_sum), then the output bias."""
    _, H1, H2, H3, O = shape
    LN = lanes(shape)
    P = LN * UNITS
    with np.errstate(all="ignore"):
        w1, w2, w3, w4 = (w.astype(np.float32) for w in split(shape, g))
        N, m = k.shape[0], k.shape[1]
        x = k.astype(np.float32) * np.float32(0.003125)  # feat32
        a = np.broadcast_to(w1[:, None, :, 6], (N, m, H1)).copy()
        for i in range(6):
            a = _fma32(w1[:, None, :, i], x[:, :, i:i + 1], a)
        h1 = np.zeros((N, m, P), np.float32)
        h1[:, :, :H1] = np.maximum(a, np.float32(0))
        h3 = _layer32(w3, _layer32(w2, h1, P), P).reshape(N, m, LN, UNITS)
        w4p = np.zeros((N, O, P), np.float32)
        w4p[:, :, :H3] = w4[:, :, :H3]
        w4p = w4p.reshape(N, O, LN, UNITS)
        z = np.empty((N, m, O), np.float32)
        for o in range(O):
            acc = np.zeros((N, m, LN), np.float32)
            for v in range(UNITS):
                acc = _fma32(w4p[:, None, o, :, v], h3[..., v], acc)
            while acc.shape[2] > 1:
                acc = acc[:, :, 0::2] + acc[:, :, 1::2]
            z[:, :, o] = acc[:, :, 0] + w4[:, None, o, H3]
    return z


def _passes(shape, g, k):
    ws = split(shape, np.asarray(g, np.float64))
    N, m = k.shape[0], k.shape[1]
    z = np.empty((N, m, shape[-1]))
    idx = np.empty((N, m), np.int32)
    with np.errstate(all="ignore"):
        for n in range(N):
            for t in range(m):
                a = np.ones(7)
                a[:6] = (k[n, t] / 2) / 160
                for w in ws:
                    zz = np.dot(w[n], a)
                    h = np.maximum(0.0, zz)
                    a = np.append(h, 1.0)
                z[n, t] = zz
                idx[n, t] = np.argmax(h)
    return z, idx


def z64(shape, g, k):
    """numpy_nn's f64 output pre-activations (NeuralNetwork.run numpy_nn.py:126-131 with ReLU), np.dot per pass."""
    return _passes(shape, g, k)[0]


def numpy_index(shape, g, k):
    """NeuralNetwork.run's decision (numpy_nn.py:120-137 with ReLU) for genomes g [N, G] on doubled centroids
    k [N, m, 6] -> [N, m] int32: np.dot per layer on [h; 1], np.maximum, np.argmax, pass by pass."""
    return _passes(shape, g, k)[1]


def cap_net(shape, scale, seed=0):
    """Signed N(0,1) weights, the four weight matrices scaled by m and the biases of layer l by m^l, so that
    max_o S_o = scale (S_o is quartic in m).  For scale near PG_RELU_CAP every gene stays far inside f32's range
    and the bound's other sums (~m^3) far below the cap: S_o alone decides the side."""
    rng = np.random.default_rng(list(shape) + [seed, 7])
    g = rng.standard_normal(genes(shape))
    ws = [w.copy() for w in split(shape, g)]
    m = (scale / s_max(shape, g)) ** 0.25
    for l, w in enumerate(ws):
        w[:, :-1] *= m
        w[:, -1] *= m ** (l + 1)
    return pack(*ws)


def tiny_net(shape, rng):
    """Signed genes of magnitude 1e-36 down to 1e-60: subnormal in f32, or zero."""
    G = genes(shape)
    return np.where(rng.random(G) < 0.5, -1.0, 1.0) * 10.0 ** -rng.uniform(36.0, 60.0, G)


def systematic_net(shape, seed=0):
    """All weights positive (nothing cancels) and every gene an f32 value v = 2^p (1 + j 2^-23) times
    (1 + 0.49 * 2^-23): every conversion to f32 rounds down by 0.98 u, all the same way.  Meant for k = 320 on
    every feature."""
    rng = np.random.default_rng(list(shape) + [seed])
    G = genes(shape)
    v = np.ldexp(1.0 + rng.integers(0, 1 << 16, G) * 2.0 ** -23, rng.integers(-3, 1, G))
    g = v * (1.0 + 0.49 * 2.0 ** -23)
    assert (g.astype(np.float32) == v).all() and (g > v).all()
    return g


def tie_net(shape, delta, rng):
    """A random network whose output rows are all equal and non-negative (every output is > 0: its bias is),
    apart from the last output's bias being delta larger: z_last - z_o = delta exactly in exact arithmetic,
    whatever the input."""
    ws = [w.copy() for w in split(shape, rng.standard_normal(genes(shape)))]
    ws[-1][:] = np.abs(ws[-1][0])
    ws[-1][-1, -1] = ws[-1][0, -1] + delta
    return pack(*ws)
