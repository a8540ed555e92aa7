"""The host model of k_relu2_block's decision (csrc/pg_relu2_block.hip,
pg_relu2_block_bound.h) in plain numpy, shared by tests/test_relu2_block_host.py
and tests/test_gpu_relu2_block.py: the f32 chain of a [6, H1 <= 128, H2 <= 128,
O] ReLU network in the kernel's documented order, on the once-rounded fused
multiply-add of tests/_relu_model.py; numpy_nn's own forward; the gcc-compiled
bound and its numpy restatement.  The genome layout, numpy's f64 chain, max_o
S_o and the builders cap_net and tiny_net are tests/_relu2_model.py's: they do
not depend on the layout.  Everything is vectorised over a leading axis of
networks."""
import os
import subprocess

import numpy as np

from _relu2_model import cap_net, genes, pack, s_max, split, tiny_net, z64  # noqa: F401 (re-exported)
from _relu_model import RELU_CAP, U32, _fma32  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_HDR = os.path.join(REPO, "neuro-genetic-pong-self-play_amd", "csrc", "pg_relu2_block_bound.h")
P = 128  # PG_RELU2_BLOCK_MAX_H: threads per network, padded units per hidden layer
CHAIN1, CHAIN2, CHAIN3 = 9, 129, 10
BLOCK_K = 150.0  # PG_RELU2_BLOCK_K = 9 + 129 + 10 + 2

# both waves of a network, the 64/65 and 127/128 edges, padding in either layer, every O
SHAPES = [[6, 2, 2, 2], [6, 65, 2, 2], [6, 2, 65, 3], [6, 64, 65, 2], [6, 65, 64, 4], [6, 100, 100, 3],
          [6, 127, 128, 4], [6, 128, 127, 2], [6, 128, 128, 3], [6, 128, 128, 4]]


def bounds(tmp_path, shape, nets):
    """pg_relu2_block_bound_genome of each genome of nets [N, G] through a stand-alone gcc program."""
    exe = tmp_path / "b2b"
    if not exe.exists():
        src = tmp_path / "b2b.c"
        src.write_text(f'#include <stdio.h>\n#include <stdlib.h>\n#include "{BOUND_HDR}"\n'
                       "int main(int argc, char **argv){ FILE *f = fopen(argv[1], \"rb\"); int hdr[4];\n"
                       " if (PG_RELU2_BLOCK_K != 150.0 || PG_RELU2_BLOCK_CHAIN1 != 9 || PG_RELU2_BLOCK_CHAIN2 != 129 ||\n"
                       "     PG_RELU2_BLOCK_CHAIN3 != 10 || PG_RELU2_BLOCK_MAX_H != 128) return 2;\n"
                       " while (fread(hdr, sizeof(int), 4, f) == 4) { int H1 = hdr[0], H2 = hdr[1], O = hdr[2];\n"
                       "  size_t G = (size_t)hdr[3]; double *g = malloc(G * sizeof(double));\n"
                       "  if (fread(g, sizeof(double), G, f) != G) return 1;\n"
                       "  printf(\"%a\\n\", (double)pg_relu2_block_bound_genome(g, H1, H2, O)); free(g); }\n"
                       " return 0; }\n")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    data = tmp_path / "nets2b.bin"
    nets = np.atleast_2d(np.ascontiguousarray(nets, np.float64))
    assert nets.shape[1] == genes(shape)
    with open(data, "wb") as fh:
        for g in nets:
            fh.write(np.array([shape[1], shape[2], shape[3], len(g)], np.int32).tobytes())
            fh.write(g.tobytes())
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(v) for v in out])


def bound_numpy(shape, g):
    """pg_relu2_block_bound_genome restated, every sum in the header's serial
    order: e of genomes g [N, G] as f32 (inf past PG_RELU_CAP or for NaN)."""
    _, H1, H2, O = shape
    w1, w2, w3 = (np.abs(w) for w in split(shape, np.atleast_2d(np.asarray(g, np.float64))))
    N = w1.shape[0]
    with np.errstate(all="ignore"):
        A = np.zeros((N, H1))
        for i in range(7):
            A = A + w1[:, :, i]
        asum = np.zeros(N)
        for j in range(H1):
            asum = asum + A[:, j]
        b, w = np.zeros((N, H2)), np.zeros((N, H2))
        for j in range(H1):
            b = b + w2[:, :, j] * A[:, j:j + 1]
            w = w + w2[:, :, j]
        b = b + w2[:, :, H1]
        S, T, W3 = np.zeros((N, O)), np.zeros((N, O)), np.zeros((N, O))
        Bs, W2s = np.zeros(N), np.zeros(N)
        for k in range(H2):
            S = S + w3[:, :, k] * b[:, k:k + 1]
            T = T + w3[:, :, k] * w[:, k:k + 1]
            W3 = W3 + w3[:, :, k]
            Bs = Bs + b[:, k]
            W2s = W2s + w[:, k]
        S = S + w3[:, :, H2]
        ok = (asum <= RELU_CAP) & (Bs <= RELU_CAP) & (W2s <= RELU_CAP)
        ok &= ((S <= RELU_CAP) & (T <= RELU_CAP) & (W3 <= RELU_CAP)).all(axis=-1)
        smax, tmax, w3max = (np.where(np.isnan(v), 0.0, v).max(axis=-1) for v in (S, T, W3))
        under = 2.0 ** -126 * (15.0 * tmax + (2.0 * asum + 132.0) * w3max + 2.0 * Bs + 271.0)
        e = ((BLOCK_K * U32) * smax + under) * (1.0 + 2.0 ** -20)
        return np.where(ok, e, np.inf).astype(np.float32)


def z32(shape, g, k):
    """k_relu2_block's f32 chain for genomes g [N, G] on doubled centroids k
    [N, m, 6] -> [N, m, O]: layer 1 as six fmas onto the bias; layer 2 one fma
    per padded layer-1 unit (128), in ascending order, onto the bias; layer 3
    one product per thread (padded unit), summed over each wave's 64 lanes by
    a pairwise tree (group_sum<64>: every step adds the same two operands in
    both partner lanes), then wave 0's sum + wave 1's, then the output bias."""
    _, H1, H2, O = shape
    with np.errstate(all="ignore"):
        w1, w2, w3 = (w.astype(np.float32) for w in split(shape, g))
        N, m = k.shape[0], k.shape[1]
        x = k.astype(np.float32) * np.float32(0.003125)  # feat32
        a = np.broadcast_to(w1[:, None, :, 6], (N, m, H1)).copy()
        for i in range(6):
            a = _fma32(w1[:, None, :, i], x[:, :, i:i + 1], a)
        h1 = np.zeros((N, m, P), np.float32)
        h1[:, :, :H1] = np.maximum(a, np.float32(0))
        w2p = np.zeros((N, P, P), np.float32)
        w2p[:, :H2, :H1] = w2[:, :, :H1]
        a2 = np.zeros((N, m, P), np.float32)
        a2[:, :, :H2] = w2[:, None, :, H1]
        for j in range(P):
            a2 = _fma32(w2p[:, None, :, j], h1[:, :, j:j + 1], a2)
        h2 = np.maximum(a2, np.float32(0))
        w3p = np.zeros((N, O, P), np.float32)
        w3p[:, :, :H2] = w3[:, :, :H2]
        z = np.empty((N, m, O), np.float32)
        for o in range(O):
            t = w3p[:, None, o, :] * h2  # f32 x f32: rounded once
            assert t.dtype == np.float32
            while t.shape[2] > 1:  # 6 steps within a wave, then the two waves
                t = t[:, :, 0::2] + t[:, :, 1::2]
            z[:, :, o] = t[:, :, 0] + w3[:, None, o, H2]
    return z


def numpy_index(shape, g, k):
    """NeuralNetwork.run's decision (numpy_nn.py:120-137 with ReLU) for genomes
    g [N, G] on doubled centroids k [N, m, 6] -> [N, m] int32: np.dot per layer
    on [h; 1], np.maximum, np.argmax, pass by pass."""
    _, H1, H2, O = shape
    w1, w2, w3 = split(shape, np.asarray(g, np.float64))
    N, m = k.shape[0], k.shape[1]
    out = np.empty((N, m), np.int32)
    with np.errstate(all="ignore"):
        for n in range(N):
            for t in range(m):
                a = np.ones(7)
                a[:6] = (k[n, t] / 2) / 160
                for w in (w1[n], w2[n], w3[n]):
                    h = np.maximum(0.0, np.dot(w, a))
                    a = np.append(h, 1.0)
                out[n, t] = np.argmax(h)
    return out


def certify(z, e):
    """relu_certify (pg_relu.hpp) on z [.., O] f32 under e [..] f32: the proven index, or -1."""
    z = np.asarray(z, np.float32)
    e = np.asarray(e, np.float32)
    srt = np.sort(z, axis=-1)
    t1, t2 = srt[..., -1], srt[..., -2]
    i1 = np.argmax(z, axis=-1)  # the first maximum: a tie keeps the lower index
    with np.errstate(all="ignore"):
        low = t1 <= -e
        top = (t1 > e) & ((t1 - t2).astype(np.float32) > np.float32(2) * e)
    return np.where(~np.isfinite(e), -1, np.where(low, 0, np.where(top, i1, -1)))


def systematic_net(shape, seed=0):
    """All weights positive (nothing cancels) and every gene an f32 value
    v = 2^p (1 + j 2^-23) times (1 + 0.49 * 2^-23): every conversion to f32
    rounds down by 0.98 u, all the same way (tests/_relu_model.py's, for this
    layout).  Meant for k = 320 on every feature."""
    rng = np.random.default_rng(list(shape) + [seed])
    G = genes(shape)
    v = np.ldexp(1.0 + rng.integers(0, 1 << 16, G) * 2.0 ** -23, rng.integers(-3, 1, G))
    g = v * (1.0 + 0.49 * 2.0 ** -23)
    assert (g.astype(np.float32) == v).all() and (g > v).all()
    return g
