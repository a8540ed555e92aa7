"""The host model of the two-hidden-layer ReLU certificate (csrc/pg_relu2_bound.h)
in plain numpy, for both layouts that hold such a network -- LANES: k_relu2's
lanes of a wave (csrc/pg_hidden2.hpp), [6, H1 <= 64, H2 <= 64, O]; BLOCK:
k_relu2_block's 256-thread block (csrc/pg_relu2_block.hip), up to 128 x 128 --
shared by tests/test_relu2_host.py, tests/test_gpu_relu2.py and
tests/test_gpu_relu2_block.py: the f32 chain of a network in the kernel's
documented order, on the once-rounded fused multiply-add of
tests/_relu_model.py; numpy_nn's f64 chain and its decision; the gcc-compiled
bound and its numpy restatement; builders of the networks a random draw does
not reach.  What does not depend on the layout (the genome layout, z64, s_max,
the builders) takes none.  Everything is vectorised over a leading axis of
networks."""
import os
import subprocess
from typing import Callable, NamedTuple

import numpy as np

from _relu_model import RELU_CAP, U32, _fma32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_HDR = os.path.join(REPO, "neuro-genetic-pong-self-play_amd", "csrc", "pg_relu2_bound.h")

# the issue's shapes, plus [6, 32, 17, 2] and [6, 20, 32, 4]: the 16-lane instance (widths 17..32), which none of
# the issue's shapes reaches, with padding in either layer; [6, 16, 16, 4] and [6, 32, 32, 3] complete the
# (lane layout, outputs) cells: the 4-lane layout with 4 outputs and the 16-lane layout with 3 (tests/_sig2_model.py
# imports this list, so k_sig2's sweeps reach the same cells)
SHAPES = [[6, 2, 2, 2], [6, 5, 4, 2], [6, 16, 16, 3], [6, 17, 33, 4], [6, 64, 2, 2], [6, 2, 64, 3], [6, 63, 64, 4],
          [6, 64, 64, 3], [6, 32, 17, 2], [6, 20, 32, 4], [6, 16, 16, 4], [6, 32, 32, 3]]
# both waves of a network, the 64/65 and 127/128 edges, padding in either layer, every O
BLOCK_SHAPES = [[6, 2, 2, 2], [6, 65, 2, 2], [6, 2, 65, 3], [6, 64, 65, 2], [6, 65, 64, 4], [6, 100, 100, 3],
                [6, 127, 128, 4], [6, 128, 127, 2], [6, 128, 128, 3], [6, 128, 128, 4]]


def lanes(H1, H2):
    """hidden2_lanes / hidden2_units (pg_hidden2.hpp): lanes per network, units of each layer per lane."""
    m = max(H1, H2)
    LN = 4 if m <= 16 else (16 if m <= 32 else 32)
    return LN, (4 if LN == 4 else 2)


def _terms_lanes(w3, h2):
    """A lane's U units, in order, by fused multiply-adds from 0."""
    acc = np.zeros(h2.shape[:-1], np.float32)
    for v in range(h2.shape[-1]):
        acc = _fma32(w3[..., v], h2[..., v], acc)
    return acc


def _terms_block(w3, h2):
    """A thread's one product, f32 x f32 rounded once (not fma(w, h, 0): that differs in the sign of a zero)."""
    t = w3[..., 0] * h2[..., 0]
    assert t.dtype == np.float32
    return t


class Layout(NamedTuple):
    """pg_relu2_layout (pg_relu2_bound.h) with what the model needs besides."""
    name: str  # also the gcc program's argument
    macros: str  # the header's macros of this layout: {macros}_CHAIN1.., {macros}_MAX_H, {macros}_K
    chain: tuple  # roundings a term of layer 1, 2, 3 passes through
    sum_ops: int  # operations of the layer-3 sum that feed one output beyond a term's own chain
    max_h: int
    SHAPES: list
    lanes: Callable  # (H1, H2) -> (LN, U): the threads that hold a network, the (padded) units of each
    terms3: Callable  # the order of layer 3 up to the tree: (w3 [N, 1, LN, U], h2 [N, m, LN, U]) -> [N, m, LN]

    @property
    def K(self):
        return float(sum(self.chain) + 2)

    @property
    def under(self):
        """The underflow term's two constants: the factor of max_o sum_k |W3_ok| beside 2 sum_j A_j, and the addend."""
        return float(self.chain[1] + 3), float(16 + self.sum_ops)


LANES = Layout("lanes", "PG_RELU2", (9, 65, 11), 0, 64, SHAPES, lanes, _terms_lanes)
BLOCK = Layout("block", "PG_RELU2_BLOCK", (9, 129, 10), 128 + 127, 128, BLOCK_SHAPES, lambda H1, H2: (128, 1),
               _terms_block)


def genes(shape):
    return sum((shape[i] + 1) * shape[i + 1] for i in range(len(shape) - 1))


def split(shape, g):
    """W1 [.., H1, 7], W2 [.., H2, H1 + 1], W3 [.., O, H2 + 1] of genomes g [.., G] (numpy_nn.py:52-69)."""
    _, H1, H2, O = shape
    g = np.asarray(g)
    a, b = H1 * 7, H1 * 7 + H2 * (H1 + 1)
    lead = g.shape[:-1]
    return (g[..., :a].reshape(lead + (H1, 7)), g[..., a:b].reshape(lead + (H2, H1 + 1)),
            g[..., b:].reshape(lead + (O, H2 + 1)))


def pack(w1, w2, w3):
    return np.concatenate([np.asarray(w, np.float64).ravel() for w in (w1, w2, w3)])


def bounds(tmp_path, layout, shape, nets):
    """pg_relu2_bound_genome, under layout, of each genome of nets [N, G] through a stand-alone gcc program
    (exit status 2: one of the header's macros is not what the layouts here say)."""
    exe = tmp_path / "b2"
    if not exe.exists():
        pins = " || ".join(f"{l.macros}_{n} != {v}" for l in (LANES, BLOCK)
                           for n, v in zip(("CHAIN1", "CHAIN2", "CHAIN3", "MAX_H", "K"), l.chain + (l.max_h, l.K)))
        src = tmp_path / "b2.c"
        src.write_text(f'#include <stdio.h>\n#include <stdlib.h>\n#include <string.h>\n#include "{BOUND_HDR}"\n'
                       "int main(int argc, char **argv){ FILE *f = fopen(argv[2], \"rb\"); int hdr[4];\n"
                       f" if ({pins}) return 2;\n"
                       " const pg_relu2_layout l = strcmp(argv[1], \"block\") ? pg_relu2_layout_lanes() : pg_relu2_layout_block();\n"
                       " while (fread(hdr, sizeof(int), 4, f) == 4) { int H1 = hdr[0], H2 = hdr[1], O = hdr[2];\n"
                       "  size_t G = (size_t)hdr[3]; double *g = malloc(G * sizeof(double));\n"
                       "  if (fread(g, sizeof(double), G, f) != G) return 1;\n"
                       "  printf(\"%a\\n\", (double)pg_relu2_bound_genome(l, g, H1, H2, O)); free(g); }\n"
                       " return 0; }\n")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    data = tmp_path / "nets2.bin"
    nets = np.atleast_2d(np.ascontiguousarray(nets, np.float64))
    assert nets.shape[1] == genes(shape)
    with open(data, "wb") as fh:
        for g in nets:
            fh.write(np.array([shape[1], shape[2], shape[3], len(g)], np.int32).tobytes())
            fh.write(g.tobytes())
    out = subprocess.run([str(exe), layout.name, str(data)], capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(v) for v in out])


def bound_numpy(layout, shape, g):
    """pg_relu2_bound_genome restated, every sum in the header's serial
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
        w3c, c = layout.under
        under = 2.0 ** -126 * (15.0 * tmax + (2.0 * asum + w3c) * w3max + 2.0 * Bs + c)
        e = ((layout.K * U32) * smax + under) * (1.0 + 2.0 ** -20)
        return np.where(ok, e, np.inf).astype(np.float32)


def z32(layout, shape, g, k):
    """The layout's f32 chain (pg_hidden2.hpp hidden2_z32; pg_relu2_block.hip block_z32) for genomes g [N, G] on
    doubled centroids k [N, m, 6] -> [N, m, O]: layer 1 as six fmas onto the bias; layer 2 one fma per padded
    layer-1 unit, in ascending order, onto the bias; layer 3 the terms of the network's LN threads, a pairwise
    tree over them, then the output bias.  The terms and the tree:
      LANES  lane hl's units hl U + v in order by fmas from 0; the tree over the LN lanes (group_sum);
      BLOCK  one product per thread (padded unit); the tree over each wave's 64 lanes (group_sum<64>: every step
             adds the same two operands in both partner lanes), then wave 0's sum + wave 1's."""
    _, H1, H2, O = shape
    LN, U = layout.lanes(H1, H2)
    P = LN * U
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
        h2 = np.maximum(a2, np.float32(0)).reshape(N, m, LN, U)
        w3p = np.zeros((N, O, P), np.float32)
        w3p[:, :, :H2] = w3[:, :, :H2]
        w3p = w3p.reshape(N, O, LN, U)
        z = np.empty((N, m, O), np.float32)
        for o in range(O):
            acc = layout.terms3(w3p[:, None, o], h2)
            while acc.shape[2] > 1:
                acc = acc[:, :, 0::2] + acc[:, :, 1::2]
            z[:, :, o] = acc[:, :, 0] + w3[:, None, o, H2]
    return z


def z64(shape, g, k):
    """numpy_nn's f64 output pre-activations (NeuralNetwork.run numpy_nn.py:126-131 with ReLU), np.dot per pass."""
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
                a1[:-1] = np.maximum(0.0, np.dot(w1[n], a0))
                a2 = np.ones(H2 + 1)
                a2[:-1] = np.maximum(0.0, np.dot(w2[n], a1))
                z[n, t] = np.dot(w3[n], a2)
    return z


def s_max(shape, g):
    """max_o S_o of genomes g [.., G] (pg_relu2_bound.h)."""
    _, H1, H2, O = shape
    w1, w2, w3 = (np.abs(w) for w in split(shape, np.asarray(g, np.float64)))
    with np.errstate(all="ignore"):
        A = w1.sum(axis=-1)
        B = np.einsum("...kj,...j->...k", w2[..., :H1], A) + w2[..., H1]
        return (np.einsum("...ok,...k->...o", w3[..., :H2], B) + w3[..., H2]).max(axis=-1)


def cap_net(shape, scale, seed=0):
    """Signed N(0,1) weights, the three weight matrices scaled by m and the
    biases of layer l by m^l, so that max_o S_o = scale (S_o is cubic in m).
    For scale near PG_RELU_CAP every gene stays far inside f32's range and the
    bound's other sums (~m^2) far below the cap: S_o alone decides the side."""
    _, H1, H2, O = shape
    rng = np.random.default_rng([H1, H2, O, seed, 7])
    g = rng.standard_normal(genes(shape))
    w1, w2, w3 = (w.copy() for w in split(shape, g))
    m = np.cbrt(scale / s_max(shape, g))
    w1 *= m
    w2[:, :H1] *= m
    w2[:, H1] *= m * m
    w3[:, :H2] *= m
    w3[:, H2] *= m ** 3
    return pack(w1, w2, w3)


def tiny_net(shape, rng):
    """Signed genes of magnitude 1e-36 down to 1e-60: subnormal in f32, or zero."""
    G = genes(shape)
    return np.where(rng.random(G) < 0.5, -1.0, 1.0) * 10.0 ** -rng.uniform(36.0, 60.0, G)


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
