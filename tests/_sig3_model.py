"""The host model of the three-hidden-layer sigmoid certificate (csrc/pg_sig3_bound.h,
k_sig3: csrc/pg_sig3.hpp) in plain numpy, shared by tests/test_sig3_host.py and
tests/test_gpu_sig3.py: the f32 chain of a network in the kernel's documented
order, on the once-rounded fused multiply-add of tests/_relu_model.py with the
emulated f32 sigmoid of tests/_sig2_model.py; numpy_nn's f64 chain and its
decision; the gcc-compiled bound and its numpy restatement; builders of the
networks a random draw does not reach.  Everything is vectorised over a
leading axis of networks."""
import os
import subprocess

import numpy as np

from _relu3_model import UNITS, genes, lanes, pack, split, tiny_net, systematic_net  # noqa: F401  (the layout is k_relu3's)
from _relu_model import _fma32
from _sig2_model import CAP, ETA, SIG, SLOPE, U32, _sig32, sigmoid64  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_HDR = os.path.join(REPO, "neuro-genetic-pong-self-play_amd", "csrc", "pg_sig3_bound.h")

# the minimum; the 8-lane layout full; each layer alone forcing the 16-lane layout; uneven widths; the 16-lane layout full
SHAPES = [[6, 2, 2, 2, 2], [6, 16, 16, 16, 2], [6, 16, 16, 16, 3], [6, 16, 16, 16, 4], [6, 17, 2, 2, 2],
          [6, 2, 17, 2, 3], [6, 2, 2, 17, 4], [6, 9, 32, 5, 3], [6, 32, 32, 32, 2], [6, 32, 32, 32, 3],
          [6, 32, 32, 32, 4]]
CHAIN = (9, 33, 33, 8)            # roundings a term of layer 1, 2, 3, 4 passes through (PG_SIG3_CHAIN1..4)
UNDER = (1.0, 6.0, 23.0, 96.0)    # PG_SIG3_UNDER_Q, _R, _W4, _C
MAX_H = 32


def bounds(tmp_path, shape, nets):
    """pg_sig3_bound_genome of each genome of nets [N, G] through a stand-alone gcc program (exit status 2: one
    of the header's macros is not what this model says)."""
    exe = tmp_path / "bs3"
    if not exe.exists():
        pins = [f"PG_SIG3_{n} != {v}" for n, v in zip(("CHAIN1", "CHAIN2", "CHAIN3", "CHAIN4"), CHAIN)]
        pins += [f"PG_SIG3_UNDER_{n} != {v}" for n, v in zip(("Q", "R", "W4", "C"), UNDER)]
        pins += [f"PG_SIG3_MAX_H != {MAX_H}", f"PG_SIG2_SIG != {SIG}", f"PG_SIG2_SLOPE != {SLOPE}", "PG_SIG2_CAP != 1e25"]
        src = tmp_path / "bs3.c"
        src.write_text(f'#include <stdio.h>\n#include <stdlib.h>\n#include "{BOUND_HDR}"\n'
                       "int main(int argc, char **argv){ FILE *f = fopen(argv[1], \"rb\"); int hdr[5];\n"
                       f" if ({' || '.join(pins)}) return 2;\n"
                       " while (fread(hdr, sizeof(int), 5, f) == 5) { size_t G = (size_t)hdr[4];\n"
                       "  double *g = malloc(G * sizeof(double));\n"
                       "  if (fread(g, sizeof(double), G, f) != G) return 1;\n"
                       "  printf(\"%a\\n\", (double)pg_sig3_bound_genome(g, hdr[0], hdr[1], hdr[2], hdr[3])); free(g); }\n"
                       " return 0; }\n")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    data = tmp_path / "nets_s3.bin"
    nets = np.atleast_2d(np.ascontiguousarray(nets, np.float64))
    assert nets.shape[1] == genes(shape)
    with open(data, "wb") as fh:
        for g in nets:
            fh.write(np.array(list(shape[1:]) + [len(g)], np.int32).tobytes())
            fh.write(g.tobytes())
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, check=True).stdout.split()
    return np.array([float.fromhex(v) for v in out]).astype(np.float32)


def _serial(v):
    s = np.zeros(v.shape[0])
    for i in range(v.shape[1]):
        s = s + v[:, i]
    return s


def sums(shape, g):
    """The sums of pg_sig3_bound.h for genomes g [N, G], every one in the header's serial order: S_o (with the
    output bias's share), Q_o, R_o, sum_l |W4_ol| [N, O]; sum_j A_j, sum_k B_k, sum_k P_k, sum_l Q3_l [N]."""
    _, H1, H2, H3, O = shape
    c1, c2, c3, c4 = CHAIN
    w1, w2, w3, w4 = (np.abs(w) for w in split(shape, np.atleast_2d(np.asarray(g, np.float64))))
    N = w1.shape[0]
    with np.errstate(all="ignore"):
        A = np.zeros((N, H1))
        for i in range(7):
            A = A + w1[:, :, i]
        P, V2 = np.zeros((N, H2)), np.zeros((N, H2))
        for j in range(H1):
            P = P + w2[:, :, j] * A[:, j:j + 1]
            V2 = V2 + w2[:, :, j]
        B = V2 + w2[:, :, H1]
        Q2 = (SLOPE * c1) * P + (SIG + c2) * B
        X2 = SLOPE * Q2 + (SIG + c3)
        X, T3, V3 = np.zeros((N, H3)), np.zeros((N, H3)), np.zeros((N, H3))
        for k in range(H2):
            X = X + w3[:, :, k] * X2[:, k:k + 1]
            T3 = T3 + w3[:, :, k] * V2[:, k:k + 1]
            V3 = V3 + w3[:, :, k]
        Q3 = X + c3 * w3[:, :, H2]
        Y = SLOPE * Q3 + (SIG + c4)
        S, Q, R, W4 = (np.zeros((N, O)) for _ in range(4))
        for l in range(H3):
            S = S + w4[:, :, l] * Y[:, l:l + 1]
            Q = Q + w4[:, :, l] * T3[:, l:l + 1]
            R = R + w4[:, :, l] * V3[:, l:l + 1]
            W4 = W4 + w4[:, :, l]
        S = S + c4 * w4[:, :, H3]
        return S, Q, R, W4, _serial(A), _serial(B), _serial(P), _serial(Q3)


def s_max(shape, g):
    """max_o S_o of genomes g [N, G] (pg_sig3_bound.h)."""
    with np.errstate(all="ignore"):
        return sums(shape, g)[0].max(axis=-1)


def bound_np(shape, g):
    """pg_sig3_bound_genome restated: e = (u max_o S_o + eta (max_o Q_o + 6 max_o R_o + 23 max_o sum_l |W4_ol| + 96))
    (1 + 2^-10) as f32, inf when a sum exceeds the cap or is not a number."""
    S, Q, R, W4, a, b, p, q3 = sums(shape, g)
    with np.errstate(all="ignore"):
        ok = (a <= CAP) & (b <= CAP) & (p <= CAP) & (q3 <= CAP)
        ok &= ((S <= CAP) & (Q <= CAP) & (R <= CAP) & (W4 <= CAP)).all(axis=-1)
        smax, qmax, rmax, wmax = (np.where(np.isnan(v), 0.0, v).max(axis=-1) for v in (S, Q, R, W4))
        under = ETA * (UNDER[0] * qmax + UNDER[1] * rmax + UNDER[2] * wmax + UNDER[3])
        e = (U32 * smax + under) * (1.0 + 2.0 ** -10)
        return np.where(ok, e, np.inf).astype(np.float32)


def _layer32(w, h, P, d):
    """One hidden layer of hidden3_z32 with the sigmoid: w [N, H, Hin + 1] f32, h [N, m, P] (padded) -> the emulated sigmoid [N, m, P]
    (padding units 0.5): one fma per padded input unit, in ascending order, onto the bias.  d [N, 1, H]: the
    sigmoids' displacement in u."""
    N, H, Hin = w.shape[0], w.shape[1], w.shape[2] - 1
    wp = np.zeros((N, P, P), np.float32)
    wp[:, :H, :Hin] = w[:, :, :Hin]
    a = np.zeros(h.shape[:2] + (P,), np.float32)
    a[:, :, :H] = w[:, None, :, Hin]
    for j in range(P):
        a = _fma32(wp[:, None, :, j], h[:, :, j:j + 1], a)
    out = np.full(a.shape, 0.5, np.float32)
    out[:, :, :H] = _sig32(a[:, :, :H], d)
    return out


def z32(shape, g, k, out=None, sign=0.0):
    """The kernel's f32 chain (pg_hidden3.hpp hidden3_z32 with the sigmoid) for genomes g [N, G] on doubled centroids k [N, m, 6]
    -> [N, m, O]: layer 1 as six fmas onto the bias; layers 2 and 3 one fma per padded unit of the layer before,
    in ascending order, onto the bias; layer 4 lane hl's units 2 hl, 2 hl + 1 in order by fmas from 0, a pairwise
    tree over the LN lanes (group_sum), then the output bias.  Padding units have activation 0.5 and zero
    outgoing weights.  sign = 0: every sigmoid as the rounded f64 one.  sign = +-1: every sigmoid displaced by
    the full allowance of 4.5 u towards (+1) or away from (-1) raising output `out`, each unit by the sign of
    its linearised influence on it: a layer-3 unit by the sign of its W4 weight, a layer-2 unit by that of
    W4[out] . W3, a layer-1 unit by that of W4[out] . W3 . W2."""
    _, H1, H2, H3, O = shape
    LN = lanes(shape)
    P = LN * UNITS
    with np.errstate(all="ignore"):
        w1, w2, w3, w4 = (w.astype(np.float32) for w in split(shape, g))
        N, m = k.shape[0], k.shape[1]
        d1, d2, d3 = np.zeros((N, 1, H1)), np.zeros((N, 1, H2)), np.zeros((N, 1, H3))
        if sign:
            i3 = w4[:, out, :H3].astype(np.float64)
            i2 = np.einsum("nl,nlk->nk", i3, w3[:, :, :H2].astype(np.float64))
            i1 = np.einsum("nk,nkj->nj", i2, w2[:, :, :H1].astype(np.float64))
            d3, d2, d1 = (sign * SIG * np.sign(i)[:, None, :] for i in (i3, i2, i1))
        x = k.astype(np.float32) * np.float32(0.003125)  # feat32
        a = np.broadcast_to(w1[:, None, :, 6], (N, m, H1)).copy()
        for i in range(6):
            a = _fma32(w1[:, None, :, i], x[:, :, i:i + 1], a)
        h1 = np.full((N, m, P), 0.5, np.float32)
        h1[:, :, :H1] = _sig32(a, d1)
        h3 = _layer32(w3, _layer32(w2, h1, P, d2), P, d3).reshape(N, m, LN, UNITS)
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


def passes(shape, g, k):
    """numpy_nn's chain (NeuralNetwork.run numpy_nn.py:120-137 with the sigmoid) for genomes g [N, G] on doubled
    centroids k [N, m, 6], np.dot per pass: (the last layer's f64 pre-activations [N, m, O], np.argmax of its
    activations [N, m], those activations [N, m, O])."""
    ws = split(shape, np.asarray(g, np.float64))
    N, m = k.shape[0], k.shape[1]
    z = np.empty((N, m, shape[-1]))
    act = np.empty((N, m, shape[-1]))
    idx = np.empty((N, m), np.int32)
    with np.errstate(all="ignore"):
        for n in range(N):
            for t in range(m):
                a = np.ones(7)
                a[:6] = (k[n, t] / 2) / 160
                for w in ws:
                    zz = np.dot(w[n], a)
                    h = 1 / (1 + np.e ** -zz)
                    a = np.append(h, 1.0)
                z[n, t], act[n, t], idx[n, t] = zz, h, np.argmax(h)
    return z, idx, act


def z64(shape, g, k):
    return passes(shape, g, k)[0]


def cap_net(shape, scale, seed=0):
    """Signed N(0,1) genes with the output layer's row of weights and biases scaled by m so that max_o S_o =
    scale (S_o is linear in W4 and b4).  For scale near PG_SIG2_CAP the other sums (which do not hold W4 twice)
    stay at or below S_o's size and every gene far inside f32's range: max_o S_o alone decides the side."""
    rng = np.random.default_rng(list(shape) + [seed, 7])
    g = rng.standard_normal(genes(shape))
    ws = [w.copy() for w in split(shape, g)]
    ws[-1] *= scale / s_max(shape, g[None])[0]
    return pack(*ws)


def const_net(shape, rng, b4, scale=1.0):
    """Random hidden layers and zero output weights: every output pre-activation is its bias b4 exactly."""
    ws = [w * scale for w in split(shape, rng.standard_normal(genes(shape)))]
    ws[-1][:] = 0.0
    ws[-1][:, -1] = b4
    return pack(*ws)
