"""The host model of k_sig2_block's decision (csrc/pg_sig2_block.hip,
pg_block2.hpp; pg_sig2_bound.h under its block layout) in plain numpy, shared by
tests/test_sig2_block_host.py and tests/test_gpu_sig2_block.py.  What does not
depend on the layout comes from tests/_sig2_model.py (the emulated and displaced
sigmoid, numpy_nn's f64 chain, certify's rule) and tests/_relu2_model.py (the
genome layout, the block layout's shapes); here are the block layout's f32 chain
-- one rounded product per thread, group_sum<64>'s tree over each wave, (wave 0 +
wave 1) + bias, padding activations 0.5 on zero weights -- the bound restated
under the block layout's constants, the gcc stand-alone program on the header's
layout-taking functions, and the shared N(0,1) passes."""
import subprocess

import numpy as np

from _relu_model import _fma32
from _relu2_model import BLOCK_SHAPES, genes, pack, split  # noqa: F401
from _sig2_model import (BOUND_HDR, CAP, ETA, SIG, SLOPE, U32, _sig32, certify_np, run64, sigmoid64,  # noqa: F401
                         z64)

P = 128                         # PG_SIG2_BLOCK_MAX_H: threads per network, padded units per hidden layer
CHAIN = (9, 129, 10)            # PG_SIG2_BLOCK_CHAIN1..3
UNDER = (3.0, 72.0, 400.0)      # pg_sig2_layout_block's underflow constants: of max T_o, of max sum_k |W3_ok|, the addend
LANE_CHAIN = (9, 65, 11)        # the lane layout's, for the comparison of the old and the new functions
LANE_UNDER = (2.0, 36.0, 80.0)


def sums(shape, g, chain=CHAIN):
    """The sums of pg_sig2_bound.h for genomes g [.., G] under a layout's chain lengths: S_o (with the output
    bias's share), T_o, sum_k |W3_ok| per output; sum_j A_j, sum_k B_k, sum_k P_k."""
    _, H1, H2, O = shape
    c1, c2, c3 = chain
    w1, w2, w3 = (np.abs(w) for w in split(shape, np.asarray(g, np.float64)))
    with np.errstate(all="ignore"):
        A = w1.sum(axis=-1)
        W = w2[..., :H1].sum(axis=-1)
        Pk = np.einsum("...kj,...j->...k", w2[..., :H1], A)
        B = W + w2[..., H1]
        Q = (SLOPE * c1) * Pk + (SIG + c2) * B
        t = SLOPE * Q + (SIG + c3)
        S = np.einsum("...ok,...k->...o", w3[..., :H2], t) + c3 * w3[..., H2]
        T = np.einsum("...ok,...k->...o", w3[..., :H2], W)
        return S, T, w3[..., :H2].sum(axis=-1), A.sum(axis=-1), B.sum(axis=-1), Pk.sum(axis=-1)


def bound_np(shape, g, chain=CHAIN, under=UNDER):
    """pg_sig2_bound_genome_l restated: e = (u max_o S_o + eta (under_t max_o T_o + under_w3 max_o sum_k |W3_ok| +
    under_c)) (1 + 2^-10) as f32, inf when a sum exceeds the cap or is not a number."""
    S, T, W3, a, b, p = sums(shape, g, chain)
    with np.errstate(all="ignore"):
        ok = (a <= CAP) & (b <= CAP) & (p <= CAP) & (S <= CAP).all(axis=-1) & (T <= CAP).all(axis=-1) & \
            (W3 <= CAP).all(axis=-1)
        e = (U32 * S.max(axis=-1) + ETA * (under[0] * T.max(axis=-1) + under[1] * W3.max(axis=-1) + under[2])) * \
            (1.0 + 2.0 ** -10)
        return np.where(ok, e, np.inf).astype(np.float32)


def bound_strings(tmp_path, which, shape, nets):
    """The %a strings a stand-alone gcc program prints for each genome of nets [N, G]: which = "block" / "lanes":
    pg_sig2_bound_genome_l under that layout; "old": pg_sig2_bound_genome, the lane layout's earlier entry.
    (exit status 2: one of the header's macros or layout fields is not what this module says)"""
    exe = tmp_path / "bsb"
    if not exe.exists():
        src = tmp_path / "bsb.c"
        pins = (f"PG_SIG2_BLOCK_CHAIN1 != {CHAIN[0]} || PG_SIG2_BLOCK_CHAIN2 != {CHAIN[1]} || "
                f"PG_SIG2_BLOCK_CHAIN3 != {CHAIN[2]} || PG_SIG2_BLOCK_MAX_H != {P} || PG_SIG2_SIG != 4.5 || "
                "PG_SIG2_SLOPE != 0.25 || PG_SIG2_CAP != 1e25 || PG_SIG2_CHAIN1 != 9 || PG_SIG2_CHAIN2 != 65 || "
                "PG_SIG2_CHAIN3 != 11 || PG_SIG2_MAX_H != 64")
        src.write_text(f'#include <stdio.h>\n#include <stdlib.h>\n#include <string.h>\n#include "{BOUND_HDR}"\n'
                       "int main(int argc, char **argv){ FILE *f = fopen(argv[2], \"rb\"); int hdr[4];\n"
                       " const pg_sig2_layout b = pg_sig2_layout_block(), n = pg_sig2_layout_lanes();\n"
                       f" if ({pins}) return 2;\n"
                       f" if (b.chain1 != {CHAIN[0]} || b.chain2 != {CHAIN[1]} || b.chain3 != {CHAIN[2]} || b.max_h != {P} ||\n"
                       f"     b.under_t != {UNDER[0]} || b.under_w3 != {UNDER[1]} || b.under_c != {UNDER[2]}) return 2;\n"
                       f" if (n.chain1 != 9 || n.chain2 != 65 || n.chain3 != 11 || n.max_h != 64 ||\n"
                       f"     n.under_t != {LANE_UNDER[0]} || n.under_w3 != {LANE_UNDER[1]} || n.under_c != {LANE_UNDER[2]}) return 2;\n"
                       " while (fread(hdr, sizeof(int), 4, f) == 4) { int H1 = hdr[0], H2 = hdr[1], O = hdr[2];\n"
                       "  size_t G = (size_t)hdr[3]; double *g = malloc(G * sizeof(double)); float e;\n"
                       "  if (fread(g, sizeof(double), G, f) != G) return 1;\n"
                       "  if (!strcmp(argv[1], \"old\")) e = pg_sig2_bound_genome(g, H1, H2, O);\n"
                       "  else e = pg_sig2_bound_genome_l(strcmp(argv[1], \"block\") ? n : b, g, H1, H2, O);\n"
                       "  printf(\"%a\\n\", (double)e); free(g); }\n"
                       " return 0; }\n")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])
    data = tmp_path / "nets_sb.bin"
    nets = np.atleast_2d(np.ascontiguousarray(nets, np.float64))
    assert nets.shape[1] == genes(shape)
    with open(data, "wb") as fh:
        for g in nets:
            fh.write(np.array([shape[1], shape[2], shape[3], len(g)], np.int32).tobytes())
            fh.write(g.tobytes())
    return subprocess.run([str(exe), which, str(data)], capture_output=True, text=True, check=True).stdout.split()


def bounds(tmp_path, shape, nets, which="block"):
    """pg_sig2_bound_genome_l under the block layout (or `which`) of each genome of nets [N, G], as f32."""
    return np.array([float.fromhex(v) for v in bound_strings(tmp_path, which, shape, nets)]).astype(np.float32)


def z32(shape, g, k, out=None, sign=0.0):
    """k_sig2_block's f32 chain (pg_block2.hpp block_z32, block_z_out) for genomes g [N, G] on doubled centroids
    k [N, m, 6] -> [N, m, O]: layer 1 as six fmas onto the bias; layer 2 one fma per padded layer-1 unit, 128 of
    them in ascending order, onto the bias; layer 3 one product per thread, f32 x f32 rounded once, the tree of
    group_sum<64> over each wave's 64 lanes (every step adds the same two operands in both partner lanes), then
    wave 0's sum + wave 1's, then the output bias.  Padding units have activation 0.5 and zero outgoing weights.
    sign, out: tests/_sig2_model.py's displacement of every sigmoid by the full 4.5 u."""
    _, H1, H2, O = shape
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
        w3p = np.zeros((N, O, P), np.float32)
        w3p[:, :, :H2] = w3[:, :, :H2]
        z = np.empty((N, m, O), np.float32)
        for o in range(O):
            acc = w3p[:, None, o, :] * h2
            assert acc.dtype == np.float32
            while acc.shape[2] > 1:
                acc = acc[:, :, 0::2] + acc[:, :, 1::2]
            z[:, :, o] = acc[:, :, 0] + w3[:, None, o, H2]
    return z


def n01_passes(shape, dtype_f32=False):
    """The N(0, 1) networks and inputs on which the host and the GPU test compare the certificate's share:
    32 genomes [32, G], doubled centroids [32, 64, 6]."""
    rng = np.random.default_rng([12] + list(shape))
    g = rng.standard_normal((32, genes(shape)))
    if dtype_f32:
        g = g.astype(np.float32).astype(np.float64)
    return g, rng.integers(0, 321, size=(32, 64, 6))


def host_share(shape, dtype_f32=False):
    """The share of n01_passes the restated certificate decides on the emulated chain."""
    g, k = n01_passes(shape, dtype_f32)
    return float(certify_np(z32(shape, g, k), bound_np(shape, g)[:, None]).mean())
