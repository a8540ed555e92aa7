#!/usr/bin/env python3
"""Generate the wide ReLU golden vectors from the REAL reference code.

Like make_relu_golden.py: make_golden.py is imported as a module (its shims
are reused, the file itself is untouched) and the reference's one-line
activation switch is thrown at run time (numpy_nn.py:26):
``numpy_nn.activation_function = numpy_nn.ReLU`` (numpy_nn.py:6-9).  Runs only
in the build container, on the CPU; the fixture is data.

relu_forward_wide.npz  NeuralNetwork.run of ReLU networks in k_wide's scope
                   (2 outputs: the reference raises for an argmax index >= 2):
                   [6,100,130,2]  4 genomes, 2 from U[0,1) and 2 from N(0,1),
                                  genes stored (f32-representable f64);
                   [6,512,512,2]  2 genomes (one U[0,1), one N(0,1)), stored as
                                  the generator seed and the sha256 of the f64
                                  gene bytes, as nn_forward_wide.json does:
                                  genes = f32(default_rng(seed).random(G)) for
                                  "init", f32(default_rng(seed).standard_normal(G))
                                  for "n1".
                   32 inputs per network, all on the game's k/320 grid (k: the
                   doubled centroids, stored).  Per pass: k, x = k / 320, the
                   output activations, their argmax, run's result.

Usage:  python tests/golden/make_relu_wide_golden.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

ref_nn = MG.ref_nn
ref_nn.activation_function = ref_nn.ReLU

N_INPUTS = 32


def passes(shape, genomes, rng):
    gidx, ks, xs, acts, idxs, runs = [], [], [], [], [], []
    for gi, g in enumerate(genomes):
        net = ref_nn.NeuralNetwork(nodes=list(shape), weights=list(g), bias=True)
        for _ in range(N_INPUTS):
            k = rng.integers(0, 321, size=6)
            x = [float(v) for v in k / 320.0]
            r = net.run(x)
            a = np.array(net.list_of_transitional_arrays[-1][:-1], dtype=np.float64)
            gidx.append(gi)
            ks.append(k)
            xs.append(x)
            acts.append(a)
            idxs.append(int(np.argmax(a)))
            runs.append([int(v) for v in r])
    zero = int((np.array(acts).max(axis=1) <= 0).sum())
    print(f"forward {shape}: {len(xs)} passes, {zero} with every output <= 0, "
          f"argmax counts {np.bincount(idxs, minlength=2).tolist()}", flush=True)
    return dict(shape=np.array(shape), gidx=np.array(gidx, dtype=np.int32), k=np.array(ks, dtype=np.int32),
                x=np.array(xs), act=np.array(acts), idx=np.array(idxs, dtype=np.int32), run=np.array(runs, dtype=np.int8))


def main():
    out = {}
    rng = np.random.default_rng(20261020)
    shape = [6, 100, 130, 2]
    G = MG.gene_count(shape)
    genomes = [MG.gen_genes(rng, dist, G) for dist in ("init", "init", "n1", "n1")]
    d = passes(shape, genomes, rng)
    d["genes"] = np.array(genomes)
    out["6x100x130x2"] = d

    shape = [6, 512, 512, 2]
    G = MG.gene_count(shape)
    seeds, dists, genomes, shas = [31, 32], ["init", "n1"], [], []
    for seed, dist in zip(seeds, dists):
        g = MG.gen_genes(np.random.default_rng(seed), dist, G)
        genomes.append(g)
        shas.append(hashlib.sha256(g.tobytes()).hexdigest())
    d = passes(shape, genomes, np.random.default_rng(20261021))
    d["seed"] = np.array(seeds)
    d["dist"] = np.array(dists)
    d["genes_sha256"] = np.array(shas)
    out["6x512x512x2"] = d

    path = os.path.join(HERE, "relu_forward_wide.npz")
    np.savez_compressed(path, **{f"{k}__{f}": v for k, dd in out.items() for f, v in dd.items()})
    print(f"{path}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
