#!/usr/bin/env python3
"""Generate the ReLU golden vectors from the REAL reference code.

Like make_golden.py (imported here as a module: its shims, fake env and
hall-of-fame stubs are reused, the file itself is untouched), with the
reference's one-line activation switch thrown (numpy_nn.py:26):
``numpy_nn.activation_function = numpy_nn.ReLU`` (numpy_nn.py:6-9).  Runs only
in the build container, on the CPU; the fixtures are data.

relu_forward.npz   NeuralNetwork.run of [6,2,2], [6,16,2], [6,64,2] and
                   [6,64,64,2] ReLU networks (2 outputs: the reference raises
                   for an argmax index >= 2), 4 genomes from U[0,1) and 4 from
                   N(0,1) per shape, 32 inputs per network (half on the game's
                   k/320 grid): genomes, inputs, run's result, the output
                   activations and their argmax.
relu_evaluate.json evaluate_s3.json's layout: whole evaluate() calls
                   (main.py:28-66) of N(0,1) [6,16,2] and [6,64,2] ReLU
                   individuals against a hall of 3 whose fitness values
                   include a negative one.  Random ReLU networks mostly lose
                   0-3 with equal timing, so individuals are drawn (and kept,
                   in order: evaluate() consumes the hall-of-fame shuffles
                   sequentially) until a case holds at least 6 individuals and
                   3 distinct fitness values.  Draws that took: [6,16,2] 6,
                   [6,64,2] 6 (see the run's printout; each evaluate() takes
                   ~7 s).

Usage:  python tests/golden/make_relu_golden.py [forward] [evaluate]
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

ref_nn = MG.ref_nn
ref_nn.activation_function = ref_nn.ReLU


def gen_forward():
    rng = np.random.default_rng(20261019)
    out = {}
    for shape in ([6, 2, 2], [6, 16, 2], [6, 64, 2], [6, 64, 64, 2]):
        key = "x".join(map(str, shape))
        G = MG.gene_count(shape)
        genes, gidx, xs, acts, idxs, runs = [], [], [], [], [], []
        for dist in ("init", "n1"):
            for _ in range(4):
                g = MG.gen_genes(rng, dist, G)
                genes.append(g)
                net = ref_nn.NeuralNetwork(nodes=list(shape), weights=list(g), bias=True)
                for k in range(32):
                    x = rng.integers(0, 321, size=6) / 320.0 if k % 2 == 0 else rng.random(6)
                    x = [float(v) for v in x]
                    r = net.run(x)
                    a = np.array(net.list_of_transitional_arrays[-1][:-1], dtype=np.float64)
                    gidx.append(len(genes) - 1)
                    xs.append(x)
                    acts.append(a)
                    idxs.append(int(np.argmax(a)))
                    runs.append([int(v) for v in r])
        out[key] = dict(shape=np.array(shape), genes=np.array(genes), gidx=np.array(gidx), x=np.array(xs),
                        act=np.array(acts), idx=np.array(idxs), run=np.array(runs))
        zero = int((np.array(acts).max(axis=1) <= 0).sum())
        print(f"forward {shape}: {len(xs)} passes, {zero} with every output <= 0", flush=True)
    np.savez_compressed(os.path.join(HERE, "relu_forward.npz"),
                        **{f"{k}__{f}": v for k, d in out.items() for f, v in d.items()})


def gen_evaluate(min_inds=6, min_distinct=3, max_draws=20):
    cases = []
    for shape, seed in (([6, 16, 2], 21), ([6, 64, 2], 22)):
        rng = np.random.default_rng(1000 + seed)
        G = MG.gene_count(shape)
        hof_genes = [rng.standard_normal(G) for _ in range(3)]
        hof_fit = [0.8125, -0.6875, 0.25]
        hof = MG._HoF([MG._Ind(list(g), f) for g, f in zip(hof_genes, hof_fit)])
        ns = MG.make_namespace(shape, hall_of_fame=hof)
        random.seed(seed)
        inds, fits = [], []
        while len(inds) < max_draws and (len(inds) < min_inds or len(set(fits)) < min_distinct):
            g = rng.standard_normal(G)
            inds.append(g)
            fits.append(float(ns["evaluate"](list(g))[0]))
            print(f"evaluate relu {shape}: draw {len(inds)} fitness={fits[-1]}", flush=True)
        if len(set(fits)) < min_distinct:
            raise SystemExit(f"{shape}: only {len(set(fits))} distinct fitness values in {max_draws} draws")
        cases.append(dict(shape=shape, random_seed=seed, activation="relu", individuals=[g.tolist() for g in inds],
                          hof_genes=[g.tolist() for g in hof_genes], hof_fitness=hof_fit, fitness=fits, games=[]))
        print(f"evaluate relu {shape}: {len(inds)} draws, {len(set(fits))} distinct fitness values", flush=True)
    with open(os.path.join(HERE, "relu_evaluate.json"), "w") as fh:
        json.dump(cases, fh)


if __name__ == "__main__":
    which = sys.argv[1:] or ["forward", "evaluate"]
    if "forward" in which:
        gen_forward()
    if "evaluate" in which:
        gen_evaluate()
