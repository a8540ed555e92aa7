"""Measure Evaluator.evaluate alone on ReLU networks: k_relu against the general
kernel (the only other way to run the workload), and the sigmoid k_service on
the same genomes for context; also the two-hidden-layer sigmoid k_sig2 against
the general and the wide kernel.  One JSON line per run.

Workload: [6,64,3] networks, 6 self-play games per genome against a hall of
pop // 4, genes N(0, 3) drawn as bench.py's default workload draws them
(torch.randn from a device generator seeded with 1234 for the population and
1235 for the hall, f64).  Each launch is timed between two device events on a
quiet stream after warm-up launches; the median and the spread (min, max, the
interquartile range) of >= 20 launches are reported.

    python tools/bench_relu.py                      # the four runs
    python tools/bench_relu.py --runs relu:4096 general:4096 --launches 30
    python tools/bench_relu.py --shape 6 64 64 3 --runs relu2:4096 general:4096   # k_relu2
    python tools/bench_relu.py --shape 6 128 128 3 --dtype float32 --launches 5 \
        --runs relu2_block:4096 relu_wide:4096 general:4096   # k_relu2_block
    python tools/bench_relu.py --shape 6 32 32 32 3 --dtype float32 \
        --runs relu3:65536 general:65536 relu3:65536 general:65536                # k_relu3
    python tools/bench_relu.py --shape 6 32 32 32 3 --activation sigmoid --dtype float32 \
        --runs sig3:65536 general:65536 sig3:65536 general:65536                  # k_sig3
    python tools/bench_relu.py --shape 6 128 128 3 --activation sigmoid --dtype float32 --launches 5 \
        --runs sig2_block:4096 wide:4096 general:4096         # k_sig2_block
    python tools/bench_relu.py --shape 6 512 512 3 --dtype float32 --launches 5 \
        --runs relu_wide:4096 general:4096                                        # k_wide's ReLU instances (4.2e)
    python tools/bench_relu.py --shape 6 64 64 3 --activation sigmoid \
        --runs sig2:4096 general:4096 wide:4096                                   # k_sig2
    python tools/bench_relu.py --runs relu:4096 relu+advance:4096 relu:4096 relu+advance:4096   # the closed-form
        # frame advance against its base kernel, alternating; relu2+advance and sig2+advance alike
    python tools/bench_relu.py --schedule reference --runs relu:4096 relu+solo:4096 relu:4096 relu+solo:4096
        # scripted-opponent games on half a lane group against the base kernel; relu2+solo,
        # sig2+solo and X+advance+solo against X+advance alike
    python tools/bench_relu.py --activation sigmoid --schedule reference \
        --runs auto:65536 auto+solo:65536 auto:65536 auto+solo:65536              # k_service's solo instance (4.2j)

--schedule: selfplay (the default: every game against a hall member), reference
(evaluate()'s kinds [0,1,2,3,3,3] per genome, the NN games against the same
hall) or scripted (generation 0's [0,1,2,0,0,0]: no hall yet).  When the runs
hold X and X+solo (or X+advance and X+advance+solo) at one population, their
fitness, rewards, scores and frames on the timed inputs are asserted equal.

Every run reports rally_share and serve_delay_share: counters [8] and [12] as
shares of the episode frames (0 for a kernel that steps every frame).

--activation sets the activation of the general and wide runs (default relu;
relu, relu2, relu3, relu2_block and relu_wide runs are always ReLU, sig2, sig3, sig2_block and service runs always
sigmoid; a five-node --shape with --activation sigmoid is what sig3 and its general runs take).  --genes uniform draws U[0, 1) genes (generation 0 of a reference
run, ga.py:85) instead of N(0, 3).

relu_wide runs also report the network passes (counter [7]) and the streaming
rate passes x gene bytes / launch time, as bench.py --config wide does for the
sigmoid k_wide.  --dtype is the genome storage type (default float64, the 4.2c
workload; float32 draws the same N(0, 3) genes in f32, BASELINE config 5's storage).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "neuro-genetic-pong-self-play_amd"))

from pong_amd.device import Evaluator  # noqa: E402

SHAPE = [6, 64, 3]
RUNS = ["relu:4096", "general:4096", "relu:65536", "service:65536"]


def workload(pop, dev, seed=1234, sigma=3.0, shape=SHAPE, dtype=torch.float64, genes="normal"):
    G = sum((shape[i] + 1) * shape[i + 1] for i in range(len(shape) - 1))
    if genes == "uniform":
        return tuple(torch.rand((n, G), generator=torch.Generator(device=dev).manual_seed(sd), dtype=dtype, device=dev)
                     for n, sd in ((pop, seed), (max(pop // 4, 1), seed + 1)))
    genomes = torch.randn((pop, G), generator=torch.Generator(device=dev).manual_seed(seed), dtype=dtype,
                          device=dev).mul_(sigma)
    hall = torch.randn((max(pop // 4, 1), G), generator=torch.Generator(device=dev).manual_seed(seed + 1),
                       dtype=dtype, device=dev).mul_(sigma)
    return genomes, hall


KERNEL_NAMES = {"relu": "k_relu", "relu2": "k_relu2", "relu3": "k_relu3", "relu2_block": "k_relu2_block", "sig2_block": "k_sig2_block", "relu_wide": "k_wide<relu>", "general": "k_general",
                "service": "k_service", "sig2": "k_sig2", "sig3": "k_sig3", "wide": "k_wide", "auto": "auto"}
FIXED_ACTIVATION = {"relu": "relu", "relu2": "relu", "relu3": "relu", "relu2_block": "relu", "relu_wide": "relu", "service": "sigmoid", "sig2": "sigmoid", "sig2_block": "sigmoid", "sig3": "sigmoid",
                    "wide": "sigmoid"}
# the names "+advance" and "+solo" go with (pong_amd.device.kernel_code); auto runs the network of --activation on
# what PG_KERNEL_AUTO picks and reports it as Evaluator.resolved_kernel does: "auto+solo" with --activation sigmoid
# --shape 6 64 3 is k_service's solo instance
MODIFIED = ("relu", "relu2", "sig2", "auto", "relu3", "sig3")
SCHEDULES = {"selfplay": None, "reference": [0, 1, 2, 3, 3, 3], "scripted": [0, 1, 2, 0, 0, 0]}


def split_name(name):
    """(base, modifiers) of a run's kernel name, e.g. "relu+advance+solo"; None if it is not one."""
    base, *mods = name.split("+")
    ok = base in KERNEL_NAMES and set(mods) <= {"advance", "solo"} and len(set(mods)) == len(mods)
    return (base, frozenset(mods)) if ok and (not mods or base in MODIFIED) else None


def schedule(ev, pop, hall, kinds):
    """The launch's (kind, opp, mult): the self-play schedule's opponents under the per-genome kinds."""
    kind, opp, mult = ev.selfplay_schedule(pop, hall.shape[0])
    if kinds is not None:
        kind = torch.tensor(kinds, dtype=torch.int32, device=kind.device).repeat(pop, 1)
    return kind, opp, mult


def run(name, pop, dev, warmup, launches, shape=SHAPE, dtype=torch.float64, activation="relu", genes="normal",
        kinds=None, keep=None):
    base, mods = split_name(name)
    activation = FIXED_ACTIVATION.get(base, activation)
    kernel = "split" if name == "service" else name
    ev = Evaluator(shape, device=dev, dtype=dtype, activation=activation, kernel=kernel,
                   precision="f64" if name == "general" else "certified")
    genomes, hall = workload(pop, dev, shape=shape, dtype=dtype, genes=genes)
    sched = schedule(ev, pop, hall, kinds)
    if kinds is not None and 3 not in kinds:
        hall = None  # generation 0: no hall of fame yet
    res = None
    for _ in range(warmup):
        res, _ = ev.evaluate(genomes, *sched, opponents=hall, out=res, validate=False)
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res, _ = ev.evaluate(genomes, *sched, opponents=hall, out=res, validate=False)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    c = res.counters.cpu().numpy()
    ms = np.array(ms)
    med = float(np.median(ms))
    q1, q3 = np.percentile(ms, [25, 75])
    frames = int(res.frames.sum())
    if keep is not None:  # the timed inputs' results, for the untimed X against X+solo comparison
        keep[(base, mods, pop)] = [getattr(res, f).clone() for f in ("fitness", "rewards", "scores", "frames")]
    kernel_name = KERNEL_NAMES[base] + ("_adv" if "advance" in mods else "") + ("_solo" if "solo" in mods else "")
    if base == "auto":
        kernel_name = "auto: " + ev.resolved_kernel()
    out = {"kernel": kernel_name, "schedule": "selfplay" if kinds is None else kinds, "genome_dtype": str(dtype).replace("torch.", ""),
            "activation": activation, "shape": list(shape), "pop": pop, "games": 6, "hall": int(hall.shape[0]) if hall is not None else 0,
            "launches": launches, "warmup": warmup,
            "ms_median": round(med, 4), "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4),
            "ms_iqr": round(float(q3 - q1), 4), "stepped_env_steps": int(c[0]), "episode_frames": frames,
            "stepped_env_steps_per_s": round(int(c[0]) / (med * 1e-3), 1), "forwards": int(c[1]),
            "f64_forwards": int(c[2]), "f64_share": round(int(c[2]) / max(int(c[1]), 1), 6),
            # the episode frames not stepped one at a time: periodic rallies jumped [8], serve delays advanced [12]
            "rally_share": round(int(c[8]) / max(frames, 1), 6), "serve_delay_share": round(int(c[12]) / max(frames, 1), 6),
            "genes": "U[0,1)" if genes == "uniform" else "N(0,3)",
            "device": torch.cuda.get_device_name(dev)}
    if name.startswith(("sig2", "sig3")):  # the cascade: forwards the f32 certificate left undecided (counter [4])
        out["stage1_failures"] = int(c[4])
        out["stage1_failure_share"] = round(int(c[4]) / max(int(c[1]), 1), 6)
    if name == "relu_wide":  # each network pass streams one network's genes once
        gene_bytes = ev.genes * genomes.element_size()
        out["network_passes"] = int(c[7])
        out["rally_frames_advanced"] = int(c[8])
        out["stream_TB_per_s"] = round(int(c[7]) * gene_bytes / (med * 1e-3) / 1e12, 3)
        out["stream_TB_per_s_min_max"] = [round(int(c[7]) * gene_bytes / (float(t) * 1e-3) / 1e12, 3) for t in (ms.max(), ms.min())]
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--runs", nargs="*", default=RUNS, help="kernel:population, kernel in relu, relu2, relu3, relu2_block, relu_wide, sig2, sig3, sig2_block, wide, general, service, auto, "
                   "relu+advance, relu2+advance, relu3+advance, sig2+advance, sig3+advance, auto+advance, and relu, relu2, relu3, sig2, sig3, auto with +solo or "
                   "+advance+solo")
    p.add_argument("--schedule", default="selfplay", choices=sorted(SCHEDULES),
                   help="the games' kinds per genome: selfplay (all against the hall), reference ([0,1,2,3,3,3]) or "
                   "scripted (generation 0: [0,1,2,0,0,0], no hall)")
    p.add_argument("--shape", nargs="+", type=int, default=SHAPE,
                   help="NETWORK_SHAPE (default 6 64 3; relu2 needs two hidden layers, e.g. 6 64 64 3)")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--launches", type=int, default=20, help="timed launches (>= 20; >= 5 for layers wider than 256, or wider than 64 with general, relu_wide or wide among the runs)")
    p.add_argument("--dtype", default="float64", choices=["float64", "float32"], help="genome storage type")
    p.add_argument("--activation", default="relu", choices=["relu", "sigmoid"],
                   help="activation of the general runs (the other kernels have one activation each)")
    p.add_argument("--genes", default="normal", choices=["normal", "uniform"], help="N(0, 3) genes or U[0, 1)")
    args = p.parse_args()
    # seconds per launch: any kernel above 256 units a layer; above 64, the general and the wide kernels
    bases = {spec.split(":")[0].split("+")[0] for spec in args.runs}
    width = max(args.shape[1:-1])
    slow = width > 256 or (width > 64 and bases & {"general", "relu_wide", "wide"})
    if args.launches < (5 if slow else 20):
        p.error("--launches must be >= 20 (>= 5 for layers wider than 256, and for layers wider than 64 when the "
                "runs hold general, relu_wide or wide: seconds per launch)")
    dev = torch.device("cuda", torch.cuda.current_device())
    keep = {}
    for spec in args.runs:
        name, pop = spec.split(":")
        if split_name(name) is None:
            p.error(f"unknown kernel {name!r}")
        print(json.dumps(run(name, int(pop), dev, args.warmup, args.launches, args.shape,
                             getattr(torch, args.dtype), args.activation, args.genes, SCHEDULES[args.schedule], keep)),
              flush=True)
    for (base, mods, pop), got in keep.items():  # X+solo against X, X+advance+solo against X+advance
        if "solo" in mods:
            want = keep.get((base, mods - {"solo"}, pop))
            for a, b in zip(got, want or ()):
                assert torch.equal(a, b), f"{base}+{'+'.join(sorted(mods))}:{pop} differs from its base kernel's results"


if __name__ == "__main__":
    main()
