"""What the GPU test modules of the kernel families share word for word: moving
genomes to the device, parametrize ids, the comparison of two results field by
field, the oracle comparison of tests/test_gpu_parity.py, the refusal check, and
the drop-in scaffolding (the hall the reference's evaluate() reads, the config
knobs as a user sets them).  A plain module: no tests and no fixtures in it.
Whatever differs between the families -- shapes, built cases, counters,
thresholds -- stays in their own files."""
import contextlib
import importlib
import random

import numpy as np
import pytest
import torch

FIELDS = ("fitness", "rewards", "scores", "frames", "total_frames", "status")


def dev_genomes(a, dev, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)


def gene_count(shape, bias=True):
    b = 1 if bias else 0
    return sum((shape[i] + b) * shape[i + 1] for i in range(len(shape) - 1))


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v).replace("torch.", "")


def same(a, b, n=None, *, what=""):
    """Two results of Evaluator.evaluate are equal in every field (in their first n rows); what: said on failure."""
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x[:n], y[:n]), (name, what) if what else name


# ------------------------------------------------- against the CPU oracle ----
def schedule(rng, n, n_games, n_opp):
    kinds = np.zeros((n, n_games), np.int32)
    for g in range(n_games):
        kinds[:, g] = [0, 1, 2, 3, 3, 3][g % 6]
    flip = rng.random((n, n_games)) < 0.15
    kinds[flip] = 0  # empty-HoF style games
    opp = rng.integers(0, n_opp, size=(n, n_games)).astype(np.int32)
    mult = np.ones((n, n_games))
    hof_games = kinds == 3
    mult[hof_games] = np.round(rng.normal(size=hof_games.sum()), 3)
    return kinds, opp, mult


def run_both(ev, oracle, genomes, opponents, kinds, opp, mult, gpu, **kw):
    dt = ev.dtype
    res, _ = ev.evaluate(dev_genomes(genomes, gpu, dt), torch.tensor(kinds, device=gpu),
                         torch.tensor(opp, device=gpu), torch.tensor(mult, device=gpu),
                         opponents=dev_genomes(opponents, gpu, dt), **kw)
    torch.cuda.synchronize()
    ref = oracle.eval_population(genomes, ev.nodes, kinds, opp, mult, opponents=opponents, bias=ev.bias,
                                 base_seed=ev.seed, n_threads=8)
    return res, ref


def assert_same(res, ref):
    np.testing.assert_array_equal(res.scores.cpu().numpy(), ref["scores"])
    np.testing.assert_array_equal(res.frames.cpu().numpy(), ref["frames"])
    np.testing.assert_array_equal(res.total_frames.cpu().numpy(), ref["total_frames"])
    np.testing.assert_array_equal(res.rewards.cpu().numpy(), ref["rewards"])
    np.testing.assert_array_equal(res.fitness.cpu().numpy(), ref["fitness"])
    np.testing.assert_array_equal(res.status.cpu().numpy(), ref["status"])


# ----------------------------------------------------------------- refusals ----
def refused(fn, word):
    """fn() raises PG_ERR_UNSUPPORTED with word in its message."""
    from pong_amd import _lib
    with pytest.raises(_lib.PongGAError) as e:
        fn()
    assert e.value.code == _lib.PG_ERR_UNSUPPORTED and word in str(e.value), str(e.value)


# -------------------------------------------------------------- the drop-in ----
class Fit:
    def __init__(self, v):
        self.values = (v,)
        self.valid = True


class Member(list):
    def __init__(self, genes, fit):
        super().__init__(genes)
        self.fitness = Fit(fit)


class HoF:
    def __init__(self, items):
        self.items = items


@contextlib.contextmanager
def dropin_config(activation=None, kernel=None):
    """config.ACTIVATION / config.KERNEL as a user sets them (None: left as it
    is): numpy_nn initialises its activation_function from the knob when it is
    imported, so it is reloaded; the kernel knob is read at each call.  Both
    knobs are restored on exit, whatever the test set meanwhile."""
    import config
    import numpy_nn
    saved = (config.ACTIVATION, config.KERNEL)
    if activation is not None:
        config.ACTIVATION = activation
    if kernel is not None:
        config.KERNEL = kernel
    importlib.reload(numpy_nn)
    try:
        yield
    finally:
        config.ACTIVATION, config.KERNEL = saved
        importlib.reload(numpy_nn)


def dropin_fitness(hall, inds):
    """ga.toolbox.map(ga.toolbox.evaluate, inds) against a fresh hall of the rows
    hall, under random.seed(5) (pick_hall_of_famer shuffles the hall in place: a
    fresh one, in the same order, per run)."""
    import ga
    import main
    main.hall_of_fame = HoF([Member(list(g), f) for g, f in zip(hall, (0.7, -0.3, 0.1, 0.0))])
    random.seed(5)
    return [fit[0] for fit in ga.toolbox.map(ga.toolbox.evaluate, inds)]
