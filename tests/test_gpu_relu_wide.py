"""PG_KERNEL_RELU_WIDE on the MI355X (run with -m gpu): k_wide's ReLU instances
(csrc/pg_wide.hip, k_wide<NG, WT, PG_ACT_RELU>) on [6, 2..512, 2..512, 2..4]
ReLU networks; pg_relu_wide_decide pins single frames.

Checkers, none of them the code under test: the reference's own numbers
(tests/golden/relu_forward_wide.npz, written by make_relu_wide_golden.py),
pg_forward in f64 for single decisions, and the general kernel with ReLU for
whole games (tests/test_gpu_relu.py pins it to the reference's numpy loop).
No transcendental is involved, so every comparison is exact (activations bit
for bit, up to the sign of zero)."""
import hashlib

import numpy as np
import pytest
import torch

from _gpu_support import FIELDS, dev_genomes, dropin_config, dropin_fitness, gene_count, ids, refused, same
from test_gpu_wide import _schedule

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]


def _relu_ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, activation="relu", **kw)


def _bits(a):
    """f64 bit patterns with -0 mapped to +0."""
    return (np.asarray(a, dtype=np.float64) + 0.0).view(np.int64)


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


# ------------------------------------------------- 1 the reference's numbers ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("key", ["6x100x130x2", "6x512x512x2"])
def test_decide_equals_reference(gpu, golden, key, dtype):
    """NeuralNetwork.run of the reference with ReLU on the game's k/320 grid:
    the argmax, and the output activations as f64 bit patterns.  [6,100,130,2]:
    4 tiles of 32 f32 (7 of 16 f64) columns, the last one partial, and a
    1-weight tail; [6,512,512,2]: 16 (32) full tiles and the same tail.  The
    genes are f32 values, so both genome storage types hold the same networks."""
    g = golden("relu_forward_wide.npz")
    shape = [int(v) for v in g[f"{key}__shape"]]
    if f"{key}__genes" in g:
        genes = g[f"{key}__genes"]
    else:
        rows = []
        for seed, dist, sha in zip(g[f"{key}__seed"], g[f"{key}__dist"], g[f"{key}__genes_sha256"]):
            rng = np.random.default_rng(int(seed))
            row = _f32(rng.random(gene_count(shape)) if str(dist) == "init" else rng.standard_normal(gene_count(shape)))
            assert hashlib.sha256(row.tobytes()).hexdigest() == str(sha)
            rows.append(row)
        genes = np.array(rows)
    np.testing.assert_array_equal(_f32(genes), genes)
    ev = _relu_ev(shape, gpu, dtype=dtype)
    index, act = ev.relu_wide_decide(dev_genomes(genes, gpu, dtype), torch.tensor(g[f"{key}__k"].astype(np.int32), device=gpu),
                                     genome_index=torch.tensor(g[f"{key}__gidx"].astype(np.int32), device=gpu))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(index.cpu().numpy(), g[f"{key}__idx"])
    np.testing.assert_array_equal(_bits(act.cpu().numpy()), _bits(g[f"{key}__act"]))


# ------------------------------------------- 2 random and extreme passes ----
_PASS_NETS = [([6, 100, 130, 4], torch.float32, True), ([6, 40, 24, 2], torch.float64, False),
              ([6, 100, 130, 4], torch.float32, False), ([6, 40, 24, 2], torch.float64, True)]


# (1e150 is not an f32 value: the f64-storage networks carry that case)
@pytest.mark.parametrize("shape,dtype,bias,genes", [
    (s, d, b, g) for s, d, b in _PASS_NETS for g in ("n1", "init", "n1e150", "zero") if g != "n1e150" or d == torch.float64],
    ids=ids)
def test_decide_equals_f64_forward(gpu, shape, dtype, bias, genes):
    """16 networks x 128 inputs: index and activations equal pg_forward's f64
    path exactly -- N(0,1) and U[0,1) genes, N(0,1) * 1e150 (f64 storage only:
    inf and NaN territory, np.argmax takes the first NaN) and the all-zero
    genome (index 0, every activation 0)."""
    rng = np.random.default_rng(sum(shape) + len(genes) + int(bias))
    G = gene_count(shape, bias)
    w = {"n1": lambda: rng.standard_normal((16, G)), "init": lambda: rng.random((16, G)),
         "n1e150": lambda: rng.standard_normal((16, G)) * 1e150, "zero": lambda: np.zeros((16, G))}[genes]()
    if dtype == torch.float32:
        w = _f32(w)
    k = rng.integers(0, 321, size=(16 * 128, 6)).astype(np.int32)
    gidx = np.repeat(np.arange(16), 128).astype(np.int32)
    ev = _relu_ev(shape, gpu, dtype=dtype, bias=bias)
    gt, kt, it = dev_genomes(w, gpu, dtype), torch.tensor(k, device=gpu), torch.tensor(gidx, device=gpu)
    index, act = ev.relu_wide_decide(gt, kt, genome_index=it)
    ref_idx, ref_act = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64")
    torch.cuda.synchronize()
    index, act, ref_idx, ref_act = (t.cpu().numpy() for t in (index, act, ref_idx, ref_act))
    np.testing.assert_array_equal(index, ref_idx)
    np.testing.assert_array_equal(np.isnan(act), np.isnan(ref_act))
    fin = ~np.isnan(act)
    np.testing.assert_array_equal(_bits(act[fin]), _bits(ref_act[fin]))
    if genes == "zero":
        assert (index == 0).all() and (act == 0).all()
    if genes == "n1e150":
        assert np.isnan(act).any()
        print(f"{shape} bias {bias}: {int(np.isnan(act).any(axis=1).sum())} of {len(act)} passes with a NaN output, "
              f"{int((np.isnan(act).any(axis=1) & ~np.isnan(act).all(axis=1)).sum())} with only some, "
              f"{int(np.isinf(act).any(axis=1).sum())} with an inf")
        first_nan = np.where(np.isnan(act).any(axis=1), np.isnan(act).argmax(axis=1), -1)
        assert (index[first_nan >= 0] == first_nan[first_nan >= 0]).all()
    if genes == "n1":
        assert len(np.unique(index)) >= 2


# -------------------------------------- 3 whole games, traced, vs k_general ----
def _traced_case(n_games):
    """13 genomes and 4 opponents of [6,96,80,3], mixed opponent kinds with 80 %
    NN.  Random ReLU networks can decide one index for ever (every output <= 0
    is index 0); with N(0,1) genes and these seeds the general kernel's traces
    show both directions in 77 %, 56 % and 80 % of the games (n_games 1, 6, 7),
    which the test asserts again from the general kernel's trace alone."""
    shape = [6, 96, 80, 3]
    rng = np.random.default_rng(300 + n_games)
    G = gene_count(shape)
    n, H = 13, 4
    genomes, opponents = rng.standard_normal((n, G)), rng.standard_normal((H, G))
    kinds, opp, mult = _schedule(rng, n, n_games, H, nn_frac=0.8)
    return shape, genomes, opponents, kinds, opp, mult


def _variety(trace, frames):
    """Share of traced games whose right paddle's codes include both 1 and 2."""
    tr = trace.cpu().numpy() & 3
    return np.mean([(1 in set(t[:f])) and (2 in set(t[:f])) for t, f in zip(tr, frames.cpu().numpy().ravel())])


@pytest.mark.parametrize("n_games", [1, 6, 7])
def test_relu_wide_equals_general_with_traces(gpu, n_games):
    """f64 genomes (NG = 4): one chunk, two chunks of 3, balanced chunks of 4 + 3.
    Every game traced: all six output arrays, both paddles' per-frame actions
    and counters[1:4] equal the general kernel's; tracing disables the rally
    jump; no certificate counters; the network passes are counted."""
    shape, genomes, opponents, kinds, opp, mult = _traced_case(n_games)
    n = len(genomes)
    ev = _relu_ev(shape, gpu, n_games=n_games)
    cap = 3000
    args = (dev_genomes(genomes, gpu), torch.tensor(kinds, device=gpu), torch.tensor(opp, device=gpu),
            torch.tensor(mult, device=gpu))
    kw = dict(opponents=dev_genomes(opponents, gpu), trace_games=n * n_games, trace_cap=cap)
    rg, tg = ev.evaluate(*args, kernel="general", **kw)
    rw, tw = ev.evaluate(*args, kernel="relu_wide", **kw)
    torch.cuda.synchronize()
    # the variety condition, from the general kernel's trace alone
    variety = _variety(tg, rg.frames.clamp(max=cap))
    print(f"n_games {n_games}: {variety:.3f} of {n * n_games} traced games move the right paddle both ways")
    assert variety >= 0.25
    same(rw, rg)
    assert torch.equal(tw, tg) and int(tw.any())
    c = rw.counters.cpu().numpy()
    assert torch.equal(rw.counters[1:4], rg.counters[1:4])
    assert c[3] == n * n_games and c[8] == 0 and c[2] == 0 and c[4] == 0 and c[7] > 0
    assert c[0] == int(rg.frames.sum())


# --------------------- 4 every instance and edge layout, untraced, vs k_general ----
@pytest.mark.parametrize("shape,bias,dtype,precision", [
    ([6, 16, 8, 3], True, torch.float64, "certified"),
    ([6, 40, 24, 2], True, torch.float32, "certified"),
    ([6, 64, 64, 3], False, torch.float64, "certified"),
    ([6, 100, 130, 4], True, torch.float32, "certified"),
    ([6, 65, 64, 3], True, torch.float32, "certified"),   # the first shape past k_relu2
    ([6, 64, 64, 3], True, torch.float64, "f64"),
], ids=ids)
def test_relu_wide_layouts_equal_general(gpu, shape, bias, dtype, precision):
    rng = np.random.default_rng(sum(shape) + 7)
    G = gene_count(shape, bias)
    n, H = 21, 5
    genomes, opponents = rng.standard_normal((n, G)) * 2.0, rng.standard_normal((H, G)) * 2.0
    genomes[::3] = rng.random((len(genomes[::3]), G))
    kinds, opp, mult = _schedule(rng, n, 6, H)
    ev = _relu_ev(shape, gpu, bias=bias, dtype=dtype, precision=precision, timeout_thresh=119, win_score=1)
    args = (dev_genomes(genomes, gpu, dtype), torch.tensor(kinds, device=gpu), torch.tensor(opp, device=gpu),
            torch.tensor(mult, device=gpu))
    rw, _ = ev.evaluate(*args, opponents=dev_genomes(opponents, gpu, dtype), kernel="relu_wide")
    rg, _ = ev.evaluate(*args, opponents=dev_genomes(opponents, gpu, dtype), kernel="general")
    torch.cuda.synchronize()
    same(rw, rg)
    c = rw.counters.cpu().numpy()
    assert c[0] + c[8] == int(rw.frames.sum()) and c[3] == n * 6 and c[1] == int(rg.counters[1])
    assert c[2] == 0 and c[4] == 0 and c[7] > 0


# ------------------------------------------------- 5 default-limit games ----
def test_relu_wide_selfplay_default_limits(gpu):
    """64 f32 genomes on the self-play schedule against 16 rows at the default
    limits (TIMEOUT_THRESH 2000, WIN_SCORE 3): the general kernel's results,
    and permutation-equivariant (a genome's result does not depend on which
    workgroup or slot evaluated it)."""
    shape = [6, 96, 80, 3]
    G = gene_count(shape)
    n, H = 64, 16
    gen = torch.Generator(device=gpu).manual_seed(11)
    genomes = torch.randn((n, G), generator=gen, dtype=torch.float32, device=gpu)
    genomes[::2] = torch.rand((n // 2, G), generator=gen, dtype=torch.float32, device=gpu)
    opponents = genomes[:H].contiguous()
    ev = _relu_ev(shape, gpu, dtype=torch.float32, kernel="relu_wide")
    kind, opp, mult = ev.selfplay_schedule(n, H)
    r1, _ = ev.evaluate(genomes, kind, opp, mult, opponents=opponents)
    rg, _ = ev.evaluate(genomes, kind, opp, mult, opponents=opponents, kernel="general")
    perm = torch.randperm(n, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    r2, _ = ev.evaluate(genomes[perm].contiguous(), kind[perm].contiguous(), opp[perm].contiguous(),
                        mult[perm].contiguous(), opponents=opponents)
    torch.cuda.synchronize()
    same(r1, rg)
    for name in FIELDS:
        assert torch.equal(getattr(r2, name), getattr(r1, name)[perm]), name
    c = r1.counters.cpu().numpy()
    assert c[3] == n * 6 and c[0] + c[8] == int(r1.frames.sum())
    print(f"default limits: {int(c[0])} stepped frames, counters[8] = {int(c[8])} frames of periodic rallies advanced at once")


# ------------------------------------------------------ 6 config 5's shape ----
def test_relu_wide_config5_shape_equals_general(gpu):
    shape = [6, 512, 512, 3]
    rng = np.random.default_rng(512)
    G = gene_count(shape)
    n, H = 3, 2
    genomes, opponents = _f32(rng.standard_normal((n, G)) * 3.0), _f32(rng.standard_normal((H, G)) * 3.0)
    kinds = np.array([[0, 1, 2, 3, 3, 3], [3, 3, 3, 3, 3, 3], [3, 0, 3, 1, 3, 2]], np.int32)
    opp = rng.integers(0, H, size=(n, 6)).astype(np.int32)
    mult = np.ones((n, 6))
    ev = _relu_ev(shape, gpu, dtype=torch.float32, timeout_thresh=119, win_score=1)
    args = (dev_genomes(genomes, gpu, torch.float32), torch.tensor(kinds, device=gpu), torch.tensor(opp, device=gpu),
            torch.tensor(mult, device=gpu))
    rw, _ = ev.evaluate(*args, opponents=dev_genomes(opponents, gpu, torch.float32), kernel="relu_wide")
    rg, _ = ev.evaluate(*args, opponents=dev_genomes(opponents, gpu, torch.float32), kernel="general")
    torch.cuda.synchronize()
    same(rw, rg)
    assert int(rw.counters[3]) == n * 6 and int(rw.counters[1]) == int(rg.counters[1]) and int(rw.counters[7]) > 0


# ------------------------------------------------------------ 7 refusals ----
def test_unsupported_combinations_are_refused(gpu):
    from pong_amd.device import Evaluator
    shape = [6, 96, 80, 3]
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    def genomes(ev):
        return torch.zeros((4, ev.genes), dtype=torch.float64, device=gpu)

    ev = _relu_ev(shape, gpu)
    g = genomes(ev)
    sig = Evaluator(shape, device=gpu)
    refused(lambda: sig.evaluate(g, z, z, m, kernel="relu_wide"), "sigmoid")
    refused(lambda: sig.relu_wide_decide(g, k), "PG_ACT_RELU")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu_wide", horizon=1000), "horizon")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu_wide", hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)),
            "hard")
    eo = _relu_ev([6, 64, 3], gpu)
    refused(lambda: eo.evaluate(genomes(eo), z, z, m, kernel="relu_wide"), "relu_wide")
    # the general ReLU refusals stay
    refused(lambda: ev.evaluate(g, z, z, m, kernel="wide"), "relu")
    refused(lambda: ev.wide_decide(g, k), "relu")
    # the supported neighbours of the refused calls still run
    for kernel in ("relu_wide", "auto", "general"):
        res, _ = ev.evaluate(g, z, z, m, kernel=kernel)
        assert int(res.counters[3]) == 24
        assert (int(res.counters[7]) > 0) == (kernel == "relu_wide")  # AUTO is still the general kernel
    index, act = ev.relu_wide_decide(g, k)
    assert (index.cpu().numpy() == 0).all() and (act.cpu().numpy() == 0).all()
    index, _ = sig.wide_decide(g, k)  # the sigmoid probe is untouched: all-zero genes tie at 0.5, index 0
    assert (index.cpu().numpy() == 0).all()


# ------------------------------------------------- 8 DeviceGA, the drop-in ----
def test_device_ga_relu_wide_generations_and_checkpoint(gpu, tmp_path):
    from pong_amd import checkpoint
    from pong_amd.evolve import DeviceGA
    shape = [6, 72, 40, 3]
    runs = {}
    for kernel in ("relu_wide", "general"):
        ga = DeviceGA(shape, 64, device=gpu, seed=9, activation="relu", kernel=kernel)
        assert ga.ev.kernel == kernel and ga.ev.activation == "relu"
        ga.initialize("normal", 1.0)
        history = [ga.step() for _ in range(3)]
        torch.cuda.synchronize()
        runs[kernel] = (ga, history, ga.hall_of_fame.clone(), ga.hof_member_fitness)
    (ga, hist, hall, hall_fit), (_, hist_g, hall_g, hall_fit_g) = runs["relu_wide"], runs["general"]
    assert hist == hist_g
    assert torch.equal(hall, hall_g) and np.array_equal(hall_fit, hall_fit_g)
    assert torch.equal(runs["relu_wide"][0].fitness, runs["general"][0].fitness)
    assert int(ga.last.counters[7]) > 0  # k_wide's ReLU instances played the games
    path = checkpoint.save(ga, str(tmp_path / "relu_wide.safetensors"))
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.activation == "relu" and ga2.kernel == "relu_wide" == ga2.ev.kernel and list(ga2.nodes) == shape
    rec, rec2 = ga.step(), ga2.step()
    torch.cuda.synchronize()
    assert rec == rec2
    assert torch.equal(ga.population_full(), ga2.population_full()) and torch.equal(ga.fitness, ga2.fitness)


@pytest.fixture
def relu_wide_dropin():
    """config.ACTIVATION = "relu" and config.KERNEL = "relu_wide" as a user sets
    them: numpy_nn initialises its activation_function from the knob when it is
    imported; the kernel knob is read at each call."""
    with dropin_config(activation="relu", kernel="relu_wide"):
        import config
        yield config


def test_dropin_evaluate_equals_general(gpu, relu_wide_dropin):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,72,40,2] ReLU network
    with config.KERNEL = "relu_wide" against the same call with KERNEL =
    "general": the same hall, the same random seed, the same fitness."""
    import main
    import numpy_nn
    import utils
    config = relu_wide_dropin
    assert numpy_nn.activation() == "relu"
    shape = [6, 72, 40, 2]
    rng = np.random.default_rng(78)
    G = gene_count(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]

        ev = main._evaluator()
        assert ev.activation == "relu" and list(ev.nodes) == shape and ev.kernel == "relu_wide"
        got = dropin_fitness(hall, inds)
        config.KERNEL = "general"
        ev_g = main._evaluator()
        assert ev_g is not ev and ev_g.kernel == "general"
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
