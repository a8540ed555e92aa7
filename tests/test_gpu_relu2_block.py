"""k_relu2_block on the MI355X (run with -m gpu): ReLU networks with two hidden
layers of up to 128 units, [6, 2..128, 2..128, 2..4] with bias, on the certified
f32 kernel that gives a game a 256-thread block (PG_KERNEL_RELU2_BLOCK;
pg_relu2_block_decide pins its decisions).

Checkers: numpy's own forward (np.dot per layer, as NeuralNetwork.run does) and
pg_forward in f64 for single decisions, the host model of the f32 chain
(tests/_relu2_model.py, its BLOCK layout) for z32, the gcc-compiled bound, the general
kernel for whole games and k_relu2 on the shapes both kernels take.  All games
run with timeout_thresh=119, win_score=1."""

import numpy as np
import pytest
import torch

import _relu2_model as M
from _gpu_support import dev_genomes, dropin_config, dropin_fitness, ids, refused, same

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
EDGE_SHAPES = [[6, 2, 2, 2], [6, 65, 2, 2], [6, 2, 65, 3], [6, 100, 100, 3], [6, 128, 128, 4]]
GAME_SHAPES = [[6, 65, 2, 2], [6, 100, 100, 3], [6, 128, 128, 4]]


def _ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, activation="relu", **kw)


def _decide(ev, gpu, genomes, k, gidx, forward=True):
    """relu2_block_decide (and the f64 pg_forward's index) on passes k [n, 6] of genomes[gidx]."""
    gt, kt = dev_genomes(genomes, gpu, ev.dtype), torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.relu2_block_decide(gt, kt, genome_index=it)
    out = [index, stage, z32, bound]
    if forward:
        out.append(ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64")[0])
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _one_ulp32(got, want):
    """got within one f32 ulp of want (both f32, finite or inf alike)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    inf = np.isinf(want)
    assert (np.isinf(got) == inf).all()
    assert (np.abs(got[~inf].view(np.int32).astype(np.int64) - want[~inf].view(np.int32).astype(np.int64)) <= 1).all()


# ------------------------------------------------------- 1 random passes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.BLOCK.SHAPES, ids=ids)
def test_decide_random_passes(gpu, tmp_path, shape, dtype):
    """64 networks (U[0,1), N(0,1) and N(0,3) genes) x 64 inputs = 4 096 passes:
    z32 is the host model's chain bit for bit, the bound the gcc-compiled one to
    one f32 ulp, and every index numpy's own forward's and pg_forward's."""
    rng = np.random.default_rng(sum(shape) + 40)
    G = M.genes(shape)
    genomes = rng.standard_normal((64, G))
    genomes[:16] = rng.random((16, G))
    genomes[48:] *= 3.0
    if dtype == torch.float32:
        genomes = genomes.astype(np.float32).astype(np.float64)  # the network the f32 population holds
    k = rng.integers(0, 321, size=(64, 64, 6))
    gidx = np.repeat(np.arange(64), 64)
    index, stage, z32, bound, fwd = _decide(_ev(shape, gpu, dtype=dtype), gpu, genomes, k.reshape(-1, 6), gidx)
    want = M.z32(M.BLOCK, shape, genomes, k).reshape(-1, shape[-1])
    np.testing.assert_array_equal(z32.view(np.int32), want.view(np.int32))
    _one_ulp32(bound, M.bounds(tmp_path, M.BLOCK, shape, genomes)[gidx])
    assert np.isfinite(bound).all() and set(np.unique(stage)) <= {0, 1}
    np.testing.assert_array_equal(index, M.numpy_index(shape, genomes, k).ravel())
    np.testing.assert_array_equal(index, fwd)
    # the decision is the documented one: stage 0 exactly where relu_certify proves an index under the bound
    np.testing.assert_array_equal(stage, (M.certify(want, bound) < 0).astype(np.int32))
    print(f"{shape} {dtype}: stage-1 share {np.mean(stage == 1):.5f} of {len(stage)} passes")


# ------------------------------------- 2 the certificate must do the work ----
@pytest.mark.parametrize("law", ["normal1", "normal3", "uniform"])
@pytest.mark.parametrize("shape", M.BLOCK.SHAPES, ids=ids)
def test_certificate_decides_most_passes(gpu, shape, law):
    """An e = inf bug would pass every equality above: per shape and gene law
    the share of passes decided by the f32 certificate (stage 0) is at least
    0.95 of 4 096 (numpy with K = 150: 0.990 .. 1.000 per cell)."""
    rng = np.random.default_rng(sum(shape) + {"normal1": 50, "normal3": 51, "uniform": 52}[law])
    G = M.genes(shape)
    genomes = {"normal1": lambda: rng.standard_normal((64, G)), "normal3": lambda: rng.standard_normal((64, G)) * 3.0,
               "uniform": lambda: rng.random((64, G))}[law]()
    k = rng.integers(0, 321, size=(4096, 6))
    index, stage, _, bound = _decide(_ev(shape, gpu), gpu, genomes, k, np.repeat(np.arange(64), 64), forward=False)
    share = float(np.mean(stage == 0))
    print(f"{shape} {law}: stage-0 share {share:.4f}")
    assert np.isfinite(bound).all()
    assert share >= 0.95


# --------------------------------------------------------- 3 built cases ----
def _tie_swapped(shape, rng):
    """Equal outputs that only np.dot's summation order tells apart: the layer-2
    units come in identical pairs (W2[2i+1] = W2[2i]), every output row carries
    the same non-negative weights and the same positive bias, and in the rows
    o >= 1 the two weights of a random half of the pairs are swapped.  f32 values."""
    _, H1, H2, O = shape
    w1 = rng.standard_normal((H1, 7))
    w2 = rng.standard_normal((H2, H1 + 1)) / np.sqrt(H1)
    w2[1::2] = w2[0:2 * (H2 // 2):2]
    row = np.append(rng.random(H2) * 0.5, 0.125 + rng.random() * 0.25)
    w3 = np.tile(row, (O, 1))
    for o in range(1, O):
        for i in np.flatnonzero(rng.random(H2 // 2) < 0.5):
            w3[o, 2 * i], w3[o, 2 * i + 1] = w3[o, 2 * i + 1], w3[o, 2 * i]
    return M.pack(w1, w2, w3).astype(np.float32).astype(np.float64)


def _bias_delta(shape, rng, base=None):
    """Outputs 0 and 1 with equal non-negative rows but for the bias of output 1 (set by the caller); further rows zero."""
    _, H1, H2, O = shape
    if base is None:
        w1 = rng.random((H1, 7)) * 0.1
        w2 = rng.random((H2, H1 + 1)) * (0.5 / H1)
        row = np.append(rng.random(H2) * (0.6 / H2), 0.125)
        w3 = np.zeros((O, H2 + 1))
        w3[0] = row
        w3[1] = row
        base = M.pack(w1, w2, w3).astype(np.float32).astype(np.float64)
    return base


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=ids)
def test_decide_built_cases(gpu, shape):
    _, H1, H2, O = shape
    rng = np.random.default_rng(60 + sum(shape))
    G = M.genes(shape)
    ev = _ev(shape, gpu)
    a, b = H1 * 7, H1 * 7 + H2 * (H1 + 1)
    seen = set()

    def check(nets, k, gidx):
        index, stage, z32, bound, fwd = _decide(ev, gpu, nets, k, gidx)
        want = np.concatenate([M.numpy_index(shape, nets[i:i + 1], k[gidx == i][None])[0] for i in range(len(nets))])
        order = np.concatenate([np.flatnonzero(gidx == i) for i in range(len(nets))])
        np.testing.assert_array_equal(index[order], want)
        np.testing.assert_array_equal(index, fwd)
        seen.update(np.unique(stage).tolist())
        return index, stage, bound

    # (a) tie networks: every pass goes to the f64 path, which must reproduce np.dot's last bit
    nets = np.array([_tie_swapped(shape, rng) for _ in range(4)])
    k = rng.integers(0, 321, size=(4 * 64, 6))
    gidx = np.repeat(np.arange(4), 64)
    index, stage, bound = check(nets, k, gidx)
    assert (stage == 1).all() and np.isfinite(bound).all()
    # (b) a bias difference delta around 2e: certified beyond it, f64 within it
    base = _bias_delta(shape, rng)
    e = float(M.bound_numpy(M.BLOCK, shape, base[None])[0])
    factors = np.array([0.0, 0.5, -0.5, 1.5, -1.5, 1.9, -1.9, 2.1, -2.1, 2.5, -2.5, 8.0, -8.0])
    nets = np.tile(base, (len(factors), 1))
    bias1 = b + (H2 + 1) + H2
    nets[:, bias1] = nets[:, bias1] + factors * e
    assert 0.02 < M.s_max(shape, base) < 5 and e < 1e-3 * nets[0, bias1]
    k = rng.integers(0, 321, size=(len(factors) * 32, 6))
    gidx = np.repeat(np.arange(len(factors)), 32)
    index, stage, bound = check(nets, k, gidx)
    f = factors[gidx]
    assert (index[f > 0] == 1).all() and (index[f < 0] == 0).all()
    assert (stage[np.abs(f) <= 1.9] == 1).all(), "a gap within 2e must not be certified"
    assert (stage[np.abs(f) >= 2.1] == 0).all(), "a gap beyond 2e is the certificate's"
    # (c) the zero boundary: all outputs but the last strongly negative, the last at +-1e-9
    nets = []
    for last in (1e-9, -1e-9):
        w3 = np.zeros((O, H2 + 1))
        w3[:O - 1, :H2] = -np.abs(rng.standard_normal((O - 1, H2)))
        w3[:O - 1, H2] = -5.0
        w3[O - 1, H2] = last
        nets.append(M.pack(rng.standard_normal((H1, 7)), rng.standard_normal((H2, H1 + 1)), w3))
    k = rng.integers(0, 321, size=(128, 6))
    gidx = np.repeat(np.arange(2), 64)
    index, stage, bound = check(np.array(nets), k, gidx)
    assert (index[gidx == 0] == O - 1).all() and (index[gidx == 1] == 0).all() and (stage == 1).all()
    # (d) the all-zero genome; a 1e30 weight in each layer; a NaN gene; an inf gene met by a zero input; f32-subnormal
    # genes; the all-zero genome but for one f32-subnormal gene, the bias of output 1: only f64 sees it win
    g = rng.standard_normal((8, G))
    g[0] = 0.0
    g[1, 5], g[2, a + 1], g[3, b + 1] = 1e30, -1e30, 1e30
    g[4, a + H1 + 1] = np.nan
    g[5, 0] = np.inf
    g[6] = M.tiny_net(shape, rng)
    g[7] = 0.0
    g[7, bias1] = 1e-40
    k = rng.integers(0, 321, size=(8 * 32, 6))
    gidx = np.repeat(np.arange(8), 32)
    k[gidx == 5, 0] = 0  # inf x 0
    index, stage, bound = check(g, k, gidx)
    assert (stage == 1).all() and (index[gidx == 0] == 0).all() and (index[gidx == 7] == 1).all()
    assert np.isinf(bound[(gidx >= 1) & (gidx <= 5)]).all() and np.isfinite(bound[(gidx == 0) | (gidx >= 6)]).all()
    assert seen == {0, 1}  # each stage occurred


# --------------------------------------------------------- 4 whole games ----
def _hard_rows(shape, rng):
    """A genome whose every forward needs f64 (a tie network), a NaN genome and a 1e30 genome (f32 values)."""
    G = M.genes(shape)
    nan, big = rng.standard_normal(G), rng.standard_normal(G)
    nan[int(rng.integers(0, G))] = np.nan
    big[shape[1] * 7] = 1e30
    return np.array([_tie_swapped(shape, rng), nan, big]).astype(np.float32).astype(np.float64)


def _population(shape, rng, n, gpu, dtype):
    g = rng.standard_normal((n, M.genes(shape)))
    g[:3] = _hard_rows(shape, rng)
    return dev_genomes(g, gpu, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", GAME_SHAPES, ids=ids)
def test_kernel_equals_general(gpu, shape, dtype):
    """48 genomes x 6 games on the reference schedule and all self-play, with a
    genome whose every forward needs f64, a NaN and a 1e30 genome among genomes
    and hall: fitness, rewards, scores, frames, total_frames, status and the
    traces equal the general kernel's bit for bit; every frame is stepped; also
    through genome_rows (a permutation) with n_active below n."""
    rng = np.random.default_rng(sum(shape) + 70)
    n, H = 48, 8
    genomes, hall = _population(shape, rng, n, gpu, dtype), _population(shape, rng, H, gpu, dtype)
    opp = rng.integers(0, H, size=(n, 6)).astype(np.int32)
    opp[:, 3] = np.arange(n) % 3  # the hard hall rows are met
    mult = np.round(rng.normal(size=(n, 6)), 3)
    ev = _ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    for kinds in ([0, 1, 2, 3, 3, 3], [3, 3, 3, 3, 3, 3]):
        sched = [torch.tensor(a, device=gpu) for a in (np.tile(np.array(kinds, np.int32), (n, 1)), opp, mult)]
        hot, hot_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="relu2_block", trace_games=n * 6, trace_cap=1024)
        ref, ref_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="general", trace_games=n * 6, trace_cap=1024)
        torch.cuda.synchronize()
        same(hot, ref)
        assert torch.equal(hot_tr, ref_tr) and int(hot_tr.any())
        ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
        assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all()
        assert ch[0] == int(ref.frames.sum()) and ch[3] == n * 6 and ch[8] == 0 and ch[12] == 0
        assert 0 < ch[2] == ch[4] < ch[1]  # the hard rows take the f64 path, the certificate carries the rest
        print(f"{shape} {dtype} {kinds}: f64 share {ch[2] / ch[1]:.5f} of {ch[1]} forwards")
    perm = torch.tensor(rng.permutation(n).astype(np.int32), device=gpu)
    act = torch.tensor([31], dtype=torch.int32, device=gpu)
    hot2, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="relu2_block", rows=perm, n_active=act)
    ref2, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="general", rows=perm, n_active=act)
    whole, _ = ev.evaluate(genomes[perm.long()].contiguous(), *sched, opponents=hall, kernel="relu2_block")
    torch.cuda.synchronize()
    same(hot2, ref2, 31)
    same(hot2, whole, 31)
    assert int(hot2.counters[3]) == 31 * 6 == int(ref2.counters[3])


def test_blocks_reload_games_in_place(gpu):
    """One launch with at least twice as many games as the persistent grid has
    blocks (2 per CU), so every block takes further games from the queue and
    replaces both networks in place: still the general kernel's results, and
    the games and steps counters are the sums over the results."""
    shape, dtype = [6, 65, 2, 2], torch.float32
    rng = np.random.default_rng(80)
    blocks = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    n = -(-2 * blocks // 6) + 1
    assert n * 6 >= 2 * blocks
    H = 16
    genomes, hall = _population(shape, rng, n, gpu, dtype), _population(shape, rng, H, gpu, dtype)
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    sched = [torch.tensor(a, device=gpu) for a in (kinds, rng.integers(0, H, size=(n, 6)).astype(np.int32),
                                                   np.round(rng.normal(size=(n, 6)), 3))]
    ev = _ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    hot, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="relu2_block")
    ref, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="general")
    torch.cuda.synchronize()
    same(hot, ref)
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert ch[3] == n * 6 and ch[0] == int(hot.frames.sum()) and (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all()
    assert ch[8] == 0 and ch[12] == 0


@pytest.mark.parametrize("shape", [[6, 16, 16, 3], [6, 64, 64, 3]], ids=ids)
def test_overlap_with_relu2(gpu, shape):
    """On the shapes k_relu2 takes too, the outputs and the steps / forwards /
    games counters are k_relu2's."""
    rng = np.random.default_rng(sum(shape) + 90)
    n, H = 64, 8
    genomes, hall = _population(shape, rng, n, gpu, torch.float64), _population(shape, rng, H, gpu, torch.float64)
    sched = [torch.tensor(a, device=gpu) for a in (np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1)),
                                                   rng.integers(0, H, size=(n, 6)).astype(np.int32),
                                                   np.round(rng.normal(size=(n, 6)), 3))]
    ev = _ev(shape, gpu, timeout_thresh=119, win_score=1)
    hot, hot_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="relu2_block", trace_games=64, trace_cap=1024)
    ref, ref_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="relu2", trace_games=64, trace_cap=1024)
    torch.cuda.synchronize()
    same(hot, ref)
    assert torch.equal(hot_tr, ref_tr)
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all() and ch[3] == n * 6


# ------------------------------------------------------------ 5 refusals ----
def test_unsupported_combinations_are_refused(gpu):
    from pong_amd.device import Evaluator
    shape = [6, 128, 128, 3]
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    def genomes(ev):
        return torch.zeros((4, ev.genes), dtype=torch.float64, device=gpu)

    ev = _ev(shape, gpu)
    g = genomes(ev)
    sig = Evaluator(shape, device=gpu)
    refused(lambda: sig.evaluate(g, z, z, m, kernel="relu2_block"), "sigmoid")
    refused(lambda: sig.relu2_block_decide(g, k), "PG_ACT_RELU")
    for other in ([6, 128, 3], [6, 129, 128, 3], [6, 128, 129, 3], [6, 1, 16, 2], [6, 16, 1, 2], [6, 8, 8, 8, 2]):
        eo = _ev(other, gpu)
        refused(lambda: eo.evaluate(genomes(eo), z, z, m, kernel="relu2_block"), "relu2_block kernel needs")
        refused(lambda: eo.relu2_block_decide(genomes(eo), k), "pg_relu2_block_decide")
    nb = _ev(shape, gpu, bias=False)
    refused(lambda: nb.evaluate(genomes(nb), z, z, m, kernel="relu2_block"), "bias")
    refused(lambda: nb.relu2_block_decide(genomes(nb), k), "bias")
    refused(lambda: _ev(shape, gpu, precision="f64").evaluate(g, z, z, m, kernel="relu2_block"), "certified")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu2_block", horizon=1000), "whole episodes")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu2_block", hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)),
            "hard-case log")
    with pytest.raises(KeyError):
        ev.evaluate(g, z, z, m, kernel="relu2_block+advance")
    with pytest.raises(KeyError):
        ev.evaluate(g, z, z, m, kernel="relu2_block+solo")
    # the supported neighbours of the refused calls still run; AUTO stays on the general kernel
    assert ev.resolved_kernel() == "general" and ev.resolved_kernel("relu2_block") == "relu2_block"
    for kernel in ("relu2_block", "auto", "general"):
        res, _ = ev.evaluate(g, z, z, m, kernel=kernel)
        assert int(res.counters[3]) == 24
    index, stage, _, _ = ev.relu2_block_decide(g, k)
    assert (index.cpu().numpy() == 0).all() and (stage.cpu().numpy() == 1).all()


# ------------------------------------------------- 6 DeviceGA, the drop-in ----
def test_device_ga_generations_and_checkpoint(gpu, tmp_path):
    """DeviceGA(kernel="relu2_block") over three generations equals kernel="general", through a checkpoint round trip."""
    from pong_amd import checkpoint
    from pong_amd.evolve import DeviceGA
    shape = [6, 65, 8, 3]

    def make(kernel):
        ga = DeviceGA(shape, 64, device=gpu, schedule="selfplay", seed=9, activation="relu", kernel=kernel)
        ga.initialize("normal", 1.0)
        return ga

    ga, ref = make("relu2_block"), make("general")
    assert ga.ev.kernel == "relu2_block" and ga.ev.resolved_kernel() == "relu2_block"
    for _ in range(2):
        assert ga.step() == ref.step()
    path = checkpoint.save(ga, str(tmp_path / "relu2_block.safetensors"))
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.kernel == "relu2_block" and ga2.activation == "relu" and list(ga2.nodes) == shape
    rec, rec2, rec_ref = ga.step(), ga2.step(), ref.step()
    torch.cuda.synchronize()
    assert rec == rec2 == rec_ref
    for other in (ga2, ref):
        assert torch.equal(ga.population_full(), other.population_full()) and torch.equal(ga.fitness, other.fitness)


@pytest.fixture
def relu_dropin():
    """config.ACTIVATION = "relu" and config.KERNEL = "relu2_block" as a user sets them."""
    with dropin_config(activation="relu", kernel="relu2_block"):
        import numpy_nn
        yield numpy_nn


def test_dropin_evaluate_equals_general(gpu, relu_dropin, monkeypatch):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,100,100,2] ReLU network
    with config.KERNEL = "relu2_block" against the same call with the evaluator
    held to the general kernel: the same hall, the same random seed, the same fitness."""
    import main
    import utils
    assert relu_dropin.activation() == "relu"
    shape = [6, 100, 100, 2]
    rng = np.random.default_rng(77)
    G = M.genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((12, G))]

        ev = main._evaluator()
        assert ev.activation == "relu" and list(ev.nodes) == shape and ev.kernel == "relu2_block"
        got = dropin_fitness(hall, inds)
        monkeypatch.setattr(ev, "kernel", "general")
        assert main._evaluator() is ev
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
