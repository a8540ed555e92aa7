"""k_relu2 on the MI355X (run with -m gpu): ReLU networks with two hidden
layers, [6, 2..64, 2..64, 2..4] with bias, on the certified f32 game kernel
(PG_KERNEL_RELU2; pg_relu2_decide pins its decisions).

Checkers: the reference's own numbers (tests/golden/relu_forward.npz), pg_forward
in f64 for single decisions, and the general kernel for whole games
(tests/test_gpu_relu.py pins it to the reference's numpy loop at [6,5,4,2])."""

import numpy as np
import pytest
import torch

import _relu2_model as M
from _gpu_support import dev_genomes, dropin_config, dropin_fitness, ids, refused, same

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
DTYPES = [torch.float64, torch.float32]


def _relu_ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, activation="relu", **kw)


def _decide_both(ev, gpu, genomes, k, gidx):
    """relu2_decide and the f64 pg_forward on the same passes (genomes as ev's dtype holds them)."""
    gt, kt = dev_genomes(genomes, gpu, ev.dtype), torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.relu2_decide(gt, kt, genome_index=it)
    ref_idx, _ = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64", want_layers=True)
    z64 = ev.last_layers[0][:, -ev.nodes[-1]:]
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, stage, z32, bound, ref_idx, z64))


def _margin(z64):
    top = -np.sort(-z64, axis=1)
    return np.where(top[:, 0] <= 0, -top[:, 0], top[:, 0] - np.maximum(top[:, 1], 0.0))


# ------------------------------------------------- 1 the reference's numbers ----
def test_decide_equals_reference(gpu, golden):
    """6x64x64x2 of relu_forward.npz (the reference's NeuralNetwork.run with
    ReLU): on the samples whose inputs are doubled centroids / 320, the index."""
    g = golden("relu_forward.npz")
    key = "6x64x64x2"
    shape = [int(v) for v in g[f"{key}__shape"]]
    x = g[f"{key}__x"]
    k = np.rint(x * 320).astype(np.int64)
    sel = np.flatnonzero(((k / 2) / 160 == x).all(axis=1) & (k >= 0).all(axis=1) & (k <= 320).all(axis=1))
    assert len(sel) == len(x) // 2
    ev = _relu_ev(shape, gpu)
    index, stage, _, bound = ev.relu2_decide(dev_genomes(g[f"{key}__genes"], gpu), torch.tensor(k[sel].astype(np.int32), device=gpu),
                                             genome_index=torch.tensor(g[f"{key}__gidx"][sel].astype(np.int32), device=gpu))
    np.testing.assert_array_equal(index.cpu().numpy(), g[f"{key}__idx"][sel])
    assert set(np.unique(stage.cpu().numpy())) <= {0, 1} and np.isfinite(bound.cpu().numpy()).all()


# ------------------------------------------------------- 2 random passes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.LANES.SHAPES, ids=ids)
def test_decide_random_passes(gpu, shape, dtype):
    """64 networks x 512 inputs: the decision is the f64 forward's, |z32 - z64|
    stays within the (finite) bound, z32 is the host model's chain bit for bit,
    every pass with a large f64 margin (> 1e-3 max_o S_o) is certified in f32,
    those are more than half, and at most 5 % of all passes take the f64 path."""
    rng = np.random.default_rng(sum(shape))
    G = M.genes(shape)
    genomes = rng.standard_normal((64, G))
    genomes[:16] = rng.random((16, G))
    if dtype == torch.float32:
        genomes = genomes.astype(np.float32).astype(np.float64)  # the network the f32 population holds
    k = rng.integers(0, 321, size=(64 * 512, 6))
    gidx = np.repeat(np.arange(64), 512)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(_relu_ev(shape, gpu, dtype=dtype), gpu, genomes, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert np.isfinite(bound).all()
    assert (np.abs(z32.astype(np.float64) - z64) <= bound[:, None]).all()
    s = M.s_max(shape, genomes)[gidx]
    assert (bound <= 2 * M.LANES.K * U32 * s).all()
    large = _margin(z64) > 1e-3 * s
    assert set(np.unique(stage)) <= {0, 1}
    print(f"{shape} {dtype}: stage-1 share {np.mean(stage == 1):.5f} of {len(stage)} passes "
          f"({np.mean(large):.4f} with a large margin)")
    assert (stage[large] == 0).all()
    assert large.mean() > 0.5
    assert np.mean(stage == 1) <= 0.05
    # the f32 chain is the documented one: the host model's z32 on the first 8 inputs of every network
    sub = (np.arange(64)[:, None] * 512 + np.arange(8)[None, :]).ravel()
    want = M.z32(M.LANES, shape, genomes, k[sub].reshape(64, 8, 6)).reshape(-1, shape[-1])
    np.testing.assert_array_equal(z32[sub].view(np.int32), want.view(np.int32))


# --------------------------------------------------------- 3 hard inputs ----
def _tie_nets(shape, rng, deltas):
    """Two equal W3 rows (outputs 0 and 1) but for a bias difference delta;
    non-negative weights throughout, so every output is > 0 and S ~ 1; any
    further output rows are zero."""
    _, H1, H2, O = shape
    nets = []
    for d in deltas:
        w1 = rng.random((H1, 7)) * 0.1
        w2 = rng.random((H2, H1 + 1)) * (0.5 / H1)
        row = np.append(rng.random(H2) * (0.6 / H2), 0.125)
        w3 = np.zeros((O, H2 + 1))
        w3[0] = row
        w3[1] = row + np.append(np.zeros(H2), d)
        nets.append(M.pack(w1, w2, w3))
    return np.array(nets)


@pytest.mark.parametrize("shape", [[6, 16, 16, 3], [6, 17, 33, 4], [6, 64, 64, 3], [6, 20, 32, 4]], ids=ids)
def test_decide_hard_inputs(gpu, shape):
    _, H1, H2, O = shape
    rng = np.random.default_rng(5 + sum(shape))
    G = M.genes(shape)
    ev = _relu_ev(shape, gpu)
    # (a) ties and near-ties
    deltas = [0.0, 1e-12, -1e-12, 1e-7, -1e-7, 1e-3, -1e-3]
    nets = _tie_nets(shape, rng, deltas)
    assert all(0.05 < s < 5 for s in M.s_max(shape, nets))
    k = rng.integers(0, 321, size=(len(deltas) * 64, 6))
    gidx = np.repeat(np.arange(len(deltas)), 64)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, nets, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    d = np.array(deltas)[gidx]
    assert (z64[:, :2] > 0).all()
    assert (index[d > 0] == 1).all() and (index[d < 0] == 0).all() and set(index[d == 0]) <= {0, 1}
    assert (stage[np.abs(d) <= 1e-7] == 1).all()
    assert (stage[np.abs(d) == 1e-3] == 0).all()
    # (b) the zero boundary: all outputs but the last strongly negative, the last at +-1e-9
    nets = []
    for last in (1e-9, -1e-9):
        w3 = np.zeros((O, H2 + 1))
        w3[:O - 1, :H2] = -np.abs(rng.standard_normal((O - 1, H2)))
        w3[:O - 1, H2] = -5.0
        w3[O - 1, H2] = last
        nets.append(M.pack(rng.standard_normal((H1, 7)), rng.standard_normal((H2, H1 + 1)), w3))
    k = rng.integers(0, 321, size=(128, 6))
    gidx = np.repeat(np.arange(2), 64)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, np.array(nets), k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert (index[gidx == 0] == O - 1).all() and (index[gidx == 1] == 0).all() and (stage == 1).all()
    # (c) the all-zero genome; a weight f32 sums cannot hold in each layer; a NaN gene; an f32-subnormal gene
    a, b = H1 * 7, H1 * 7 + H2 * (H1 + 1)
    # (and the all-zero genome but for one f32-subnormal gene, the bias of output 1: only f64 sees it win)
    g = rng.standard_normal((7, G))
    g[0] = 0.0
    g[1, 5], g[2, a + 3], g[3, b + 1] = 1e30, -1e30, 1e30
    g[4, a + 1] = np.nan
    g[5] = M.tiny_net(shape, rng)
    g[6] = 0.0
    g[6, b + (H2 + 1) + H2] = 1e-40
    k = rng.integers(0, 321, size=(7 * 64, 6))
    gidx = np.repeat(np.arange(7), 64)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, g, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert (stage == 1).all() and (index[gidx == 0] == 0).all() and (index[gidx == 6] == 1).all()
    assert np.isinf(bound[(gidx >= 1) & (gidx <= 4)]).all() and np.isfinite(bound[(gidx == 0) | (gidx >= 5)]).all()


# --------------------------------------------------------- 4 whole games ----
def _f64_rows(shape, rng, n):
    """n genomes that always need the f64 path: tie, 1e30, all-zero and NaN, in turn (f32 values throughout)."""
    _, H1, H2, O = shape
    G = M.genes(shape)
    a = H1 * 7
    rows = []
    for i in range(n):
        if i % 4 == 0:
            g = _tie_nets(shape, rng, [0.0])[0]
        elif i % 4 == 1:
            g = rng.standard_normal(G)
            g[(0, a, G - 1)[(i // 4) % 3]] = 1e30
        elif i % 4 == 2:
            g = np.zeros(G)
        else:
            g = rng.standard_normal(G)
            g[int(rng.integers(0, G))] = np.nan
        rows.append(g)
    return np.array(rows).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.LANES.SHAPES, ids=ids)
def test_relu2_kernel_equals_general(gpu, shape, dtype):
    """k_relu2's certified decisions are the f64 forward's: every output array,
    the per-frame traces of the first 64 games and the step / forward / game
    counters equal the general kernel's, the certified path carries the games,
    AUTO resolves to k_relu2; also on genomes that always need the f64 path,
    and through genome_rows (a permutation) with n_active below n."""
    rng = np.random.default_rng(sum(shape) + 1)
    G = M.genes(shape)
    n, H = 256, 16
    genomes, opponents = dev_genomes(rng.standard_normal((n, G)), gpu, dtype), dev_genomes(rng.standard_normal((H, G)), gpu, dtype)
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    opp = rng.integers(0, H, size=(n, 6)).astype(np.int32)
    mult = np.round(rng.normal(size=(n, 6)), 3)
    assert (mult < 0).any() and (mult > 0).any()
    sched = [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    ev = _relu_ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    got = {}
    for kernel in ("relu2", "general", "auto"):
        got[kernel] = ev.evaluate(genomes, *sched, opponents=opponents, kernel=kernel, trace_games=64, trace_cap=2048)
    torch.cuda.synchronize()
    (hot, hot_tr), (ref, ref_tr), (auto, _) = got["relu2"], got["general"], got["auto"]
    same(hot, ref)
    assert torch.equal(hot_tr, ref_tr) and int(hot_tr.any())
    ch, cr, ca = (r.counters.cpu().numpy() for r in (hot, ref, auto))
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all()
    assert ch[0] == int(ref.frames.sum()) and ch[3] == n * 6 and ch[8] == 0 and ch[12] == 0
    print(f"{shape} {dtype}: f64 share {ch[2] / ch[1]:.5f} of {ch[1]} forwards")
    assert ch[2] == ch[4] <= 0.25 * ch[1]
    assert (ca == ch).all()  # AUTO resolves to k_relu2 in its scope
    # genomes and opponents that always need the f64 path
    hard, hard_opp = dev_genomes(_f64_rows(shape, rng, 64), gpu, dtype), dev_genomes(_f64_rows(shape, rng, H), gpu, dtype)
    hsched = [t[:64].contiguous() for t in sched]
    hot_h, tr_h = ev.evaluate(hard, *hsched, opponents=hard_opp, kernel="relu2", trace_games=64, trace_cap=2048)
    ref_h, rtr_h = ev.evaluate(hard, *hsched, opponents=hard_opp, kernel="general", trace_games=64, trace_cap=2048)
    torch.cuda.synchronize()
    same(hot_h, ref_h)
    assert torch.equal(tr_h, rtr_h)
    chh = hot_h.counters.cpu().numpy()
    assert (chh[[0, 1, 3]] == ref_h.counters.cpu().numpy()[[0, 1, 3]]).all() and chh[2] == chh[4] == chh[1]
    # genome_rows as a permutation, n_active below n
    perm = torch.tensor(rng.permutation(n).astype(np.int32), device=gpu)
    act = torch.tensor([170], dtype=torch.int32, device=gpu)
    hot2, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="relu2", rows=perm, n_active=act)
    ref2, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general", rows=perm, n_active=act)
    whole, _ = ev.evaluate(genomes[perm.long()].contiguous(), *sched, opponents=opponents, kernel="relu2")
    torch.cuda.synchronize()
    same(hot2, ref2, 170)
    same(hot2, whole, 170)
    assert int(hot2.counters[3]) == 170 * 6 == int(ref2.counters[3])


@pytest.mark.parametrize("shape,n,dtype", [([6, 16, 16, 3], 4096, torch.float64), ([6, 20, 32, 4], 1024, torch.float32),
                                           ([6, 64, 64, 3], 1024, torch.float64)], ids=ids)
def test_relu2_groups_play_several_games(gpu, shape, n, dtype):
    """More games than the launch has lane groups (2 blocks per CU of 32, 8 or 4
    groups), so every group takes further games from the queue and replaces its
    networks in place: still the general kernel's results."""
    rng = np.random.default_rng(sum(shape) + 2)
    G = M.genes(shape)
    LN, _ = M.lanes(shape[1], shape[2])
    groups = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count * (256 // (2 * LN))
    assert n * 6 > 1.4 * groups
    H = 64
    genomes, opponents = dev_genomes(rng.standard_normal((n, G)), gpu, dtype), dev_genomes(rng.standard_normal((H, G)), gpu, dtype)
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    sched = [torch.tensor(a, device=gpu) for a in (kinds, rng.integers(0, H, size=(n, 6)).astype(np.int32),
                                                   np.round(rng.normal(size=(n, 6)), 3))]
    ev = _relu_ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    hot, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="relu2")
    ref, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general")
    torch.cuda.synchronize()
    same(hot, ref)
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all() and ch[3] == n * 6 and ch[2] == ch[4] <= 0.25 * ch[1]


@pytest.mark.parametrize("shape", [[6, 2, 2, 2], [6, 17, 3, 3], [6, 33, 64, 4]], ids=ids)
def test_relu2_counter_flush(gpu, shape):
    """The shared game loop's flush of a family whose stages are 0/1: one
    count of f64 forwards goes to both [2] and [4].  The smallest padded shape
    of each layout (4, 16, 32 lanes), 8 genomes x 2 games against hall rows so
    that both half-groups play; half of the rows always need the f64 path."""
    rng = np.random.default_rng(sum(shape) + 3)
    G = M.genes(shape)
    genomes = dev_genomes(np.concatenate([rng.standard_normal((4, G)), _f64_rows(shape, rng, 4)]), gpu, torch.float64)
    hall = dev_genomes(np.concatenate([rng.standard_normal((2, G)), _f64_rows(shape, rng, 2)]), gpu, torch.float64)
    sched = [torch.tensor(a, device=gpu) for a in (np.full((8, 2), 3, np.int32), rng.integers(0, 4, size=(8, 2)).astype(np.int32),
                                                   np.ones((8, 2)))]
    ev = _relu_ev(shape, gpu, n_games=2, timeout_thresh=119, win_score=1)
    res, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="relu2")
    c = res.counters.cpu().numpy()
    print(f"{shape}: forwards {c[1]}, f64 {c[2]}")
    assert 0 < c[2] == c[4] <= c[1]


# ------------------------------------------------------------ 5 refusals ----
def test_unsupported_combinations_are_refused(gpu):
    from pong_amd.device import Evaluator
    shape = [6, 64, 64, 3]
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    def genomes(ev):
        return torch.zeros((4, ev.genes), dtype=torch.float64, device=gpu)

    ev = _relu_ev(shape, gpu)
    g = genomes(ev)
    sig = Evaluator(shape, device=gpu)
    refused(lambda: sig.evaluate(g, z, z, m, kernel="relu2"), "sigmoid")
    refused(lambda: sig.relu2_decide(g, k), "PG_ACT_RELU")
    for other in ([6, 64, 3], [6, 65, 64, 3], [6, 64, 65, 3], [6, 1, 16, 2], [6, 16, 1, 2], [6, 8, 8, 8, 2]):
        eo = _relu_ev(other, gpu)
        refused(lambda: eo.evaluate(genomes(eo), z, z, m, kernel="relu2"), "relu2")
        refused(lambda: eo.relu2_decide(genomes(eo), k), "relu2")
    nb = _relu_ev(shape, gpu, bias=False)
    refused(lambda: nb.evaluate(genomes(nb), z, z, m, kernel="relu2"), "bias")
    refused(lambda: _relu_ev(shape, gpu, precision="f64").evaluate(g, z, z, m, kernel="relu2"), "certified")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu2", horizon=1000), "horizon")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu2", hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)),
            "hard")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu"), "relu")  # outside k_relu's shapes
    refused(lambda: ev.evaluate(g, z, z, m, kernel="wide"), "relu")
    refused(lambda: ev.wide_decide(g, k), "relu")
    refused(lambda: ev.relu_decide(g, k), "relu")
    # the supported neighbours of the refused calls still run
    for kernel in ("relu2", "auto", "general"):
        res, _ = ev.evaluate(g, z, z, m, kernel=kernel)
        assert int(res.counters[3]) == 24
    res, _ = _relu_ev(shape, gpu, precision="f64").evaluate(g, z, z, m)  # AUTO with f64 precision: the general kernel
    assert int(res.counters[3]) == 24 and int(res.counters[4]) == 0
    index, stage, _, _ = ev.relu2_decide(g, k)
    assert (index.cpu().numpy() == 0).all() and (stage.cpu().numpy() == 1).all()


# ------------------------------------------------- 6 DeviceGA, the drop-in ----
def test_device_ga_relu2_generations_and_checkpoint(gpu, tmp_path):
    from pong_amd import checkpoint
    from pong_amd.device import Evaluator
    from pong_amd.evolve import DeviceGA
    shape = [6, 16, 16, 3]
    ga = DeviceGA(shape, 256, device=gpu, schedule="selfplay", seed=9, activation="relu")
    assert ga.activation == "relu" and ga.ev.activation == "relu" and ga.ev.kernel == "auto"
    ga.initialize("normal", 1.0)
    exact = Evaluator(shape, device=gpu, activation="relu", kernel="general", seed=ga.ev.seed)
    checked = []

    def check(g, rows, opponents, res):
        n = res.fitness.shape[0]
        played = int(ga.last_count[0]) if ga.last_count is not None else n
        pt = torch.arange(played, device=gpu)
        r = ga.last_rows[pt].long() if ga.last_rows is not None else pt
        kind, opp, mult = ga.eval_schedule(g)
        ref, _ = exact.evaluate(rows[r].contiguous(), kind[:played].contiguous(), opp[:played].contiguous(),
                                mult[:played].contiguous(), opponents=opponents)
        torch.cuda.synchronize()
        assert torch.equal(res.fitness[:played], ref.fitness) and torch.equal(res.frames[:played], ref.frames)
        checked.append((g, played))

    ga.on_evaluate = check
    ga.step()
    ga.step()
    assert [g for g, _ in checked] == [0, 1] and checked[1][1] > 0
    ga.on_evaluate = None
    path = checkpoint.save(ga, str(tmp_path / "relu2.safetensors"))
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.activation == "relu" and list(ga2.nodes) == shape
    rec, rec2 = ga.step(), ga2.step()
    torch.cuda.synchronize()
    assert rec == rec2
    assert torch.equal(ga.population_full(), ga2.population_full()) and torch.equal(ga.fitness, ga2.fitness)


@pytest.fixture
def relu_dropin():
    """config.ACTIVATION = "relu" as a user sets it: numpy_nn initialises its
    activation_function from the knob when it is imported."""
    with dropin_config(activation="relu"):
        import numpy_nn
        yield numpy_nn


def test_dropin_evaluate_equals_general(gpu, relu_dropin, monkeypatch):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,16,16,2] ReLU network
    (AUTO: k_relu2) against the same call with the evaluator held to the
    general kernel: the same hall, the same random seed, the same fitness."""
    import main
    import utils
    assert relu_dropin.activation() == "relu"
    shape = [6, 16, 16, 2]
    rng = np.random.default_rng(77)
    G = M.genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]

        ev = main._evaluator()
        assert ev.activation == "relu" and list(ev.nodes) == shape and ev.kernel == "auto"
        got = dropin_fitness(hall, inds)
        monkeypatch.setattr(ev, "kernel", "general")
        assert main._evaluator() is ev
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
