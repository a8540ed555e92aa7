"""ReLU policy networks on the MI355X (run with -m gpu): activation_function =
ReLU (numpy_nn.py:6-9, 26) through pg_forward, the general kernel, the
certified f32 kernel k_relu (pg_relu_decide pins its decisions), the drop-in
modules and DeviceGA.

Checkers: the reference's own numbers (tests/golden/relu_forward.npz,
relu_evaluate.json, written by tests/golden/make_relu_golden.py), the numpy
loop (oracle/numpy_loop.py with its activation replaced by np.maximum(0.0, .))
for the exact path, and the exact path for the hot one."""
import random

import numpy as np
import pytest
import torch

from _gpu_support import HoF, Member, dev_genomes, dropin_config, gene_count, refused, same

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24


def _relu_ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, activation="relu", **kw)


# ------------------------------------------------------------ 1 pg_forward ----
@pytest.mark.parametrize("key", ["6x2x2", "6x16x2", "6x64x2", "6x64x64x2"])
@pytest.mark.parametrize("precision", ["certified", "f64"])
def test_forward_equals_reference(gpu, golden, key, precision):
    """NeuralNetwork.run of the reference with ReLU: the index, and the output
    activations bit for bit up to the sign of zero (no transcendental: every
    pre-activation is np.dot's, tests/test_gpu_blas_order.py)."""
    g = golden("relu_forward.npz")
    shape = [int(v) for v in g[f"{key}__shape"]]
    ev = _relu_ev(shape, gpu, precision=precision)
    idx, act = ev.forward(dev_genomes(g[f"{key}__genes"], gpu), dev_genomes(g[f"{key}__x"], gpu),
                          genome_index=torch.tensor(g[f"{key}__gidx"].astype(np.int32), device=gpu))
    np.testing.assert_array_equal(idx.cpu().numpy(), g[f"{key}__idx"])
    np.testing.assert_array_equal(act.cpu().numpy() + 0.0, g[f"{key}__act"] + 0.0)


# ------------------------------------------------- 2 games, the exact path ----
def _numpy_games(NL, shape, genomes, opponents, kinds, opp, mult, thresh, win):
    n, games = kinds.shape
    out = dict(fitness=np.zeros(n), rewards=np.zeros((n, games)), scores=np.zeros((n, games, 2), np.int32),
               frames=np.zeros((n, games), np.int32), total_frames=np.zeros((n, games)))
    for i in range(n):
        right = NL.NumpyNet(shape, genomes[i])
        rewards = []
        for g in range(games):
            k = int(kinds[i, g])
            left = (NL.NumpyNet(shape, opponents[int(opp[i, g])]) if k == 3
                    else NL.ScoreHardcoded() if k == 2 else NL.Hardcoded())
            env = NL._Env(NL.O.game_seed(0, g), k == 1)
            rew, f, s1, s2, tf = NL.perform_episode(env, left, right, float(mult[i, g]) if k == 3 else 1.0, thresh, win)
            rewards.append(rew)
            out["rewards"][i, g], out["frames"][i, g], out["total_frames"][i, g] = rew, f, tf
            out["scores"][i, g] = (s1, s2)
        out["fitness"][i] = sum(rewards) / float(games)  # main.py:66
    return out


@pytest.mark.parametrize("shape", [[6, 2, 2], [6, 16, 3], [6, 5, 4, 2], [6, 1, 2]])
def test_general_kernel_equals_numpy_loop(gpu, oracle, monkeypatch, shape):
    """k_general with ReLU against the reference's per-frame numpy loop, whole
    evaluate() calls at TIMEOUT_THRESH 119 / WIN_SCORE 1 (~70 frames a game);
    two hidden layers and a single hidden unit included: the general kernel is
    what tests/test_gpu_relu_instances.py trusts for whole games.
    A decision whose outputs are all <= 0 is an all-zero tie, index 0: it must
    have occurred.  It does in all four shapes (the numpy loop alone decides
    that: 635 of 2 656, 201 of 3 934, 832 of 2 408 and 622 of 2 284 decisions)."""
    import warnings

    import numpy_loop as NL
    monkeypatch.setattr(NL, "_sigmoid", lambda x: np.maximum(0.0, x))
    ties = [0, 0]
    run0 = NL.NumpyNet.run

    def run(self, x):
        r = run0(self, x)
        ties[0] += 1
        ties[1] += bool(self.acts[-1][:-1].max() <= 0)
        return r

    monkeypatch.setattr(NL.NumpyNet, "run", run)
    rng = np.random.default_rng(sum(shape))
    G = gene_count(shape)
    n, H = 8, 3
    genomes, opponents = rng.standard_normal((n, G)), rng.standard_normal((H, G))
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    opp = rng.integers(0, H, size=(n, 6)).astype(np.int32)
    mult = np.ones((n, 6))
    mult[:, 3:] = np.round(rng.normal(size=(n, 3)), 3)
    mult[0, 3] = -0.625
    ev = _relu_ev(shape, gpu, kernel="general", timeout_thresh=119, win_score=1)
    res, _ = ev.evaluate(dev_genomes(genomes, gpu), torch.tensor(kinds, device=gpu), torch.tensor(opp, device=gpu),
                         torch.tensor(mult, device=gpu), opponents=dev_genomes(opponents, gpu))
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # find_stuff's mean of an absent colour
        ref = _numpy_games(NL, shape, genomes, opponents, kinds, opp, mult, 119, 1)
    for name in ("scores", "frames", "total_frames", "rewards", "fitness"):
        np.testing.assert_array_equal(getattr(res, name).cpu().numpy(), ref[name], err_msg=name)
    assert not res.status.cpu().numpy().any()
    assert (mult < 0).any() and ties[1] > 0, ties
    print(f"{shape}: {ties[1]} of {ties[0]} decisions had every output <= 0")


# -------------------------------- 3 games, the hot path against the exact ----
@pytest.mark.parametrize("shape,dist,dtype", [([6, 64, 3], "n1", torch.float64), ([6, 16, 2], "init", torch.float64),
                                              ([6, 200, 4], "n1", torch.float32)])
def test_relu_kernel_equals_general(gpu, shape, dist, dtype):
    """k_relu's certified decisions are the f64 forward's: every output array,
    the per-frame traces of the first 64 games and the step / forward / game
    counters equal the general kernel's; also through genome_rows (a
    permutation) with n_active below n."""
    rng = np.random.default_rng(sum(shape))
    G = gene_count(shape)
    n, H = 1024, 64
    draw = (lambda s: rng.random(s)) if dist == "init" else (lambda s: rng.standard_normal(s))
    genomes, opponents = dev_genomes(draw((n, G)), gpu, dtype), dev_genomes(draw((H, G)), gpu, dtype)
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    opp = rng.integers(0, H, size=(n, 6)).astype(np.int32)
    mult = np.round(rng.normal(size=(n, 6)), 3)
    sched = [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    ev = _relu_ev(shape, gpu, dtype=dtype)
    got = {}
    for kernel in ("relu", "general", "auto"):
        got[kernel] = ev.evaluate(genomes, *sched, opponents=opponents, kernel=kernel, trace_games=64, trace_cap=2048)
    torch.cuda.synchronize()
    (hot, hot_tr), (ref, ref_tr), (auto, _) = got["relu"], got["general"], got["auto"]
    same(hot, ref)
    assert torch.equal(hot_tr, ref_tr) and int(hot_tr.any())
    ch, cr, ca = (r.counters.cpu().numpy() for r in (hot, ref, auto))
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all()
    assert ch[0] == int(ref.frames.sum()) and ch[3] == n * 6 and ch[8] == 0 and ch[12] == 0
    assert ch[2] == ch[4] <= ch[1]
    assert (ca == ch).all()  # AUTO resolves to k_relu in its scope
    print(f"{shape} {dist}: f64 share {ch[2] / ch[1]:.5f} of {ch[1]} forwards")
    # genome_rows as a permutation, n_active below n
    perm = torch.tensor(rng.permutation(n).astype(np.int32), device=gpu)
    act = torch.tensor([700], dtype=torch.int32, device=gpu)
    hot2, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="relu", rows=perm, n_active=act)
    ref2, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general", rows=perm, n_active=act)
    whole, _ = ev.evaluate(genomes[perm.long()].contiguous(), *sched, opponents=opponents, kernel="relu")
    torch.cuda.synchronize()
    same(hot2, ref2, 700)
    same(hot2, whole, 700)
    assert int(hot2.counters[3]) == 700 * 6 == int(ref2.counters[3])


# ------------------------------------------------------------ 4 relu_decide ----
def _s_max(shape, g):
    H, O = shape[1], shape[2]
    w1, w2 = np.abs(g[: H * 7].reshape(H, 7)), np.abs(g[H * 7:].reshape(O, H + 1))
    return (w2[:, :H] @ w1.sum(axis=1) + w2[:, H]).max()


def _decide_both(ev, gpu, genomes, k, gidx):
    gt, kt = dev_genomes(genomes, gpu), torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.relu_decide(gt, kt, genome_index=it)
    ref_idx, _ = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64", want_layers=True)
    z64 = ev.last_layers[0][:, -ev.nodes[-1]:]
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, stage, z32, bound, ref_idx, z64))


def test_relu_decide_random_passes(gpu):
    """64 networks x 512 inputs: the decision is the f64 forward's, |z32 - z64|
    stays within the bound, and every pass with a large f64 margin (> 1e-3
    max_o S_o, ~400 times the bound the derivation allows) is certified in f32."""
    shape = [6, 64, 3]
    rng = np.random.default_rng(4)
    G = gene_count(shape)
    genomes = rng.standard_normal((64, G))
    genomes[:16] = rng.random((16, G))
    k = rng.integers(0, 321, size=(64 * 512, 6))
    gidx = np.repeat(np.arange(64), 512)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(_relu_ev(shape, gpu), gpu, genomes, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert np.isfinite(bound).all()
    assert (np.abs(z32.astype(np.float64) - z64) <= bound[:, None]).all()
    s = np.array([_s_max(shape, g) for g in genomes])[gidx]
    assert (bound <= 64 * U32 * s).all()
    top = -np.sort(-z64, axis=1)
    margin = np.where(top[:, 0] <= 0, -top[:, 0], top[:, 0] - np.maximum(top[:, 1], 0.0))
    large = margin > 1e-3 * s
    assert large.mean() > 0.5 and (stage[large] == 0).all()
    assert set(np.unique(stage)) <= {0, 1}
    print(f"stage-0 share {np.mean(stage == 0):.5f} of {len(stage)} passes ({np.mean(large):.4f} with a large margin)")


def test_relu_decide_near_ties_zero_boundary_and_huge_weights(gpu):
    rng = np.random.default_rng(5)
    # (b) two equal output rows but for a bias difference delta, outputs > 0, S ~ 1
    shape = [6, 16, 2]
    H = 16
    deltas = [0.0, 1e-12, -1e-12, 1e-7, -1e-7, 1e-3, -1e-3]
    nets = []
    for d in deltas:
        w1 = rng.random((H, 7)) * 0.1
        row = np.append(rng.random(H) * 0.3, 0.125)
        nets.append(np.concatenate([w1.ravel(), row, row + np.append(np.zeros(H), d)]))
    nets = np.array(nets)
    assert all(0.3 < _s_max(shape, g) < 3 for g in nets)
    k = rng.integers(0, 321, size=(len(deltas) * 64, 6))
    gidx = np.repeat(np.arange(len(deltas)), 64)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(_relu_ev(shape, gpu), gpu, nets, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    d = np.array(deltas)[gidx]
    assert (z64 > 0).all()
    assert (index[d == 0] == 0).all() and (index[d > 0] == 1).all() and (index[d < 0] == 0).all()
    assert (stage[np.abs(d) <= 1e-7] == 1).all()
    # (c) the zero boundary: two outputs strongly negative, the third at +-1e-9
    shape = [6, 16, 3]
    nets = []
    for third in (1e-9, -1e-9):
        w1 = rng.standard_normal((H, 7))
        w2 = np.zeros((3, H + 1))
        w2[:2, :H] = -np.abs(rng.standard_normal((2, H)))
        w2[:2, H] = -5.0
        w2[2, H] = third
        nets.append(np.concatenate([w1.ravel(), w2.ravel()]))
    k = rng.integers(0, 321, size=(128, 6))
    gidx = np.repeat(np.arange(2), 64)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(_relu_ev(shape, gpu), gpu, np.array(nets), k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert (index[gidx == 0] == 2).all() and (index[gidx == 1] == 0).all() and (stage == 1).all()
    # (d) a weight f32 sums cannot hold: bound inf, always the f64 forward
    shape = [6, 64, 3]
    g = rng.standard_normal((2, gene_count(shape)))
    g[0, 5] = 1e30
    g[1, 64 * 7 + 3] = -1e30
    k = rng.integers(0, 321, size=(128, 6))
    gidx = np.repeat(np.arange(2), 64)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(_relu_ev(shape, gpu), gpu, g, k, gidx)
    assert np.isinf(bound).all() and (stage == 1).all()
    np.testing.assert_array_equal(index, ref_idx)


# ------------------------------------------------------------ 5 unsupported ----
def test_unsupported_combinations_are_refused(gpu):
    from pong_amd.device import Evaluator
    shape = [6, 64, 3]
    G = gene_count(shape)
    genomes = torch.zeros((4, G), dtype=torch.float64, device=gpu)
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    ev = _relu_ev(shape, gpu)
    refused(lambda: ev.evaluate(genomes, z, z, m, kernel="split"), "relu")
    refused(lambda: ev.evaluate(genomes, z, z, m, horizon=1000), "relu")
    refused(lambda: ev.evaluate(genomes, z, z, m, hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)), "relu")
    refused(lambda: ev.decide(genomes, k), "relu")
    wide = _relu_ev([6, 64, 64, 3], gpu, dtype=torch.float32)
    gw = torch.zeros((4, wide.genes), dtype=torch.float32, device=gpu)
    refused(lambda: wide.evaluate(gw, z, z, m, kernel="wide"), "relu")
    refused(lambda: wide.wide_decide(gw, k), "relu")
    refused(lambda: wide.evaluate(gw, z, z, m, kernel="relu"), "relu")  # outside k_relu's shapes
    refused(lambda: _relu_ev(shape, gpu, precision="f64").evaluate(genomes, z, z, m, kernel="relu"), "certified")
    sig = Evaluator(shape, device=gpu)
    refused(lambda: sig.evaluate(genomes, z, z, m, kernel="relu"), "sigmoid")
    refused(lambda: sig.relu_decide(genomes, k), "PG_ACT_RELU")
    # the supported neighbours of the refused calls still run
    res, _ = ev.evaluate(genomes, z, z, m)
    assert int(res.counters[3]) == 24


# ---------------------------------------------------------------- 6 drop-in ----
@pytest.fixture
def relu_dropin():
    """config.ACTIVATION = "relu" as a user sets it: numpy_nn initialises its
    activation_function from the knob when it is imported."""
    with dropin_config(activation="relu"):
        import numpy_nn
        yield numpy_nn


def test_dropin_evaluate_matches_reference(gpu, golden, relu_dropin):
    """relu_evaluate.json: the fitness of the REAL evaluate() with
    activation_function = ReLU, through ga.toolbox.map / main.evaluate."""
    import ga
    import main
    import utils
    assert relu_dropin.activation() == "relu" and main.numpy_nn is relu_dropin
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        for case in golden("relu_evaluate.json"):
            assert len(set(case["fitness"])) >= 3 and min(case["hof_fitness"]) < 0
            utils.NETWORK_SHAPE = case["shape"]
            main.hall_of_fame = HoF([Member(g, f) for g, f in zip(case["hof_genes"], case["hof_fitness"])])
            random.seed(case["random_seed"])
            inds = [list(g) for g in case["individuals"]]
            got = [fit[0] for fit in ga.toolbox.map(ga.toolbox.evaluate, inds)]
            assert got == case["fitness"]
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved


def test_dropin_network_run_matches_reference(gpu, golden, relu_dropin):
    g = golden("relu_forward.npz")
    for key in ("6x16x2", "6x64x64x2"):
        shape = [int(v) for v in g[f"{key}__shape"]]
        for s in range(0, len(g[f"{key}__x"]), 41):
            net = relu_dropin.NeuralNetwork(nodes=shape, weights=list(g[f"{key}__genes"][g[f"{key}__gidx"][s]]), bias=True)
            assert net.run(list(g[f"{key}__x"][s])) == list(g[f"{key}__run"][s])
            np.testing.assert_array_equal(net.list_of_transitional_arrays[-1][:-1] + 0.0, g[f"{key}__act"][s] + 0.0)
    # the reference's one-line switch, thrown back and forth at run time
    net = relu_dropin.NeuralNetwork(nodes=[6, 16, 2], weights=list(g["6x16x2__genes"][5]), bias=True)
    x = list(g["6x16x2__x"][5 * 32])
    net.run(x)
    relu_act = net.list_of_transitional_arrays[-1][:-1].copy()
    relu_dropin.activation_function = relu_dropin.sigmoid
    net.run(x)
    assert (net.list_of_transitional_arrays[-1][:-1] != relu_act).any()
    assert ((0 < net.list_of_transitional_arrays[-1][:-1]) & (net.list_of_transitional_arrays[-1][:-1] < 1)).all()


# --------------------------------------------------------------- 7 DeviceGA ----
def test_device_ga_relu_generations_and_checkpoint(gpu, tmp_path):
    from pong_amd import checkpoint
    from pong_amd.device import Evaluator
    from pong_amd.evolve import DeviceGA
    shape = [6, 16, 3]
    ga = DeviceGA(shape, 256, device=gpu, schedule="selfplay", seed=9, activation="relu")
    assert ga.activation == "relu" and ga.ev.activation == "relu"
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
    path = checkpoint.save(ga, str(tmp_path / "relu.safetensors"))
    assert checkpoint._config(ga)["activation"] == "relu"
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.activation == "relu" and ga2.ev.activation == "relu"
    rec, rec2 = ga.step(), ga2.step()
    torch.cuda.synchronize()
    assert rec == rec2
    assert torch.equal(ga.population_full(), ga2.population_full()) and torch.equal(ga.fitness, ga2.fitness)
