"""k_relu3 on the MI355X (run with -m gpu): ReLU networks with three hidden
layers, [6, 2..32, 2..32, 2..32, 2..4] with bias, on the certified f32 game
kernel (PG_KERNEL_RELU3; pg_relu3_decide pins its decisions).

Checkers: pg_forward in f64 and plain numpy for single decisions, the host
model (tests/_relu3_model.py) for the f32 chain, the CPU oracle and the general
kernel for whole games.  Every comparison is exact equality."""

import numpy as np
import pytest
import torch

import _relu3_cells as C
import _relu3_model as M
from _gpu_support import FIELDS, dev_genomes, dropin_config, dropin_fitness, ids, refused, same
from test_gpu_advance import DEFAULT, _assert_advance_equals_stepping
from test_gpu_modifier_instances import check_cell_population, oracle_result
from test_gpu_solo import _equal

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
DTYPES = [torch.float64, torch.float32]


def _relu_ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, activation="relu", **kw)


def _decide_both(ev, gpu, genomes, k, gidx):
    """relu3_decide and the f64 pg_forward on the same passes (genomes as ev's dtype holds them)."""
    gt, kt = dev_genomes(genomes, gpu, ev.dtype), torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.relu3_decide(gt, kt, genome_index=it)
    ref_idx, _ = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64", want_layers=True)
    z64 = ev.last_layers[0][:, -ev.nodes[-1]:]
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, stage, z32, bound, ref_idx, z64))


def _margin(z64):
    top = -np.sort(-z64, axis=1)
    return np.where(top[:, 0] <= 0, -top[:, 0], top[:, 0] - np.maximum(top[:, 1], 0.0))


# ------------------------------------------------------- 1 random passes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_decide_random_passes(gpu, shape, dtype):
    """64 networks (16 of them U[0,1)) x 512 inputs: the decision is the f64 forward's, |z32 - z64| stays within
    the (finite) bound, z32 is the host model's chain bit for bit on 8 inputs per network, every pass with a
    large f64 margin (> 1e-3 max_o S_o) is certified in f32, those are at least 30 % of all passes, and at most
    5 % of all passes take the f64 path."""
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
    np.testing.assert_array_equal(bound.reshape(64, 512)[:, 1:], bound.reshape(64, 512)[:, :1].repeat(511, axis=1))
    want_e = M.bound_numpy(shape, genomes)  # (the lanes' partial sums against the serial loop: an f32 ulp)
    assert (np.abs(bound[::512].view(np.int32) - want_e.view(np.int32)) <= 1).all()
    assert (np.abs(z32.astype(np.float64) - z64) <= bound[:, None]).all()
    s = M.s_max(shape, genomes)[gidx]
    large = _margin(z64) > 1e-3 * s
    assert set(np.unique(stage)) <= {0, 1}
    print(f"{shape} {dtype}: stage-1 share {np.mean(stage == 1):.5f} of {len(stage)} passes "
          f"({np.mean(large):.4f} with a large margin)")
    assert (stage[large] == 0).all()
    assert large.mean() >= 0.3
    assert np.mean(stage == 1) <= 0.05
    sub = (np.arange(64)[:, None] * 512 + np.arange(8)[None, :]).ravel()
    want = M.z32(shape, genomes, k[sub].reshape(64, 8, 6)).reshape(-1, shape[-1])
    np.testing.assert_array_equal(z32[sub].view(np.int32), want.view(np.int32))


# --------------------------------------------------------- 2 hard inputs ----
def _layer_starts(shape):
    at, out = 0, []
    for a, b in zip(shape[:-1], shape[1:]):
        out.append(at)
        at += (a + 1) * b
    return out


def _hard_nets(shape, rng):
    """(networks [N, G], whether the bound of each is inf): tie networks (equal output rows apart from a bias
    delta, down to one f64 ulp either way), the all-zero genome, a NaN gene in each layer, a 1e30 weight, a
    network where every output is <= 0, f32-subnormal genes."""
    G = M.genes(shape)
    nets, inf = [], []
    for d in (0.0, 1e-3, -1e-3, 1e-7, -1e-12):
        nets.append(M.tie_net(shape, d, rng))
        inf.append(False)
    for up in (True, False):  # the last output's bias one f64 ulp above / below the others'
        g = M.tie_net(shape, 0.0, rng)
        g[-1] = np.nextafter(g[-1], np.inf if up else -np.inf)
        nets.append(g)
        inf.append(False)
    nets.append(np.zeros(G))
    inf.append(False)
    for at in _layer_starts(shape):
        g = rng.standard_normal(G)
        g[at + 1] = np.nan
        nets.append(g)
        inf.append(True)
    g = rng.standard_normal(G)
    g[_layer_starts(shape)[2]] = 1e30
    nets.append(g)
    inf.append(True)
    ws = [w.copy() for w in M.split(shape, rng.standard_normal(G))]
    ws[-1][:, :-1] = -np.abs(ws[-1][:, :-1])  # h3 >= 0 times weights <= 0, biases < 0: every output <= 0
    ws[-1][:, -1] = -np.abs(ws[-1][:, -1]) - 0.5
    nets.append(M.pack(*ws))
    inf.append(False)
    nets.append(M.tiny_net(shape, rng))
    inf.append(False)
    return np.array(nets), np.array(inf)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [[6, 2, 2, 2, 2], [6, 16, 16, 16, 3], [6, 9, 32, 5, 3], [6, 32, 32, 32, 4]], ids=ids)
def test_decide_hard_inputs(gpu, shape, dtype):
    """Each hard network on 24 inputs is decided as numpy decides it (np.dot, np.maximum, np.argmax, pass by
    pass) and as pg_forward does; the stage is 1 wherever the bound is inf."""
    rng = np.random.default_rng(5 + sum(shape))
    nets, inf = _hard_nets(shape, rng)
    if dtype == torch.float32:
        with np.errstate(all="ignore"):
            nets = nets.astype(np.float32).astype(np.float64)  # (1e30 stays finite in f32; the ulp ties collapse to ties)
    m = 24
    k = rng.integers(0, 321, size=(len(nets), m, 6))
    k[:, 0], k[:, 1] = 0, 320
    gidx = np.repeat(np.arange(len(nets)), m)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(_relu_ev(shape, gpu, dtype=dtype), gpu, nets,
                                                          k.reshape(-1, 6), gidx)
    want = M.numpy_index(shape, nets, k).ravel()
    np.testing.assert_array_equal(index, want)
    np.testing.assert_array_equal(index, ref_idx)
    np.testing.assert_array_equal(np.isinf(bound), inf[gidx])
    assert (stage[inf[gidx]] == 1).all() and set(np.unique(stage)) <= {0, 1}
    zero = gidx == 7  # the all-zero genome: a tie at 0 under a bound of 0 + underflow, never certified
    assert (index[zero] == 0).all() and (stage[zero] == 1).all()
    neg = gidx == len(nets) - 2  # every output <= 0: index 0
    assert (z64[neg] <= 0).all() and (index[neg] == 0).all()
    print(f"{shape} {dtype}: stage-1 share on the tie networks {np.mean(stage[gidx < 7] == 1):.3f}")
    # a positive top output within 1e-7 of the next: no f32 certificate can tell them apart
    close = ((gidx == 0) | (gidx >= 3) & (gidx < 7)) & (z64.max(axis=1) > 0)
    assert close.any() and (stage[close] == 1).all()


# --------------------------------------------------------- 3 whole games ----
@pytest.mark.parametrize("cell", C.CELLS, ids=C.cell_id)
def test_relu3_instances_equal_the_oracle(gpu, oracle, cell):
    """A cell's population of 96 against a hall of 24 at the default 2000 / 3 on relu3, relu3+advance,
    relu3+solo, relu3+advance+solo and general: every output array is the CPU oracle's, the instance asked for
    is the one that runs, the advance and solo counters add up."""
    _, shape, genes = cell
    shape = list(shape)
    dtype = torch.float32 if genes == "f32" else torch.float64
    pop = C.cell_population(cell)
    genomes, members, kinds, opp, mult = pop
    ev = _relu_ev(shape, gpu, dtype=dtype)
    kernels = ("relu3", "relu3+advance", "relu3+solo", "relu3+advance+solo", "general")
    for k in kernels:  # no fallback to the base kernel
        assert ev.resolved_kernel(k) == k, (k, ev.resolved_kernel(k))
    args = [dev_genomes(genomes, gpu, dtype)] + [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    hall = dev_genomes(members, gpu, dtype)
    got = {k: ev.evaluate(*args, opponents=hall, kernel=k)[0] for k in kernels}
    torch.cuda.synchronize()
    ref = oracle_result(oracle, cell, pop, base_seed=ev.seed)
    shares = check_cell_population(oracle, cell, pop, ref, floors=C.FLOORS)
    what = C.cell_id(cell)
    print(f"{what}: seed {C.SEEDS[cell[1]]}, timed out {shares[0]:.3f}, by score {shares[1]:.3f}, "
          f"timed out after a point {shares[2]:.3f}")
    for k in kernels:
        for name in FIELDS:
            np.testing.assert_array_equal(getattr(got[k], name).cpu().numpy(), ref[name], err_msg=f"{what} {k} {name}")
    _assert_advance_equals_stepping("relu3", got["relu3+advance"], got["relu3"], got["general"], DEFAULT, what)
    _equal(got["relu3+solo"], got["relu3"], what + " +solo")
    _equal(got["relu3+advance+solo"], got["relu3+advance"], what + " +advance+solo")
    c, cg = got["relu3"].counters.cpu().numpy(), got["general"].counters.cpu().numpy()
    assert (c[[0, 1, 3]] == cg[[0, 1, 3]]).all() and c[2] == c[4] <= 0.25 * c[1]


def _f64_rows(shape, rng, n):
    """n genomes that always need the f64 path: tie, 1e30, all-zero and NaN, in turn (f32 values throughout)."""
    G = M.genes(shape)
    rows = []
    for i in range(n):
        if i % 4 == 0:
            g = M.tie_net(shape, 0.0, rng)
        elif i % 4 == 1:
            g = rng.standard_normal(G)
            g[_layer_starts(shape)[(i // 4) % 4]] = 1e30
        elif i % 4 == 2:
            g = np.zeros(G)
        else:
            g = rng.standard_normal(G)
            g[int(rng.integers(0, G))] = np.nan
        rows.append(g)
    return np.array(rows).astype(np.float32).astype(np.float64)


def _sched(rng, n, hall, gpu):
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    return [torch.tensor(a, device=gpu) for a in (kinds, rng.integers(0, hall, size=(n, 6)).astype(np.int32),
                                                   np.round(rng.normal(size=(n, 6)), 3))]


@pytest.mark.parametrize("n", [1024, 4096])
def test_relu3_groups_play_several_games(gpu, n):
    """[6,16,16,16,3] with 1 024 and 4 096 genomes (x 6 games).  At 4 096 the launch has fewer lane groups (2
    blocks per CU of 16) than games, so every group takes further games from the queue and replaces its
    networks in place: still the general kernel's results, on every instance."""
    shape, dtype, H = [6, 16, 16, 16, 3], torch.float64, 64
    rng = np.random.default_rng(sum(shape) + 2 + n)
    G = M.genes(shape)
    groups = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count * (256 // (2 * M.lanes(shape)))
    assert n < 4096 or n * 6 > 1.4 * groups
    genomes, opponents = dev_genomes(rng.standard_normal((n, G)), gpu, dtype), dev_genomes(rng.standard_normal((H, G)), gpu, dtype)
    sched = _sched(rng, n, H, gpu)
    ev = _relu_ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    ref, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general")
    cr = ref.counters.cpu().numpy()
    for kernel in ("relu3", "relu3+advance", "relu3+solo", "relu3+advance+solo"):
        hot, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel=kernel)
        torch.cuda.synchronize()
        same(hot, ref, what=kernel)
        ch = hot.counters.cpu().numpy()
        assert ch[3] == cr[3] == n * 6 and ch[0] + ch[8] + ch[12] == cr[0] and ch[2] == ch[4] <= 0.25 * ch[1], kernel


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [[6, 16, 16, 16, 3], [6, 9, 32, 5, 3]], ids=ids)
def test_traced_launch_equals_general(gpu, shape, dtype):
    """The per-frame traces of the first 64 games equal the general kernel's, also on genomes that always need
    the f64 path; a traced relu3+advance launch runs with the advance off, counter for counter the stepping
    kernel; relu3+solo traced keeps solo on."""
    rng = np.random.default_rng(sum(shape) + 1)
    G = M.genes(shape)
    n, H = 128, 16
    rows = np.concatenate([rng.standard_normal((n - 32, G)), _f64_rows(shape, rng, 32)])
    hall = np.concatenate([rng.standard_normal((H - 4, G)), _f64_rows(shape, rng, 4)])
    genomes, opponents = dev_genomes(rng.permutation(rows), gpu, dtype), dev_genomes(hall, gpu, dtype)
    sched = _sched(rng, n, H, gpu)
    ev = _relu_ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    got = {k: ev.evaluate(genomes, *sched, opponents=opponents, kernel=k, trace_games=64, trace_cap=2048)
           for k in ("relu3", "relu3+advance", "relu3+solo", "general")}
    torch.cuda.synchronize()
    ref, ref_tr = got["general"]
    assert int(ref_tr.any())
    for k in ("relu3", "relu3+advance", "relu3+solo"):
        res, tr = got[k]
        same(res, ref, what=k)
        assert torch.equal(tr, ref_tr), k
        assert torch.equal(res.counters, got["relu3"][0].counters), k
    c, cr = got["relu3"][0].counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (c[[0, 1, 3]] == cr[[0, 1, 3]]).all() and c[8] == 0 and c[12] == 0 and 0 < c[2] == c[4] < c[1]
    assert ev.resolved_kernel("relu3+advance", traced=True) == "relu3"
    assert ev.resolved_kernel("relu3+advance+solo", traced=True) == "relu3+solo"


def test_relu3_counter_flush(gpu):
    """The shared game loop's flush of a family whose stages are 0/1: one count of f64 forwards goes to both
    [2] and [4].  [6,2,2,2,2], 8 genomes x 2 games against hall rows so that both half-groups play; half of the
    rows always need the f64 path."""
    shape = [6, 2, 2, 2, 2]
    rng = np.random.default_rng(sum(shape) + 3)
    G = M.genes(shape)
    genomes = dev_genomes(np.concatenate([rng.standard_normal((4, G)), _f64_rows(shape, rng, 4)]), gpu, torch.float64)
    hall = dev_genomes(np.concatenate([rng.standard_normal((2, G)), _f64_rows(shape, rng, 2)]), gpu, torch.float64)
    sched = [torch.tensor(a, device=gpu) for a in (np.full((8, 2), 3, np.int32), rng.integers(0, 4, size=(8, 2)).astype(np.int32),
                                                   np.ones((8, 2)))]
    ev = _relu_ev(shape, gpu, n_games=2, timeout_thresh=119, win_score=1)
    res, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="relu3")
    ref, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="general")
    same(res, ref)
    c, cr = res.counters.cpu().numpy(), ref.counters.cpu().numpy()
    print(f"{shape}: forwards {c[1]}, f64 {c[2]}")
    assert 0 < c[2] == c[4] <= c[1] == cr[1] and c[3] == 16 and (c[5:] == 0).all()


# ------------------------------------------------------------ 4 refusals ----
def test_unsupported_combinations_are_refused(gpu):
    from pong_amd.device import Evaluator
    shape = [6, 16, 16, 16, 3]
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    def genomes(ev):
        return torch.zeros((4, ev.genes), dtype=torch.float64, device=gpu)

    ev = _relu_ev(shape, gpu)
    g = genomes(ev)
    sig = Evaluator(shape, device=gpu)
    refused(lambda: sig.evaluate(g, z, z, m, kernel="relu3"), "sigmoid")
    refused(lambda: sig.relu3_decide(g, k), "PG_ACT_RELU")
    for other in ([6, 33, 2, 2, 2], [6, 2, 2, 33, 2], [6, 1, 2, 2, 2], [6, 2, 2, 2, 5], [6, 8, 8, 3], [6, 8, 8, 8, 8, 3]):
        eo = _relu_ev(other, gpu)
        for kernel in ("relu3", "relu3+advance+solo"):
            refused(lambda: eo.evaluate(genomes(eo), z, z, m, kernel=kernel), "relu3 kernel needs NETWORK_SHAPE")
        refused(lambda: eo.relu3_decide(genomes(eo), k), "relu3")
    nb = _relu_ev(shape, gpu, bias=False)
    refused(lambda: nb.evaluate(genomes(nb), z, z, m, kernel="relu3"), "bias")
    refused(lambda: nb.relu3_decide(genomes(nb), k), "bias")
    refused(lambda: _relu_ev(shape, gpu, precision="f64").evaluate(g, z, z, m, kernel="relu3"), "certified")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu3", horizon=1000), "horizon")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu3", hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)),
            "hard")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="relu2"), "relu2")  # outside k_relu2's shapes
    refused(lambda: ev.relu2_decide(g, k), "relu2")
    # the supported neighbours of the refused calls still run; AUTO stays on the general kernel
    for kernel in ("relu3", "relu3+advance", "relu3+solo", "auto", "auto+advance", "general"):
        res, _ = ev.evaluate(g, z, z, m, kernel=kernel)
        assert int(res.counters[3]) == 24
    assert ev.resolved_kernel("auto") == ev.resolved_kernel("auto+advance") == ev.resolved_kernel("auto+solo") == "general"
    index, stage, _, _ = ev.relu3_decide(g, k)
    assert (index.cpu().numpy() == 0).all() and (stage.cpu().numpy() == 1).all()


# ------------------------------------------------- 5 DeviceGA, the drop-in ----
def test_device_ga_relu3_generations_and_checkpoint(gpu, tmp_path):
    from pong_amd import checkpoint
    from pong_amd.device import Evaluator
    from pong_amd.evolve import DeviceGA
    shape = [6, 16, 16, 16, 3]
    ga = DeviceGA(shape, 256, device=gpu, schedule="selfplay", seed=9, activation="relu", kernel="relu3")
    assert ga.activation == "relu" and ga.ev.activation == "relu" and ga.ev.kernel == "relu3"
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
        assert int(res.counters[4]) == int(res.counters[2]) < int(res.counters[1])  # the certified kernel played
        checked.append((g, played))

    ga.on_evaluate = check
    ga.step()
    ga.step()
    assert [g for g, _ in checked] == [0, 1] and checked[1][1] > 0
    ga.on_evaluate = None
    path = checkpoint.save(ga, str(tmp_path / "relu3.safetensors"))
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.activation == "relu" and list(ga2.nodes) == shape and ga2.ev.kernel == "relu3"
    rec, rec2 = ga.step(), ga2.step()
    torch.cuda.synchronize()
    assert rec == rec2
    assert torch.equal(ga.population_full(), ga2.population_full()) and torch.equal(ga.fitness, ga2.fitness)


@pytest.fixture
def relu3_dropin():
    """config.ACTIVATION = "relu" and config.KERNEL = "relu3" as a user sets them."""
    with dropin_config(activation="relu", kernel="relu3"):
        import config
        yield config


def test_dropin_evaluate_equals_general(gpu, relu3_dropin):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,16,16,16,2] ReLU network with config.KERNEL = "relu3"
    against the same call with "general": the same hall, the same random seed, the same fitness."""
    import main
    import utils
    config = relu3_dropin
    shape = [6, 16, 16, 16, 2]
    rng = np.random.default_rng(83)
    G = M.genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]
        ev = main._evaluator()
        assert ev.activation == "relu" and list(ev.nodes) == shape and ev.kernel == "relu3"
        got = dropin_fitness(hall, inds)
        config.KERNEL = "general"
        ev_b = main._evaluator()
        assert ev_b is not ev and ev_b.kernel == "general"
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
