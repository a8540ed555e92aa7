"""k_sig2_block on the MI355X (run with -m gpu): sigmoid networks with two
hidden layers of up to 128 units, [6, 2..128, 2..128, 2..4] with bias, on the
certified f32 kernel that gives a game a 256-thread block (PG_KERNEL_SIG2_BLOCK;
pg_sig2_block_decide pins its decisions).

Checkers: pg_forward in f64 (numpy's order, the correctly rounded sigmoid) for
single decisions, numpy's own NeuralNetwork.run restated with np.dot where the
host's pow decides the case as numpy's does, the bound's restatement and the
host model's certificate share (tests/_sig2_block_model.py), the general kernel
for whole games, k_sig2 on the shapes both kernels take, and the C oracle.  All
games but the oracle's run with timeout_thresh=119, win_score=1."""

import numpy as np
import pytest
import torch

import _sig2_block_model as M
from _gpu_support import assert_same, dev_genomes, dropin_config, dropin_fitness, ids, refused, run_both, same, schedule

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
EDGE_SHAPES = [[6, 2, 2, 2], [6, 65, 2, 2], [6, 2, 65, 3], [6, 100, 100, 3], [6, 128, 128, 4]]
GAME_SHAPES = [[6, 65, 2, 2], [6, 100, 100, 3], [6, 128, 128, 4]]


def _ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, **kw)


def _decide_both(ev, gpu, genomes, k, gidx):
    """sig2_block_decide and the f64 pg_forward on the same passes (genomes as ev's dtype holds them)."""
    gt, kt = dev_genomes(genomes, gpu, ev.dtype), torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.sig2_block_decide(gt, kt, genome_index=it)
    ref_idx, _ = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64", want_layers=True)
    z64 = ev.last_layers[0][:, -ev.nodes[-1]:]
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, stage, z32, bound, ref_idx, z64))


# ------------------------------------------------------- 1 random passes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.BLOCK_SHAPES, ids=ids)
def test_decide_random_passes(gpu, shape, dtype):
    """64 networks x 64 inputs (U[0,1), N(0,1), N(0,3) and N(0,30) genes): the
    decision is the f64 forward's on every pass, the bound the restatement's to
    one f32 ulp and |z32 - z64| within it.  On the host model's N(0,1) passes
    the certificate decides at least the host model's share - 0.01."""
    f32 = dtype == torch.float32
    rng = np.random.default_rng(sum(shape) + 200)
    G = M.genes(shape)
    genomes = rng.standard_normal((64, G))
    genomes[:16] = rng.random((16, G))
    genomes[32:48] *= 3.0
    genomes[48:] *= 30.0
    if f32:
        genomes = genomes.astype(np.float32).astype(np.float64)  # the network the f32 population holds
    k = rng.integers(0, 321, size=(64 * 64, 6))
    gidx = np.repeat(np.arange(64), 64)
    ev = _ev(shape, gpu, dtype=dtype)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, genomes, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert np.isfinite(bound).all() and set(np.unique(stage)) <= {0, 1, 2, 3}
    want = M.bound_np(shape, genomes)[gidx]  # (the threads' partial sums against a serial sum: to one f32 ulp)
    assert (np.abs(bound.astype(np.float64) - want) <= np.spacing(want)).all()
    ratio = np.abs(z32.astype(np.float64) - z64).max(axis=1) / bound
    print(f"{shape} {dtype}: largest |z32 - z64| / e {ratio.max():.4f}; stages "
          f"{[round(float(np.mean(stage == s)), 5) for s in range(4)]} of {len(stage)} passes")
    assert (ratio <= 1.0).all()
    # the certificate's share on the passes tests/test_sig2_block_host.py draws
    g1, k1 = M.n01_passes(shape, f32)
    gidx1 = np.repeat(np.arange(len(g1)), k1.shape[1])
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, g1, k1.reshape(-1, 6), gidx1)
    np.testing.assert_array_equal(index, ref_idx)
    assert (np.abs(z32.astype(np.float64) - z64) <= bound[:, None]).all()
    host, got = M.host_share(shape, f32), float(np.mean(stage == 0))
    print(f"{shape} {dtype}: stage-0 share on the N(0,1) passes: device {got:.4f}, host model {host:.4f}")
    assert got >= host - 0.01


# ---------------------------------------------------------- 2 built cases ----
def _const_net(shape, rng, b3, scale=1.0):
    """Random hidden layers and zero output weights: every output pre-activation is its bias b3 exactly."""
    _, H1, H2, O = shape
    w3 = np.zeros((O, H2 + 1))
    w3[:, H2] = b3
    return M.pack(rng.standard_normal((H1, 7)) * scale, rng.standard_normal((H2, H1 + 1)) * scale, w3)


def _pad(b, O, fill=-5.0):
    return np.array(list(b) + [fill] * (O - len(b)))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=ids)
def test_decide_built_cases(gpu, shape):
    """tests/test_gpu_sig2.py::test_decide_built_cases' constructions on the block layout's edge shapes."""
    _, H1, H2, O = shape
    rng = np.random.default_rng(5 + sum(shape))
    ev = _ev(shape, gpu)
    G = M.genes(shape)
    a, b = H1 * 7, H1 * 7 + H2 * (H1 + 1)
    cases = {}
    # two saturated outputs (a tie at 1.0: the first index wins), either order; an output in the band around 53 ln 2
    cases["saturated"] = [_const_net(shape, rng, _pad(v, O)) for v in ([40.0, 38.0], [38.0, 40.0], [37.0, 36.74],
                                                                         [36.7368, 40.0], [36.0, 36.7368])]
    # two outputs on one plateau (gap 1e-9) and on neighbouring ones (2^-52 e^z apart), z = 28 .. 35
    plateau = []
    for zc in (28.0, 30.0, 30.4, 33.0, 35.0):
        w = 2.0 ** -52 * np.exp(zc)
        plateau += [_const_net(shape, rng, _pad(v, O)) for v in ([zc, zc + 1e-9], [zc + 1e-9, zc], [zc, zc + w],
                                                                  [zc + w, zc], [zc, zc + 3 * w], [zc + 40 * w, zc])]
    cases["plateau"] = plateau
    # the plateau regime's gap rule at its true width: gaps between 2^-52 e^z and 2^-50 e^z at z = 33
    cases["tight"] = [_const_net(shape, rng, _pad(v, O), 0.01) for v in ([33.0, 33.0 - gap] for gap in
                                                                         (0.06, 0.08, 0.1, 0.12, 0.15))]
    cases["low"] = [_const_net(shape, rng, np.array([-720.0, -715.0, -730.0, -711.0][:O])),
                    _const_net(shape, rng, np.array([-800.0, -709.9, -750.0, -5000.0][:O]))]
    big = rng.standard_normal((3, G))
    big[0, 5], big[1, a + 1], big[2, b + 1] = 1e30, -1e30, 1e30
    cases["huge"] = list(big)
    nan = rng.standard_normal((3, G))
    nan[0, 2], nan[1, a + 1], nan[2, b + (H2 + 1)] = np.nan, np.nan, np.nan
    cases["nan"] = list(nan)
    cases["zero"] = [np.zeros(G)]
    cases["easy"] = [_const_net(shape, rng, _pad([1.0, -1.0], O)), _const_net(shape, rng, _pad([-2.0, 3.0], O))]
    names = [n for n, nets in cases.items() for _ in nets]
    nets = np.array([g for nets in cases.values() for g in nets])
    per = 16
    k = rng.integers(0, 321, size=(len(nets) * per, 6))
    gidx = np.repeat(np.arange(len(nets)), per)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, nets, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    which = np.array(names)[gidx]
    seen = {n: sorted(set(stage[which == n].tolist())) for n in cases}
    print(f"{shape}: stages by case {seen}")
    # numpy's own run where the case does not hang on the last bits of the host's pow
    for n in ("saturated", "low", "huge", "nan", "zero", "easy"):
        for i in np.flatnonzero(np.array(names) == n):
            rows = np.flatnonzero(gidx == i)
            np.testing.assert_array_equal(index[rows], M.run64(shape, nets[i], k[rows]), err_msg=f"{n} net {i}")
    sat = index[which == "saturated"].reshape(-1, per)
    assert (sat[0] == 0).all() and (sat[1] == 0).all() and (sat[2] == 0).all()  # ties at 1.0: the first index
    assert (index[which == "low"] == 0).all() and (index[which == "zero"] == 0).all()
    assert np.isinf(bound[(which == "huge") | (which == "nan")]).all()
    assert np.isfinite(bound[(which != "huge") & (which != "nan")]).all()
    assert seen["easy"] == [0] and seen["huge"] == [3] and seen["nan"] == [3] and seen["zero"] == [3] and seen["low"] == [3]
    assert 1 in seen["tight"] and 2 in seen["plateau"]
    assert set(stage.tolist()) == {0, 1, 2, 3}  # every stage of the cascade occurs


# --------------------------------------------------------- 3 whole games ----
def _hard_rows(shape, rng, n):
    """n genomes whose every forward fails stage 0: two outputs on one plateau, an exact tie (equal output rows),
    the all-zero genome, every output below -709.8, a genome over the cap and a NaN genome, in turn (f32 values)."""
    _, H1, H2, O = shape
    G = M.genes(shape)
    rows = []
    for i in range(n):
        if i % 6 == 0:
            g = _const_net(shape, rng, _pad([30.0, 30.0 + 1e-9], O))
        elif i % 6 == 1:
            g = _const_net(shape, rng, np.full(O, 1.0))
        elif i % 6 == 2:
            g = np.zeros(G)
        elif i % 6 == 3:
            g = _const_net(shape, rng, np.array([-720.0, -715.0, -730.0, -711.0][:O]))
        elif i % 6 == 4:
            g = rng.standard_normal(G)
            g[H1 * 7] = 1e30
        else:
            g = rng.standard_normal(G)
            g[int(rng.integers(0, G))] = np.nan
        rows.append(g)
    return np.array(rows).astype(np.float32).astype(np.float64)


def _population(shape, rng, n, gpu, dtype, hard=6):
    g = rng.standard_normal((n, M.genes(shape)))
    g[:hard] = _hard_rows(shape, rng, hard)
    return dev_genomes(g, gpu, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", GAME_SHAPES, ids=ids)
def test_kernel_equals_general(gpu, shape, dtype):
    """48 genomes x 6 games on the reference schedule (all four opponent kinds)
    and all self-play, with genomes whose every forward fails stage 0 (an
    over-cap and a NaN genome among them) in population and hall: fitness,
    rewards, scores, frames, total_frames, status and the traces equal the
    general kernel's bit for bit; every frame is stepped; also through
    genome_rows (a permutation) with n_active below n."""
    rng = np.random.default_rng(sum(shape) + 210)
    n, H = 48, 8
    genomes, hall = _population(shape, rng, n, gpu, dtype), _population(shape, rng, H, gpu, dtype)
    opp = rng.integers(0, H, size=(n, 6)).astype(np.int32)
    opp[:, 3] = np.arange(n) % 6  # the hard hall rows are met
    mult = np.round(rng.normal(size=(n, 6)), 3)
    ev = _ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    for kinds in ([0, 1, 2, 3, 3, 3], [3, 3, 3, 3, 3, 3]):
        sched = [torch.tensor(a, device=gpu) for a in (np.tile(np.array(kinds, np.int32), (n, 1)), opp, mult)]
        hot, hot_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="sig2_block", trace_games=n * 6, trace_cap=1024)
        ref, ref_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="general", trace_games=n * 6, trace_cap=1024)
        torch.cuda.synchronize()
        same(hot, ref)
        assert torch.equal(hot_tr, ref_tr) and int(hot_tr.any())
        ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
        assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all()
        assert ch[0] == int(ref.frames.sum()) and ch[3] == n * 6 and ch[8] == 0 and ch[12] == 0
        assert 0 < ch[2] <= ch[4] < ch[1]  # the hard rows fail stage 0, the certificate carries the rest
        print(f"{shape} {dtype} {kinds}: stage-0 failures {ch[4] / ch[1]:.5f}, f64 {ch[2] / ch[1]:.5f} of {ch[1]} forwards")
    perm = torch.tensor(rng.permutation(n).astype(np.int32), device=gpu)
    act = torch.tensor([31], dtype=torch.int32, device=gpu)
    hot2, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="sig2_block", rows=perm, n_active=act)
    ref2, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="general", rows=perm, n_active=act)
    whole, _ = ev.evaluate(genomes[perm.long()].contiguous(), *sched, opponents=hall, kernel="sig2_block")
    torch.cuda.synchronize()
    same(hot2, ref2, 31)
    same(hot2, whole, 31)
    assert int(hot2.counters[3]) == 31 * 6 == int(ref2.counters[3])


def test_blocks_reload_games_in_place(gpu):
    """One launch with at least twice as many games as the persistent grid has
    blocks (2 per CU), so every block takes further games from the queue and
    replaces both networks, their bounds and make_cert's constants in place:
    still the general kernel's results, and the games and steps counters are
    the sums over the results."""
    shape, dtype = [6, 65, 2, 2], torch.float32
    rng = np.random.default_rng(220)
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
    hot, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="sig2_block")
    ref, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="general")
    torch.cuda.synchronize()
    same(hot, ref)
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert ch[3] == n * 6 and ch[0] == int(hot.frames.sum()) and (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all()
    assert ch[8] == 0 and ch[12] == 0 and ch[2] <= ch[4] < ch[1]


@pytest.mark.parametrize("shape,law,n", [([6, 65, 33, 3], "init", 24), ([6, 65, 33, 3], "n3", 24),
                                         ([6, 128, 128, 3], "init", 8), ([6, 128, 128, 3], "n3", 8)], ids=ids)
def test_matches_oracle(gpu, oracle, shape, law, n):
    """Against the C oracle at the default limits (whole episodes to 21 points or the default timeout): a small
    ragged population, U[0,1) (ga.py's initial law) and N(0,3) genes; every array equal."""
    rng = np.random.default_rng(sum(shape) + (0 if law == "init" else 7) + 230)
    G = M.genes(shape)
    H = 5
    draw = (lambda s: rng.random(s)) if law == "init" else (lambda s: rng.standard_normal(s) * 3.0)
    genomes, opponents = draw((n, G)), draw((H, G))
    kinds, opp, mult = schedule(rng, n, 6, H)
    ev = _ev(shape, gpu, kernel="sig2_block")
    res, ref = run_both(ev, oracle, genomes, opponents, kinds, opp, mult, gpu)
    assert_same(res, ref)
    c = res.counters.cpu().numpy()
    assert c[0] == int(ref["frames"].sum()) and c[8] == 0 and c[12] == 0 and c[2] <= c[4] <= c[1]
    print(f"{shape} {law}: stage-0 failures {c[4] / c[1]:.5f}, f64 {c[2] / c[1]:.5f} of {c[1]} forwards")


@pytest.mark.parametrize("shape", [[6, 16, 16, 3], [6, 64, 64, 3]], ids=ids)
def test_overlap_with_sig2(gpu, shape):
    """On the shapes k_sig2 takes too, the outputs and the steps / forwards / games counters are k_sig2's."""
    rng = np.random.default_rng(sum(shape) + 240)
    n, H = 64, 8
    genomes, hall = _population(shape, rng, n, gpu, torch.float64), _population(shape, rng, H, gpu, torch.float64)
    sched = [torch.tensor(a, device=gpu) for a in (np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1)),
                                                   rng.integers(0, H, size=(n, 6)).astype(np.int32),
                                                   np.round(rng.normal(size=(n, 6)), 3))]
    ev = _ev(shape, gpu, timeout_thresh=119, win_score=1)
    hot, hot_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="sig2_block", trace_games=64, trace_cap=1024)
    ref, ref_tr = ev.evaluate(genomes, *sched, opponents=hall, kernel="sig2", trace_games=64, trace_cap=1024)
    torch.cuda.synchronize()
    same(hot, ref)
    assert torch.equal(hot_tr, ref_tr)
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all() and ch[3] == n * 6


# ------------------------------------------------------------ 4 refusals ----
def test_unsupported_combinations_are_refused(gpu):
    shape = [6, 128, 128, 3]
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    def genomes(ev):
        return torch.zeros((4, ev.genes), dtype=torch.float64, device=gpu)

    ev = _ev(shape, gpu)
    g = genomes(ev)
    relu = _ev(shape, gpu, activation="relu")
    refused(lambda: relu.evaluate(g, z, z, m, kernel="sig2_block"), "sigmoid")
    refused(lambda: relu.sig2_block_decide(g, k), "sigmoid")
    for other in ([6, 128, 3], [6, 129, 128, 3], [6, 128, 129, 3], [6, 1, 16, 2], [6, 16, 1, 2], [6, 8, 8, 8, 2]):
        eo = _ev(other, gpu)
        refused(lambda: eo.evaluate(genomes(eo), z, z, m, kernel="sig2_block"), "sig2_block kernel needs")
        refused(lambda: eo.sig2_block_decide(genomes(eo), k), "pg_sig2_block_decide")
    nb = _ev(shape, gpu, bias=False)
    refused(lambda: nb.evaluate(genomes(nb), z, z, m, kernel="sig2_block"), "bias")
    refused(lambda: nb.sig2_block_decide(genomes(nb), k), "bias")
    refused(lambda: _ev(shape, gpu, precision="f64").evaluate(g, z, z, m, kernel="sig2_block"), "certified")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="sig2_block", horizon=1000), "horizon")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="sig2_block", hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)),
            "hard")
    with pytest.raises(KeyError):
        ev.evaluate(g, z, z, m, kernel="sig2_block+advance")
    with pytest.raises(KeyError):
        ev.evaluate(g, z, z, m, kernel="sig2_block+solo")
    # the supported neighbours of the refused calls still run; AUTO has not moved: it is the wide kernel here
    assert ev.resolved_kernel() == "wide" and ev.resolved_kernel("sig2_block") == "sig2_block"
    rng = np.random.default_rng(3)
    gr = dev_genomes(rng.standard_normal((4, ev.genes)) * 3.0, gpu)
    got = {kernel: ev.evaluate(gr, z, z, m, kernel=kernel)[0] for kernel in ("sig2_block", "general", "auto")}
    torch.cuda.synchronize()
    assert int(got["sig2_block"].counters[3]) == int(got["general"].counters[3]) == 24
    same(got["sig2_block"], got["general"])
    same(got["auto"], got["general"])
    index, stage, _, _ = ev.sig2_block_decide(g, k)  # all-zero genes: every output 0.5, index 0, decided in f64
    assert (index.cpu().numpy() == 0).all() and (stage.cpu().numpy() == 3).all()


# ------------------------------------------------- 5 DeviceGA, the drop-in ----
def test_device_ga_generations_and_checkpoint(gpu, tmp_path):
    """DeviceGA(kernel="sig2_block") over three generations equals kernel="general", through a checkpoint round trip."""
    from pong_amd import checkpoint
    from pong_amd.evolve import DeviceGA
    shape = [6, 65, 8, 3]

    def make(kernel):
        ga = DeviceGA(shape, 64, device=gpu, schedule="selfplay", seed=9, kernel=kernel)
        ga.initialize("normal", 1.0)
        return ga

    ga, ref = make("sig2_block"), make("general")
    assert ga.ev.kernel == "sig2_block" and ga.ev.resolved_kernel() == "sig2_block" and ga.ev.activation == "sigmoid"
    for _ in range(2):
        assert ga.step() == ref.step()
    path = checkpoint.save(ga, str(tmp_path / "sig2_block.safetensors"))
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.kernel == "sig2_block" and ga2.activation == "sigmoid" and list(ga2.nodes) == shape
    rec, rec2, rec_ref = ga.step(), ga2.step(), ref.step()
    torch.cuda.synchronize()
    assert rec == rec2 == rec_ref
    for other in (ga2, ref):
        assert torch.equal(ga.population_full(), other.population_full()) and torch.equal(ga.fitness, other.fitness)
    assert int(ga.last.counters[1]) > 0 and int(ga.last.counters[4]) < int(ga.last.counters[1])  # the certificate played


@pytest.fixture
def sig2_block_dropin():
    """config.KERNEL = "sig2_block" as a user sets it (the knob is read at each call; the activation is the default sigmoid)."""
    with dropin_config(activation="sigmoid", kernel="sig2_block"):
        import config
        yield config


def test_dropin_evaluate_equals_general(gpu, sig2_block_dropin, monkeypatch):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,100,100,2] sigmoid network
    with config.KERNEL = "sig2_block" against the same call with the evaluator
    held to the general kernel: the same hall, the same random seed, the same fitness."""
    import main
    import numpy_nn
    import utils
    assert numpy_nn.activation() == "sigmoid"
    shape = [6, 100, 100, 2]
    rng = np.random.default_rng(78)
    G = M.genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((12, G))]

        ev = main._evaluator()
        assert ev.activation == "sigmoid" and list(ev.nodes) == shape and ev.kernel == "sig2_block"
        got = dropin_fitness(hall, inds)
        monkeypatch.setattr(ev, "kernel", "general")
        assert main._evaluator() is ev
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
