"""k_sig2 on the MI355X (run with -m gpu): sigmoid networks with two hidden
layers, [6, 2..64, 2..64, 2..4] with bias, on the certified f32 game kernel
(PG_KERNEL_SIG2; pg_sig2_decide pins its decisions).

Checkers: pg_forward in f64 (numpy's order, the correctly rounded sigmoid) for
single decisions, numpy's own NeuralNetwork.run restated with np.dot where the
host's pow decides the case as numpy's does, the general kernel for whole
games, and the C oracle (which plays any sigmoid NETWORK_SHAPE)."""

import numpy as np
import pytest
import torch

import _sig2_model as M
from _gpu_support import assert_same, dev_genomes, dropin_config, dropin_fitness, ids, refused, run_both, same, schedule

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]


def _ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, **kw)


def _decide_both(ev, gpu, genomes, k, gidx):
    """sig2_decide and the f64 pg_forward on the same passes (genomes as ev's dtype holds them)."""
    gt, kt = dev_genomes(genomes, gpu, ev.dtype), torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.sig2_decide(gt, kt, genome_index=it)
    ref_idx, _ = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64", want_layers=True)
    z64 = ev.last_layers[0][:, -ev.nodes[-1]:]
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, stage, z32, bound, ref_idx, z64))


# ------------------------------------------------------- 1 random passes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_decide_random_passes(gpu, shape, dtype):
    """64 networks x 512 inputs (U[0,1), N(0,1), N(0,3) and N(0,30) genes): the
    decision is the f64 forward's on every pass and |z32 - z64| stays within the
    bound.  On the host test's N(0,1) passes the certificate decides at least
    the host model's share - 0.01."""
    f32 = dtype == torch.float32
    rng = np.random.default_rng(sum(shape) + 100)
    G = M.genes(shape)
    genomes = rng.standard_normal((64, G))
    genomes[:16] = rng.random((16, G))
    genomes[32:48] *= 3.0
    genomes[48:] *= 30.0
    if f32:
        genomes = genomes.astype(np.float32).astype(np.float64)  # the network the f32 population holds
    k = rng.integers(0, 321, size=(64 * 512, 6))
    gidx = np.repeat(np.arange(64), 512)
    ev = _ev(shape, gpu, dtype=dtype)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, genomes, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert np.isfinite(bound).all() and set(np.unique(stage)) <= {0, 1, 2, 3}
    want = M.bound_np(shape, genomes)[gidx]  # (the lanes' partial sums against a serial sum: to one f32 ulp)
    assert (np.abs(bound.astype(np.float64) - want) <= np.spacing(want)).all()
    ratio = np.abs(z32.astype(np.float64) - z64).max(axis=1) / bound
    print(f"{shape} {dtype}: largest |z32 - z64| / e {ratio.max():.4f}; stages "
          f"{[round(float(np.mean(stage == s)), 5) for s in range(4)]} of {len(stage)} passes")
    assert (ratio <= 1.0).all()
    # the certificate's share on the passes tests/test_sig2_host.py draws
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


@pytest.mark.parametrize("shape", [[6, 16, 16, 3], [6, 17, 33, 4], [6, 20, 32, 4], [6, 5, 4, 2]], ids=ids)
def test_decide_built_cases(gpu, shape):
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
    big[0, 5], big[1, a + 3], big[2, b + 1] = 1e30, -1e30, 1e30
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
    """n genomes whose every forward fails the f32 certificate: two outputs on one plateau, an exact tie, the
    all-zero genome and every output below -709.8, in turn (f32 values throughout)."""
    _, H1, H2, O = shape
    rows = []
    for i in range(n):
        if i % 4 == 0:
            g = _const_net(shape, rng, _pad([30.0, 30.0 + 1e-9], O))
        elif i % 4 == 1:
            g = _const_net(shape, rng, np.full(O, 1.0))
        elif i % 4 == 2:
            g = np.zeros(M.genes(shape))
        else:
            g = _const_net(shape, rng, np.array([-720.0, -715.0, -730.0, -711.0][:O]))
        rows.append(g)
    return np.array(rows).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_sig2_kernel_equals_general(gpu, shape, dtype):
    """k_sig2's decisions are the f64 forward's: every output array, the
    per-frame traces of the first 64 games and the step / forward / game
    counters equal the general kernel's; also on genomes whose every forward
    fails stage 1, and through genome_rows (a permutation) with n_active below n."""
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
    ev = _ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    hot, hot_tr = ev.evaluate(genomes, *sched, opponents=opponents, kernel="sig2", trace_games=64, trace_cap=2048)
    ref, ref_tr = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general", trace_games=64, trace_cap=2048)
    torch.cuda.synchronize()
    same(hot, ref)
    assert torch.equal(hot_tr, ref_tr) and int(hot_tr.any())
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all()
    assert ch[0] == int(ref.frames.sum()) and ch[3] == n * 6 and ch[8] == 0 and ch[12] == 0
    print(f"{shape} {dtype}: stage-1 failures {ch[4] / ch[1]:.5f}, f64 {ch[2] / ch[1]:.5f} of {ch[1]} forwards")
    assert ch[2] <= ch[4] < ch[1]
    # genomes and opponents whose every forward fails stage 1
    hard, hard_opp = dev_genomes(_hard_rows(shape, rng, 64), gpu, dtype), dev_genomes(_hard_rows(shape, rng, H), gpu, dtype)
    hsched = [t[:64].contiguous() for t in sched]
    hot_h, tr_h = ev.evaluate(hard, *hsched, opponents=hard_opp, kernel="sig2", trace_games=64, trace_cap=2048)
    ref_h, rtr_h = ev.evaluate(hard, *hsched, opponents=hard_opp, kernel="general", trace_games=64, trace_cap=2048)
    torch.cuda.synchronize()
    same(hot_h, ref_h)
    assert torch.equal(tr_h, rtr_h)
    chh = hot_h.counters.cpu().numpy()
    assert (chh[[0, 1, 3]] == ref_h.counters.cpu().numpy()[[0, 1, 3]]).all()
    assert chh[4] == chh[1] and 0 < chh[2] <= chh[4]
    # genome_rows as a permutation, n_active below n
    perm = torch.tensor(rng.permutation(n).astype(np.int32), device=gpu)
    act = torch.tensor([170], dtype=torch.int32, device=gpu)
    hot2, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="sig2", rows=perm, n_active=act)
    ref2, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general", rows=perm, n_active=act)
    whole, _ = ev.evaluate(genomes[perm.long()].contiguous(), *sched, opponents=opponents, kernel="sig2")
    torch.cuda.synchronize()
    same(hot2, ref2, 170)
    same(hot2, whole, 170)
    assert int(hot2.counters[3]) == 170 * 6 == int(ref2.counters[3])


@pytest.mark.parametrize("shape", [[6, 5, 4, 2], [6, 20, 32, 3], [6, 33, 17, 3]], ids=ids)
@pytest.mark.parametrize("dist", ["init", "n3"])
def test_sig2_matches_oracle(gpu, oracle, shape, dist):
    """One shape per layout against the C oracle at default limits: n = 97, H = 13 (ragged)."""
    rng = np.random.default_rng(sum(shape) + (0 if dist == "init" else 7))
    G = M.genes(shape)
    n, H = 97, 13
    draw = (lambda s: rng.random(s)) if dist == "init" else (lambda s: rng.standard_normal(s) * 3.0)
    genomes, opponents = draw((n, G)), draw((H, G))
    kinds, opp, mult = schedule(rng, n, 6, H)
    ev = _ev(shape, gpu, kernel="sig2")
    res, ref = run_both(ev, oracle, genomes, opponents, kinds, opp, mult, gpu)
    assert_same(res, ref)
    c = res.counters.cpu().numpy()
    assert c[0] == int(ref["frames"].sum()) and c[8] == 0 and c[12] == 0 and c[2] <= c[4] <= c[1]
    print(f"{shape} {dist}: stage-1 failures {c[4] / c[1]:.5f}, f64 {c[2] / c[1]:.5f} of {c[1]} forwards")


@pytest.mark.parametrize("shape,n,dtype", [([6, 16, 16, 3], 4096, torch.float64), ([6, 20, 32, 4], 1024, torch.float32),
                                           ([6, 64, 64, 3], 1024, torch.float64)], ids=ids)
def test_sig2_groups_play_several_games(gpu, shape, n, dtype):
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
    ev = _ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    hot, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="sig2")
    ref, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general")
    torch.cuda.synchronize()
    same(hot, ref)
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all() and ch[3] == n * 6 and ch[2] <= ch[4] < ch[1]


@pytest.mark.parametrize("shape", [[6, 2, 2, 2], [6, 17, 3, 3], [6, 33, 64, 4]], ids=ids)
def test_sig2_counter_flush(gpu, shape):
    """The shared game loop's flush of a family whose stages are 0..3: [2] the
    f64 forwards (stage 3) <= [4] the stage-1 failures (stage > 0) <= [1] the
    forwards.  The smallest padded shape of each layout (4, 16, 32 lanes), 8
    genomes x 2 games against hall rows so that both half-groups play; half of
    the rows fail stage 1 at every forward."""
    rng = np.random.default_rng(sum(shape) + 3)
    G = M.genes(shape)
    genomes = dev_genomes(np.concatenate([rng.standard_normal((4, G)), _hard_rows(shape, rng, 4)]), gpu, torch.float64)
    hall = dev_genomes(np.concatenate([rng.standard_normal((2, G)), _hard_rows(shape, rng, 2)]), gpu, torch.float64)
    sched = [torch.tensor(a, device=gpu) for a in (np.full((8, 2), 3, np.int32), rng.integers(0, 4, size=(8, 2)).astype(np.int32),
                                                   np.ones((8, 2)))]
    ev = _ev(shape, gpu, n_games=2, timeout_thresh=119, win_score=1)
    res, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="sig2")
    c = res.counters.cpu().numpy()
    print(f"{shape}: forwards {c[1]}, stage-1 failures {c[4]}, f64 {c[2]}")
    assert 0 < c[2] <= c[4] <= c[1]


# ------------------------------------------------------------ 4 refusals ----
def test_unsupported_combinations_are_refused(gpu):
    shape = [6, 16, 16, 3]
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    def genomes(ev):
        return torch.zeros((4, ev.genes), dtype=torch.float64, device=gpu)

    ev = _ev(shape, gpu)
    g = genomes(ev)
    relu = _ev(shape, gpu, activation="relu")
    refused(lambda: relu.evaluate(g, z, z, m, kernel="sig2"), "sigmoid")
    refused(lambda: relu.sig2_decide(g, k), "sigmoid")
    for other in ([6, 64, 3], [6, 65, 64, 3], [6, 64, 65, 3], [6, 1, 16, 2], [6, 16, 1, 2], [6, 8, 8, 8, 2]):
        eo = _ev(other, gpu)
        refused(lambda: eo.evaluate(genomes(eo), z, z, m, kernel="sig2"), "sig2")
        refused(lambda: eo.sig2_decide(genomes(eo), k), "sig2")
    nb = _ev(shape, gpu, bias=False)
    refused(lambda: nb.evaluate(genomes(nb), z, z, m, kernel="sig2"), "bias")
    refused(lambda: nb.sig2_decide(genomes(nb), k), "bias")
    refused(lambda: _ev(shape, gpu, precision="f64").evaluate(g, z, z, m, kernel="sig2"), "certified")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="sig2", horizon=1000), "horizon")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="sig2", hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)),
            "hard")
    # the supported neighbours of the refused calls still run; AUTO has not moved: it is the general kernel
    rng = np.random.default_rng(3)
    gr = dev_genomes(rng.standard_normal((4, ev.genes)) * 3.0, gpu)
    got = {kernel: ev.evaluate(gr, z, z, m, kernel=kernel)[0] for kernel in ("sig2", "general", "auto")}
    torch.cuda.synchronize()
    c = {kernel: r.counters.cpu().numpy() for kernel, r in got.items()}
    assert c["sig2"][3] == c["general"][3] == 24
    assert (c["auto"] == c["general"]).all()
    same(got["sig2"], got["general"])
    same(got["auto"], got["general"])
    index, stage, _, _ = ev.sig2_decide(g, k)  # all-zero genes: every output 0.5, index 0, decided in f64
    assert (index.cpu().numpy() == 0).all() and (stage.cpu().numpy() == 3).all()


# ------------------------------------------------- 5 DeviceGA, the drop-in ----
def test_device_ga_sig2_generations_and_checkpoint(gpu, tmp_path):
    from pong_amd import checkpoint
    from pong_amd.evolve import DeviceGA
    shape = [6, 16, 16, 3]
    runs = {}
    for kernel in ("sig2", "general"):
        ga = DeviceGA(shape, 64, device=gpu, seed=9, kernel=kernel)
        assert ga.ev.kernel == kernel and ga.ev.activation == "sigmoid"
        ga.initialize("normal", 1.0)
        history = [ga.step() for _ in range(3)]
        torch.cuda.synchronize()
        runs[kernel] = (ga, history, ga.hall_of_fame.clone(), ga.hof_member_fitness)
    (ga, hist, hall, hall_fit), (ga_g, hist_g, hall_g, hall_fit_g) = runs["sig2"], runs["general"]
    assert hist == hist_g  # the logbook
    assert torch.equal(hall, hall_g) and np.array_equal(hall_fit, hall_fit_g)
    assert torch.equal(ga.fitness, ga_g.fitness) and torch.equal(ga.population_full(), ga_g.population_full())
    assert int(ga.last.counters[1]) > 0 and int(ga.last.counters[4]) < int(ga.last.counters[1])  # k_sig2 played
    path = checkpoint.save(ga, str(tmp_path / "sig2.safetensors"))
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.activation == "sigmoid" and ga2.kernel == "sig2" == ga2.ev.kernel and list(ga2.nodes) == shape
    rec, rec2 = ga.step(), ga2.step()
    torch.cuda.synchronize()
    assert rec == rec2
    assert torch.equal(ga.population_full(), ga2.population_full()) and torch.equal(ga.fitness, ga2.fitness)


@pytest.fixture
def sig2_dropin():
    """config.KERNEL = "sig2" as a user sets it (the knob is read at each call; the activation is the default sigmoid)."""
    with dropin_config(activation="sigmoid", kernel="sig2"):
        import config
        yield config


def test_dropin_evaluate_equals_default(gpu, sig2_dropin):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,16,16,2] sigmoid network
    with config.KERNEL = "sig2" against the same call with the default KERNEL =
    "auto": the same hall, the same random seed, the same fitness."""
    import main
    import numpy_nn
    import utils
    config = sig2_dropin
    assert numpy_nn.activation() == "sigmoid"
    shape = [6, 16, 16, 2]
    rng = np.random.default_rng(79)
    G = M.genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]

        ev = main._evaluator()
        assert ev.activation == "sigmoid" and list(ev.nodes) == shape and ev.kernel == "sig2"
        got = dropin_fitness(hall, inds)
        config.KERNEL = "auto"
        ev_d = main._evaluator()
        assert ev_d is not ev and ev_d.kernel == "auto"
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
