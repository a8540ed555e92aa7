"""k_sig3 on the MI355X (run with -m gpu): sigmoid networks with three hidden
layers, [6, 2..32, 2..32, 2..32, 2..4] with bias, on the certified f32 game
kernel (PG_KERNEL_SIG3; pg_sig3_decide pins its decisions).

Checkers: pg_forward in f64 (numpy's order, the correctly rounded sigmoid) and
the CPU oracle's nn_run for single decisions, the gcc-compiled bound header for
the bound, the CPU oracle and the general kernel for whole games.  Every
comparison of a decision or a game is exact equality."""

import numpy as np
import pytest
import torch

import _sig3_cells as C
import _sig3_model as M
from _gpu_support import FIELDS, dev_genomes, dropin_config, dropin_fitness, ids, refused, same
from test_gpu_advance import DEFAULT, _assert_advance_equals_stepping
from test_gpu_modifier_instances import check_cell_population, oracle_result
from test_gpu_solo import _equal

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
KERNELS = ("sig3", "sig3+advance", "sig3+solo", "sig3+advance+solo")


def _ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, **kw)


def _decide_both(ev, gpu, genomes, k, gidx):
    """sig3_decide and the f64 pg_forward on the same passes (genomes as ev's dtype holds them)."""
    gt, kt = dev_genomes(genomes, gpu, ev.dtype), torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.sig3_decide(gt, kt, genome_index=it)
    ref_idx, _ = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64", want_layers=True)
    z64 = ev.last_layers[0][:, -ev.nodes[-1]:]
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, stage, z32, bound, ref_idx, z64))


# ------------------------------------------------------- 1 random passes ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_decide_random_passes(gpu, tmp_path, shape, dtype):
    """48 networks (16 each of U[0,1), N(0,1) and N(0,3) genes) x 64 inputs: the decision is the f64 forward's
    on every pass, |z32 - z64| stays within the returned bound, which is the gcc-compiled header's to one f32
    ulp, and the stages are the cascade's."""
    rng = np.random.default_rng(sum(shape) + 300)
    G = M.genes(shape)
    genomes = rng.standard_normal((48, G))
    genomes[:16] = rng.random((16, G))
    genomes[32:] *= 3.0
    if dtype == torch.float32:
        genomes = genomes.astype(np.float32).astype(np.float64)  # the network the f32 population holds
    per = 64
    k = rng.integers(0, 321, size=(48 * per, 6))
    gidx = np.repeat(np.arange(48), per)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(_ev(shape, gpu, dtype=dtype), gpu, genomes, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    assert np.isfinite(bound).all() and set(np.unique(stage)) <= {0, 1, 2, 3}
    want = M.bounds(tmp_path, shape, genomes)[gidx]  # (the lanes' partial sums against the serial loop: an f32 ulp)
    assert (np.abs(bound.view(np.int32) - want.view(np.int32)) <= 1).all()
    ratio = np.abs(z32.astype(np.float64) - z64).max(axis=1) / bound
    for name, rows in (("U[0,1)", gidx < 16), ("N(0,1)", (gidx >= 16) & (gidx < 32)), ("N(0,3)", gidx >= 32)):
        print(f"{shape} {dtype} {name}: largest |z32 - z64| / e {ratio[rows].max():.4f}; stages "
              f"{[round(float(np.mean(stage[rows] == s)), 4) for s in range(4)]} of {int(rows.sum())} passes")
    assert (ratio <= 1.0).all()


# ---------------------------------------------------------- 2 built cases ----
def _pad(b, O, fill=-5.0):
    return np.array(list(b) + [fill] * (O - len(b)))


@pytest.mark.parametrize("shape", [[6, 2, 2, 2, 2], [6, 16, 16, 16, 3], [6, 9, 32, 5, 3], [6, 32, 32, 32, 4]], ids=ids)
def test_decide_built_cases(gpu, oracle, shape):
    """Networks with zero output weights (every output pre-activation is its bias, exactly) around each rule of
    the cascade, and NaN, 1e30 and all-zero genes: every pass is decided as the CPU oracle's nn_run decides it and
    as pg_forward does, and each stage is taken by the cases built for it."""
    O = shape[-1]
    rng = np.random.default_rng(7 + sum(shape))
    ev = _ev(shape, gpu)
    G = M.genes(shape)
    starts = np.cumsum([0] + [(a + 1) * b for a, b in zip(shape[:-1], shape[1:])])[:4]
    cases = {}
    # z beyond 36.74 (53 ln 2): two saturated outputs tie at 1.0 and the first index wins, either order; an output
    # in the band around the threshold; a lone saturated output
    cases["saturated"] = [M.const_net(shape, rng, _pad(v, O)) for v in ([40.0, 38.0], [38.0, 40.0], [37.0, 36.74],
                                                                         [36.7368, 40.0], [36.0, 36.7368])]
    cases["lone"] = [M.const_net(shape, rng, _pad(v, O)) for v in ([40.0, 3.0], [3.0, 40.0])]
    # two outputs on one plateau (gap 1e-9: a tie, the lower index) and on adjacent ones (2^-52 e^z apart), z = 28 .. 35
    plateau = []
    for zc in (28.0, 30.0, 30.4, 33.0, 35.0):
        w = 2.0 ** -52 * np.exp(zc)
        plateau += [M.const_net(shape, rng, _pad(v, O)) for v in ([zc, zc + 1e-9], [zc + 1e-9, zc], [zc, zc + w],
                                                                  [zc + w, zc], [zc, zc + 3 * w], [zc + 40 * w, zc])]
    cases["plateau"] = plateau
    # the plateau regime's gap rule at its true width: gaps between 2^-52 e^z and 2^-50 e^z at z = 33
    cases["tight"] = [M.const_net(shape, rng, _pad(v, O), 0.01) for v in ([33.0, 33.0 - gap] for gap in
                                                                          (0.06, 0.08, 0.1, 0.12, 0.15))]
    # a near-tie below 22.2, inside 2e (e >= 8 u |b4|): no f32 rule can tell the two apart
    cases["near"] = [M.const_net(shape, rng, _pad(v, O)) for v in ([1.0, 1.0 + 1e-9], [1.0 + 1e-9, 1.0], [20.0, 20.0],
                                                                   [-3.0, -3.0 + 1e-8])]
    cases["low"] = [M.const_net(shape, rng, np.array([-720.0, -715.0, -730.0, -711.0][:O]))]
    big = rng.standard_normal((4, G))
    nan = rng.standard_normal((4, G))
    for i, at in enumerate(starts):
        big[i, at + 1], nan[i, at + 1] = (1e30, -1e30)[i % 2], np.nan
    cases["huge"], cases["nan"] = list(big), list(nan)
    cases["zero"] = [np.zeros(G)]
    cases["easy"] = [M.const_net(shape, rng, _pad([1.0, -1.0], O)), M.const_net(shape, rng, _pad([-2.0, 3.0], O))]
    names = [n for n, nets in cases.items() for _ in nets]
    nets = np.array([g for nets in cases.values() for g in nets])
    per = 8
    k = rng.integers(0, 321, size=(len(nets) * per, 6))
    gidx = np.repeat(np.arange(len(nets)), per)
    index, stage, z32, bound, ref_idx, z64 = _decide_both(ev, gpu, nets, k, gidx)
    np.testing.assert_array_equal(index, ref_idx)
    want = np.array([oracle.nn_run(nets[i], shape, (kk / 2) / 160)[0] for i, kk in zip(gidx, k)])
    np.testing.assert_array_equal(index, want)
    which = np.array(names)[gidx]
    seen = {n: sorted(set(stage[which == n].tolist())) for n in cases}
    print(f"{shape}: stages by case {seen}")
    sat = index[which == "saturated"].reshape(-1, per)
    assert (sat[0] == 0).all() and (sat[1] == 0).all() and (sat[2] == 0).all()  # ties at 1.0: the first index
    lone = index[which == "lone"].reshape(-1, per)
    assert (lone[0] == 0).all() and (lone[1] == 1).all() and seen["lone"] == [0]
    tie = index[which == "plateau"].reshape(-1, 6, per)
    assert (tie[:, 0] == 0).all() and (tie[:, 1] == 0).all()  # one plateau: a tie, the lower index
    assert (index[which == "low"] == 0).all() and (index[which == "zero"] == 0).all()
    zero = z64[which == "zero"]
    assert (zero == 0).all()  # (every output 0.5)
    assert np.isinf(bound[(which == "huge") | (which == "nan")]).all()
    assert np.isfinite(bound[(which != "huge") & (which != "nan")]).all()
    assert seen["easy"] == [0] and seen["huge"] == [3] and seen["nan"] == [3] and seen["zero"] == [3] and seen["low"] == [3]
    assert seen["near"] == [3]
    assert 1 in seen["tight"] and 2 in seen["plateau"]
    assert set(stage.tolist()) == {0, 1, 2, 3}  # every stage of the cascade occurs


# --------------------------------------------------------- 3 whole games ----
@pytest.mark.parametrize("cell", C.CELLS, ids=C.cell_id)
def test_sig3_instances_equal_the_oracle(gpu, oracle, cell):
    """A cell's population of 96 against a hall of 24 at the default 2000 / 3 on sig3, sig3+advance, sig3+solo,
    sig3+advance+solo and general: every output array is the CPU oracle's, the instance asked for is the one
    that runs, the advance and solo counters add up."""
    _, shape, genes = cell
    shape = list(shape)
    dtype = torch.float32 if genes == "f32" else torch.float64
    pop = C.cell_population(cell)
    genomes, members, kinds, opp, mult = pop
    ev = _ev(shape, gpu, dtype=dtype)
    kernels = KERNELS + ("general",)
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
    _assert_advance_equals_stepping("sig3", got["sig3+advance"], got["sig3"], got["general"], DEFAULT, what)
    _equal(got["sig3+solo"], got["sig3"], what + " +solo")
    _equal(got["sig3+advance+solo"], got["sig3+advance"], what + " +advance+solo")
    c, cg = got["sig3"].counters.cpu().numpy(), got["general"].counters.cpu().numpy()
    print(f"{what}: stage-1 failures {c[4] / c[1]:.5f}, f64 {c[2] / c[1]:.5f} of {c[1]} forwards")
    assert (c[[0, 1, 3]] == cg[[0, 1, 3]]).all() and c[2] <= c[4] < c[1]


def _hard_rows(shape, rng, n):
    """n genomes whose every forward fails the f32 certificate: two outputs on one plateau, an exact tie, the
    all-zero genome and every output below -709.8, in turn (f32 values throughout)."""
    O = shape[-1]
    rows = []
    for i in range(n):
        if i % 4 == 0:
            g = M.const_net(shape, rng, _pad([30.0, 30.0 + 1e-9], O))
        elif i % 4 == 1:
            g = M.const_net(shape, rng, np.full(O, 1.0))
        elif i % 4 == 2:
            g = np.zeros(M.genes(shape))
        else:
            g = M.const_net(shape, rng, np.array([-720.0, -715.0, -730.0, -711.0][:O]))
        rows.append(g)
    return np.array(rows).astype(np.float32).astype(np.float64)


def _sched(rng, n, hall, gpu):
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    return [torch.tensor(a, device=gpu) for a in (kinds, rng.integers(0, hall, size=(n, 6)).astype(np.int32),
                                                   np.round(rng.normal(size=(n, 6)), 3))]


@pytest.mark.parametrize("shape,n,dtype", [([6, 16, 16, 16, 3], 4096, torch.float64),
                                           ([6, 32, 32, 32, 4], 1024, torch.float32)], ids=ids)
def test_sig3_groups_play_several_games(gpu, shape, n, dtype):
    """More games than the launch has lane groups (2 blocks per CU of 16 or 8 groups), so every group takes
    further games from the queue and replaces its networks in place: still the general kernel's results, on
    every instance."""
    H = 64
    rng = np.random.default_rng(sum(shape) + 2 + n)
    G = M.genes(shape)
    groups = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count * (256 // (2 * M.lanes(shape)))
    assert n * 6 > 1.4 * groups
    genomes, opponents = dev_genomes(rng.standard_normal((n, G)), gpu, dtype), dev_genomes(rng.standard_normal((H, G)), gpu, dtype)
    sched = _sched(rng, n, H, gpu)
    ev = _ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    ref, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel="general")
    cr = ref.counters.cpu().numpy()
    for kernel in KERNELS:
        hot, _ = ev.evaluate(genomes, *sched, opponents=opponents, kernel=kernel)
        torch.cuda.synchronize()
        same(hot, ref, what=kernel)
        ch = hot.counters.cpu().numpy()
        assert ch[3] == cr[3] == n * 6 and ch[0] + ch[8] + ch[12] == cr[0] and ch[2] <= ch[4] < ch[1], kernel


# ------------------------------------------------ 4 lifecycle, interface ----
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [[6, 16, 16, 16, 3], [6, 9, 32, 5, 3]], ids=ids)
def test_traced_launch_equals_general(gpu, shape, dtype):
    """The per-frame traces of the first 64 games equal the general kernel's, also on genomes whose every
    forward fails the certificate; a traced sig3+advance launch runs with the advance off, counter for counter
    the stepping kernel; sig3+solo traced keeps solo on."""
    rng = np.random.default_rng(sum(shape) + 1)
    G = M.genes(shape)
    n, H = 128, 16
    rows = np.concatenate([rng.standard_normal((n - 32, G)), _hard_rows(shape, rng, 32)])
    hall = np.concatenate([rng.standard_normal((H - 4, G)), _hard_rows(shape, rng, 4)])
    genomes, opponents = dev_genomes(rng.permutation(rows), gpu, dtype), dev_genomes(hall, gpu, dtype)
    sched = _sched(rng, n, H, gpu)
    ev = _ev(shape, gpu, dtype=dtype, timeout_thresh=119, win_score=1)
    got = {k: ev.evaluate(genomes, *sched, opponents=opponents, kernel=k, trace_games=64, trace_cap=2048)
           for k in ("sig3", "sig3+advance", "sig3+solo", "general")}
    torch.cuda.synchronize()
    ref, ref_tr = got["general"]
    assert int(ref_tr.any())
    for k in ("sig3", "sig3+advance", "sig3+solo"):
        res, tr = got[k]
        same(res, ref, what=k)
        assert torch.equal(tr, ref_tr), k
        assert torch.equal(res.counters, got["sig3"][0].counters), k
    c, cr = got["sig3"][0].counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (c[[0, 1, 3]] == cr[[0, 1, 3]]).all() and c[8] == 0 and c[12] == 0 and 0 < c[2] <= c[4] < c[1]
    assert ev.resolved_kernel("sig3+advance", traced=True) == "sig3"
    assert ev.resolved_kernel("sig3+advance+solo", traced=True) == "sig3+solo"


@pytest.mark.parametrize("shape", [[6, 2, 2, 2, 2], [6, 2, 17, 2, 3]], ids=ids)
def test_sig3_counter_flush(gpu, shape):
    """The shared game loop's flush of a family whose stages are 0..3: [2] the f64 forwards (stage 3) <= [4] the
    stage-1 failures (stage > 0) <= [1] the forwards.  The smallest padded shape of each layout, 8 genomes x 2
    games against hall rows so that both half-groups play; half of the rows fail stage 1 at every forward."""
    rng = np.random.default_rng(sum(shape) + 3)
    G = M.genes(shape)
    genomes = dev_genomes(np.concatenate([rng.standard_normal((4, G)), _hard_rows(shape, rng, 4)]), gpu, torch.float64)
    hall = dev_genomes(np.concatenate([rng.standard_normal((2, G)), _hard_rows(shape, rng, 2)]), gpu, torch.float64)
    sched = [torch.tensor(a, device=gpu) for a in (np.full((8, 2), 3, np.int32), rng.integers(0, 4, size=(8, 2)).astype(np.int32),
                                                   np.ones((8, 2)))]
    ev = _ev(shape, gpu, n_games=2, timeout_thresh=119, win_score=1)
    res, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="sig3")
    ref, _ = ev.evaluate(genomes, *sched, opponents=hall, kernel="general")
    same(res, ref)
    c, cr = res.counters.cpu().numpy(), ref.counters.cpu().numpy()
    print(f"{shape}: forwards {c[1]}, stage-1 failures {c[4]}, f64 {c[2]}")
    assert 0 < c[2] <= c[4] <= c[1] == cr[1] and c[3] == 16 and c[8] == 0 and c[12] == 0


def test_unsupported_combinations_are_refused(gpu):
    shape = [6, 16, 16, 16, 3]
    z = torch.zeros((4, 6), dtype=torch.int32, device=gpu)
    m = torch.ones((4, 6), dtype=torch.float64, device=gpu)
    k = torch.zeros((4, 6), dtype=torch.int32, device=gpu)

    def genomes(ev):
        return torch.zeros((4, ev.genes), dtype=torch.float64, device=gpu)

    ev = _ev(shape, gpu)
    g = genomes(ev)
    relu = _ev(shape, gpu, activation="relu")
    refused(lambda: relu.evaluate(g, z, z, m, kernel="sig3"), "RELU3")
    refused(lambda: relu.sig3_decide(g, k), "sigmoid")
    for other in ([6, 33, 2, 2, 2], [6, 2, 2, 33, 2], [6, 1, 2, 2, 2], [6, 2, 2, 2, 5], [6, 8, 8, 3], [6, 8, 8, 8, 8, 3]):
        eo = _ev(other, gpu)
        for kernel in ("sig3", "sig3+advance+solo"):
            refused(lambda: eo.evaluate(genomes(eo), z, z, m, kernel=kernel), "sig3 kernel needs NETWORK_SHAPE")
        refused(lambda: eo.sig3_decide(genomes(eo), k), "sig3")
    nb = _ev(shape, gpu, bias=False)
    refused(lambda: nb.evaluate(genomes(nb), z, z, m, kernel="sig3"), "bias")
    refused(lambda: nb.sig3_decide(genomes(nb), k), "bias")
    refused(lambda: _ev(shape, gpu, precision="f64").evaluate(g, z, z, m, kernel="sig3"), "certified")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="sig3", horizon=1000), "horizon")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="sig3", hard_log=torch.zeros((8, 8), dtype=torch.int32, device=gpu)),
            "hard")
    refused(lambda: ev.evaluate(g, z, z, m, kernel="sig2"), "sig2")  # outside k_sig2's shapes
    # the supported neighbours of the refused calls still run; AUTO has not moved: it is the general kernel
    rng = np.random.default_rng(3)
    gr = dev_genomes(rng.standard_normal((4, ev.genes)) * 3.0, gpu)
    got = {kernel: ev.evaluate(gr, z, z, m, kernel=kernel)[0] for kernel in KERNELS + ("general", "auto", "auto+advance")}
    torch.cuda.synchronize()
    for kernel, res in got.items():
        assert int(res.counters[3]) == 24, kernel
        same(res, got["general"], what=kernel)
    assert (got["auto"].counters.cpu().numpy() == got["general"].counters.cpu().numpy()).all()
    assert ev.resolved_kernel("auto") == ev.resolved_kernel("auto+advance") == ev.resolved_kernel("auto+solo") == "general"
    index, stage, _, _ = ev.sig3_decide(g, k)  # all-zero genes: every output 0.5, index 0, decided in f64
    assert (index.cpu().numpy() == 0).all() and (stage.cpu().numpy() == 3).all()


def test_device_ga_sig3_generations_and_checkpoint(gpu, tmp_path):
    from pong_amd import checkpoint
    from pong_amd.evolve import DeviceGA
    shape = [6, 16, 16, 16, 3]
    runs = {}
    for kernel in ("sig3", "general"):
        ga = DeviceGA(shape, 64, device=gpu, seed=9, kernel=kernel)
        assert ga.ev.kernel == kernel and ga.ev.activation == "sigmoid"
        ga.initialize("normal", 1.0)
        history = [ga.step() for _ in range(3)]
        torch.cuda.synchronize()
        runs[kernel] = (ga, history, ga.hall_of_fame.clone(), ga.hof_member_fitness)
    (ga, hist, hall, hall_fit), (ga_g, hist_g, hall_g, hall_fit_g) = runs["sig3"], runs["general"]
    assert hist == hist_g  # the logbook
    assert torch.equal(hall, hall_g) and np.array_equal(hall_fit, hall_fit_g)
    assert torch.equal(ga.fitness, ga_g.fitness) and torch.equal(ga.population_full(), ga_g.population_full())
    assert int(ga.last.counters[1]) > 0 and int(ga.last.counters[4]) < int(ga.last.counters[1])  # k_sig3 played
    path = checkpoint.save(ga, str(tmp_path / "sig3.safetensors"))
    ga2 = checkpoint.load(path, device=gpu)
    assert ga2.activation == "sigmoid" and ga2.kernel == "sig3" == ga2.ev.kernel and list(ga2.nodes) == shape
    rec, rec2 = ga.step(), ga2.step()
    torch.cuda.synchronize()
    assert rec == rec2
    assert torch.equal(ga.population_full(), ga2.population_full()) and torch.equal(ga.fitness, ga2.fitness)


@pytest.fixture
def sig3_dropin():
    """config.KERNEL = "sig3" as a user sets it (the knob is read at each call; the activation is the default sigmoid)."""
    with dropin_config(activation="sigmoid", kernel="sig3"):
        import config
        yield config


def test_dropin_evaluate_equals_default(gpu, sig3_dropin):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,16,16,16,2] sigmoid network with config.KERNEL = "sig3"
    against the same call with the default KERNEL = "auto": the same hall, the same random seed, the same
    fitness."""
    import main
    import numpy_nn
    import utils
    config = sig3_dropin
    assert numpy_nn.activation() == "sigmoid"
    shape = [6, 16, 16, 16, 2]
    rng = np.random.default_rng(89)
    G = M.genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]
        ev = main._evaluator()
        assert ev.activation == "sigmoid" and list(ev.nodes) == shape and ev.kernel == "sig3"
        got = dropin_fitness(hall, inds)
        config.KERNEL = "auto"
        ev_d = main._evaluator()
        assert ev_d is not ev and ev_d.kernel == "auto"
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
