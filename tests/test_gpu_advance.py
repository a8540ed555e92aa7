"""PG_KERNEL_ADVANCE on the MI355X (run with -m gpu): k_relu_adv, k_relu2_adv and
k_sig2_adv -- the certified f32 families with serve delays and periodic rallies
advanced in closed form -- against their stepping kernels, the
general kernel and the C oracle.

The population is made of "noisy trackers" so that timeouts (periodic rallies)
and scored games occur side by side: two units of layer 1 compute
+-8 (me - ball_y) (features 4 and 1), each later layer passes them on (ReLU:
identity weights on units 0/1; sigmoid: +-4 (u0 - u1)), every other weight is 0,
and genome i = tracker + sigma_i N(0, 1) over all genes, sigma cycling through
0.3, 1, 3.  Every test asserts on its *reference* run that >= 5 % of the games
timed out, >= 50 % ended by score and >= 1 % timed out after a point, so a
population that stops exercising the advance fails loudly; the seeds were picked
so that the CPU oracle (for ReLU: oracle.eval_population(..., activation="relu"))
meets the three conditions at every shape and limit used here, and every ReLU
population's general-kernel result is compared with that oracle's (runs()).
At (timeout_thresh 32, win_score 1) every game times out at frame 34, just
after the first serve; that is asserted there in place of the three conditions.
"""

import numpy as np
import pytest
import torch

from _gpu_support import FIELDS, dev_genomes, dropin_config, dropin_fitness, ids, same

pytestmark = pytest.mark.gpu

SIGMAS = (0.3, 1.0, 3.0)
N, HALL = 192, 24
FAMILIES = {"relu": "relu", "relu2": "relu", "sig2": "sigmoid"}  # kernel name -> activation
# every family at the smallest padded shape of each of its layouts
SHAPES = {"relu": [[6, 2, 2], [6, 65, 3], [6, 129, 4]],
          "relu2": [[6, 2, 2, 2], [6, 17, 3, 3], [6, 33, 64, 4]],
          "sig2": [[6, 2, 2, 2], [6, 17, 3, 3], [6, 33, 64, 4]]}
F32_SHAPE = {"relu": [6, 65, 3], "relu2": [6, 17, 3, 3], "sig2": [6, 33, 64, 4]}
DEFAULT, SHORT, SERVE = (0, 0), (600, 2), (32, 1)  # (timeout_thresh, win_score); 0 = 2000 / 3
# the seed of a population where the default (the sum of the shape) leaves the three conditions little room on
# the CPU: the wider ReLU trackers time out in 4.6-6 % of their games under most seeds, in 6-10 % under these
SEEDS = {((6, 65, 3), "relu", N): 128, ((6, 129, 4), "relu", N): 114, ((6, 17, 3, 3), "relu", N): 57,
         ((6, 33, 64, 4), "relu", N): 50}


def _genes(shape):
    return sum((shape[i] + 1) * shape[i + 1] for i in range(len(shape) - 1))


def tracker(shape, activation):
    """The tracker network's genes: rows of [inputs..., bias] per unit, layer by layer."""
    layers = [np.zeros((shape[i + 1], shape[i] + 1)) for i in range(len(shape) - 1)]
    layers[0][0, 4], layers[0][0, 1] = 8.0, -8.0   # u0 = +8 (me - ball_y): positive when the paddle is below the ball
    layers[0][1, 4], layers[0][1, 1] = -8.0, 8.0   # u1 = -8 (me - ball_y)
    for w in layers[1:]:
        if activation == "relu":
            w[0, 0] = w[1, 1] = 1.0
        else:
            w[0, 0], w[0, 1], w[1, 0], w[1, 1] = 4.0, -4.0, -4.0, 4.0
    return np.concatenate([w.ravel() for w in layers])


def population(shape, activation, n=N, hall=HALL, seed=None):
    """(genomes [n, G], hall [hall, G], kinds, opp, mult [n, 6]) as numpy arrays."""
    if seed is None:
        seed = SEEDS.get((tuple(shape), activation, n), sum(shape))
    rng = np.random.default_rng(seed)
    base = tracker(shape, activation)

    def noisy(m):
        sigma = np.array(SIGMAS)[np.arange(m) % 3][:, None]
        return base[None, :] + sigma * rng.standard_normal((m, base.size))

    genomes, members = noisy(n), noisy(hall)
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    opp = rng.integers(0, hall, size=(n, 6)).astype(np.int32)
    mult = np.round(rng.normal(size=(n, 6)), 3)
    return genomes, members, kinds, opp, mult


def outcome_shares(scores, limits):
    """(timed out, ended by score, timed out after a point) as shares of the games."""
    win = min(limits[1] or 3, 21)
    s = np.asarray(scores).reshape(-1, 2)
    timed_out = (s < win).all(axis=1)
    return float(timed_out.mean()), float((~timed_out).mean()), float((timed_out & (s.sum(axis=1) > 0)).mean())


def _check_population(ref, limits, what):
    shares = outcome_shares(ref.scores.cpu().numpy(), limits)
    print(f"{what}: timed out {shares[0]:.3f}, by score {shares[1]:.3f}, timed out after a point {shares[2]:.3f}")
    if limits == SERVE:
        assert shares[0] == 1.0 and (ref.frames.cpu().numpy() == 34).all(), what
    else:
        assert shares[0] >= 0.05 and shares[1] >= 0.5 and shares[2] >= 0.01, (what, shares)


def _serves(res, limits):
    """Serves that followed a full delay: one per point, and the first one of a
    game that timed out (a game won on a point serves no more)."""
    win = min(limits[1] or 3, 21)
    s = res.scores.cpu().numpy().reshape(-1, 2)
    return int(s.sum() + (s < win).all(axis=1).sum())


def _assert_general_equals_oracle(ev, general, host, dtype, limits):
    """The general kernel's ReLU games are the CPU oracle's (activation="relu";
    pinned to the reference by tests/test_oracle_relu.py), f32 genes as rounded."""
    import oracle
    oracle.build()
    genomes, members, kinds, opp, mult = host
    if dtype == torch.float32:
        genomes, members = (a.astype(np.float32).astype(np.float64) for a in (genomes, members))
    ref = oracle.eval_population(genomes, ev.nodes, kinds, opp, mult, opponents=members, base_seed=ev.seed, n_threads=8,
                                 timeout_thresh=limits[0], win_score=limits[1], activation="relu")
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(general, name).cpu().numpy(), ref[name], err_msg=name)


_runs = {}


def runs(gpu, family, shape, dtype=torch.float64, limits=DEFAULT, n=N, hall=HALL):
    """(evaluator, the population on the device, {kernel: EvalResult}) of one population on
    family+advance, family and general; computed once and shared by the tests."""
    from pong_amd.device import Evaluator
    key = (family, tuple(shape), dtype, limits, n)
    if key not in _runs:
        act = FAMILIES[family]
        genomes, members, kinds, opp, mult = population(shape, act, n, hall)
        ev = Evaluator(shape, device=gpu, dtype=dtype, activation=act, timeout_thresh=limits[0], win_score=limits[1])
        data = dict(genomes=dev_genomes(genomes, gpu, dtype), opponents=dev_genomes(members, gpu, dtype),
                    sched=[torch.tensor(a, device=gpu) for a in (kinds, opp, mult)], host=(genomes, members, kinds, opp, mult))
        got = {k: ev.evaluate(data["genomes"], *data["sched"], opponents=data["opponents"], kernel=k)[0]
               for k in (family + "+advance", family, "general")}
        torch.cuda.synchronize()
        _check_population(got["general"], limits, f"{family} {shape} {dtype} {limits} n={n}")
        if act == "relu":
            _assert_general_equals_oracle(ev, got["general"], data["host"], dtype, limits)
        _runs[key] = (ev, data, got)
    return _runs[key]


def _assert_advance_equals_stepping(family, adv, base, ref, limits, what):
    same(adv, base, what=what)
    same(adv, ref, what=what)
    ca, cb = adv.counters.cpu().numpy(), base.counters.cpu().numpy()
    frames = int(ref.frames.sum())
    print(f"{what}: frames {frames}, stepped {ca[0]}, rally [8] {ca[8]} ({ca[8] / frames:.3f}), serve delays [12] "
          f"{ca[12]} ({ca[12] / frames:.3f}); forwards {ca[1]} of {cb[1]}")
    assert ca[3] == cb[3] == ref.frames.numel()
    assert ca[0] + ca[8] + ca[12] == frames == cb[0] and cb[8] == 0 and cb[12] == 0
    assert ca[1] <= cb[1] and ca[2] <= ca[4] <= ca[1]
    assert ca[12] == 29 * _serves(ref, limits)
    if limits == SERVE:
        assert ca[8] == 0  # no rally reaches its 8th return in the 4 frames after the serve
    else:
        assert ca[8] > 0 and ca[1] < cb[1]


# ------------------------------------------------- 0 the serve-delay count ----
def test_serve_delay_formula_on_the_split_kernel(gpu):
    """counters[12] = 29 per serve that followed a full delay, confirmed on
    k_service (kernel="split"), which has always advanced them: a sigmoid
    [6,2,2] population of this file's construction."""
    from pong_amd.device import Evaluator
    shape = [6, 2, 2]
    genomes, members, kinds, opp, mult = population(shape, "sigmoid")
    ev = Evaluator(shape, device=gpu)
    args = [dev_genomes(genomes, gpu)] + [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    got = {k: ev.evaluate(*args, opponents=dev_genomes(members, gpu), kernel=k)[0] for k in ("split", "general")}
    torch.cuda.synchronize()
    _check_population(got["general"], DEFAULT, f"split {shape}")
    same(got["split"], got["general"])
    c = got["split"].counters.cpu().numpy()
    assert c[12] == 29 * _serves(got["general"], DEFAULT) and c[8] > 0
    assert c[0] + c[8] + c[12] == int(got["general"].frames.sum())


# ------------------------------------------------------ 1 equals stepping ----
CASES = [(f, s, torch.float64) for f in FAMILIES for s in SHAPES[f]] + [(f, F32_SHAPE[f], torch.float32) for f in FAMILIES]


@pytest.mark.parametrize("family,shape,dtype", CASES, ids=ids)
def test_advance_equals_stepping(gpu, family, shape, dtype):
    """"X+advance" against "X" and "general" at default limits: every output
    array equal; [0] + [8] + [12] = the episodes' frames = the stepping kernel's
    [0]; fewer forwards; [8] > 0; [12] = 29 per serve."""
    _, _, got = runs(gpu, family, shape, dtype)
    _assert_advance_equals_stepping(family, got[family + "+advance"], got[family], got["general"], DEFAULT,
                                    f"{family} {shape} {dtype}")


def test_sig2_advance_matches_oracle(gpu, oracle):
    shape = [6, 2, 2, 2]
    ev, data, got = runs(gpu, "sig2", shape)
    genomes, members, kinds, opp, mult = data["host"]
    ref = oracle.eval_population(genomes, shape, kinds, opp, mult, opponents=members, base_seed=ev.seed, n_threads=8)
    res = got["sig2+advance"]
    for name in ("scores", "frames", "total_frames", "rewards", "fitness", "status"):
        np.testing.assert_array_equal(getattr(res, name).cpu().numpy(), ref[name], err_msg=name)


# --------------------------------------------------------------- 2 limits ----
@pytest.mark.parametrize("limits", [SHORT, SERVE], ids=ids)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_advance_under_other_limits(gpu, family, limits):
    """TIMEOUT_THRESH 600 / WIN_SCORE 2, and 32 / 1, where the timeout passes
    just after the first serve (frame 34: 29 advanced, 5 stepped)."""
    shape = SHAPES[family][0]
    _, _, got = runs(gpu, family, shape, limits=limits)
    _assert_advance_equals_stepping(family, got[family + "+advance"], got[family], got["general"], limits,
                                    f"{family} {shape} {limits}")


# ------------------------------------------------------ 3 traced launches ----
@pytest.mark.parametrize("family", list(FAMILIES))
def test_traced_launch_runs_with_the_advance_off(gpu, family):
    shape = SHAPES[family][0]
    ev, data, got = runs(gpu, family, shape)
    out = {k: ev.evaluate(data["genomes"], *data["sched"], opponents=data["opponents"], kernel=k, trace_games=96,
                          trace_cap=2048) for k in (family + "+advance", "general")}
    torch.cuda.synchronize()
    (adv, adv_tr), (ref, ref_tr) = out[family + "+advance"], out["general"]
    same(adv, ref)
    assert torch.equal(adv_tr, ref_tr) and int(adv_tr.any())
    c = adv.counters.cpu().numpy()
    assert c[8] == 0 and c[12] == 0 and c[0] == int(ref.frames.sum())
    assert (c == got[family].counters.cpu().numpy()).all()  # the stepping kernel, counter for counter


# -------------------------------------------------------------- 4 reloads ----
@pytest.mark.parametrize("family,shape,n", [("relu2", [6, 2, 2, 2], 4096), ("sig2", [6, 33, 64, 4], 1024)], ids=ids)
def test_groups_reload_games_with_a_fresh_search(gpu, family, shape, n):
    """More games than the launch has lane groups, so every group takes further
    games from the queue: a rally search left open by a group's previous game
    (its saved key, count and span) would make the next one jump early."""
    LN = 4 if max(shape[1:-1]) <= 16 else (16 if max(shape[1:-1]) <= 32 else 32)
    groups = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count * (256 // (2 * LN))
    assert n * 6 > 1.4 * groups
    _, _, got = runs(gpu, family, shape, n=n, hall=64)
    _assert_advance_equals_stepping(family, got[family + "+advance"], got[family], got["general"], DEFAULT,
                                    f"{family} {shape} n={n}")


# ----------------------------------------------------------------- 5 AUTO ----
@pytest.mark.parametrize("family,shape", [("relu", [6, 2, 2]), ("relu2", [6, 2, 2, 2])], ids=ids)
def test_auto_advance_in_the_relu_scopes(gpu, family, shape):
    ev, data, got = runs(gpu, family, shape)
    auto, _ = ev.evaluate(data["genomes"], *data["sched"], opponents=data["opponents"], kernel="auto+advance")
    torch.cuda.synchronize()
    same(auto, got[family + "+advance"])
    assert torch.equal(auto.counters, got[family + "+advance"].counters) and int(auto.counters[12]) > 0


@pytest.mark.parametrize("activation,shape,general", [("sigmoid", [6, 64, 3], False), ("relu", [6, 4, 4, 4, 2], True),
                                                      ("sigmoid", [6, 16, 16, 3], True)], ids=ids)
def test_auto_advance_changes_nothing_elsewhere(gpu, activation, shape, general):
    """Where AUTO resolves to SPLIT ([6,64,3] sigmoid) or GENERAL (a ReLU net
    outside k_relu's and k_relu2's scopes; a two-hidden-layer sigmoid net, which
    stays on GENERAL: SIG2 is chosen explicitly only) the bit changes nothing."""
    from pong_amd.device import Evaluator
    genomes, members, kinds, opp, mult = population(shape, activation, n=48, hall=8)
    ev = Evaluator(shape, device=gpu, activation=activation)
    args = [dev_genomes(genomes, gpu)] + [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    got = {k: ev.evaluate(*args, opponents=dev_genomes(members, gpu), kernel=k)[0]
           for k in ("auto+advance", "auto", "general")}
    torch.cuda.synchronize()
    same(got["auto+advance"], got["auto"])
    same(got["auto+advance"], got["general"])
    assert torch.equal(got["auto+advance"].counters, got["auto"].counters)
    c, cg = got["auto+advance"].counters.cpu().numpy(), got["general"].counters.cpu().numpy()
    if general:
        assert (c == cg).all() and c[8] == 0 and c[12] == 0
    else:
        assert c[12] > 0  # k_service, as ever


# ------------------------------------------------- 6 DeviceGA, the drop-in ----
def test_device_ga_auto_advance_generations(gpu):
    from pong_amd.evolve import DeviceGA
    shape = [6, 16, 3]
    out = {}
    for kernel in ("auto+advance", "auto"):
        ga = DeviceGA(shape, 64, device=gpu, seed=9, activation="relu", kernel=kernel)
        assert ga.ev.kernel == kernel and ga.ev.activation == "relu"
        ga.initialize("normal", 1.0)
        history = [ga.step() for _ in range(3)]
        torch.cuda.synchronize()
        out[kernel] = (ga, history, ga.hall_of_fame.clone(), ga.hof_member_fitness)
    (ga, hist, hall, hall_fit), (ga_b, hist_b, hall_b, hall_fit_b) = out["auto+advance"], out["auto"]
    assert hist == hist_b
    assert torch.equal(hall, hall_b) and np.array_equal(hall_fit, hall_fit_b)
    assert torch.equal(ga.fitness, ga_b.fitness) and torch.equal(ga.population_full(), ga_b.population_full())
    assert int(ga.last.counters[12]) > 0 and int(ga_b.last.counters[12]) == 0  # k_relu_adv played


@pytest.fixture
def relu_advance_dropin():
    """config.ACTIVATION = "relu" and config.KERNEL = "auto+advance" as a user sets them."""
    with dropin_config(activation="relu", kernel="auto+advance"):
        import config
        yield config


def test_dropin_evaluate_equals_auto(gpu, relu_advance_dropin):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,16,3] ReLU network with
    config.KERNEL = "auto+advance" against the same call with "auto": the same
    hall, the same random seed, the same fitness."""
    import main
    import utils
    config = relu_advance_dropin
    shape = [6, 16, 3]
    rng = np.random.default_rng(81)
    G = _genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]

        ev = main._evaluator()
        assert ev.activation == "relu" and list(ev.nodes) == shape and ev.kernel == "auto+advance"
        got = dropin_fitness(hall, inds)
        config.KERNEL = "auto"
        ev_b = main._evaluator()
        assert ev_b is not ev and ev_b.kernel == "auto"
        want = dropin_fitness(hall, inds)
        assert got == want and len(set(got)) >= 3
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
