"""PG_KERNEL_SOLO on the MI355X (run with -m gpu): k_relu_solo, k_relu2_solo,
k_sig2_solo and their _adv_solo twins -- a game against a scripted opponent on
half a lane group, a game against a hall-of-fame row on a whole one (DESIGN.md
4.2i) -- against their base kernels and the general kernel.

"Equal" means torch.equal on fitness, rewards, scores, frames, total_frames and
status, and (against the base kernel) equality of all 16 counters.  The
populations, shapes and limits are test_gpu_advance's: 192 noisy trackers and a
hall of 24, rows below 96 playing kinds [0,1,2,3,3,3] and the rest all-NN.
"""

import numpy as np
import pytest
import torch

from _gpu_support import FIELDS, dev_genomes, dropin_config, dropin_fitness, ids
from test_gpu_advance import DEFAULT, F32_SHAPE, FAMILIES, SERVE, SHAPES, SHORT, _genes, population, runs

pytestmark = pytest.mark.gpu

NN = 3  # PG_OPP_NN
ONE_SHAPE = {"relu": [6, 65, 3], "relu2": [6, 17, 3, 3], "sig2": [6, 17, 3, 3]}  # the 8- and 16-lane layouts


def _equal(a, b, what="", counters=True):
    for name in FIELDS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (name, what)
    if counters:
        assert torch.equal(a.counters, b.counters), (what, a.counters.tolist(), b.counters.tolist())


def _play(ev, data, kernel, **kw):
    return ev.evaluate(data["genomes"], *data["sched"], opponents=data["opponents"], kernel=kernel, **kw)


def _assert_solo_equals_base(ev, data, family, base, base_adv, general, what):
    """X+solo = X (outputs, counters) = general (outputs); X+advance+solo = X+advance."""
    solo, _ = _play(ev, data, family + "+solo")
    both, _ = _play(ev, data, family + "+advance+solo")
    swapped, _ = _play(ev, data, family + "+solo+advance")
    torch.cuda.synchronize()
    _equal(solo, base, what)
    _equal(solo, general, what, counters=False)
    _equal(both, base_adv, what)
    _equal(swapped, base_adv, what)
    c = solo.counters.cpu().numpy()
    assert c[3] == general.frames.numel() and c[0] == int(general.frames.sum()) and c[8] == 0 and c[12] == 0
    return solo, both


# ------------------------------------------------- 1 the smallest shapes ----
CASES = [(f, s, torch.float64) for f in FAMILIES for s in SHAPES[f]] + [(f, F32_SHAPE[f], torch.float32) for f in FAMILIES]


@pytest.mark.parametrize("family,shape,dtype", CASES, ids=ids)
def test_solo_equals_base(gpu, family, shape, dtype):
    ev, data, got = runs(gpu, family, shape, dtype)
    kinds = data["host"][2]
    frames = got["general"].frames.cpu().numpy()
    # the population plays solo games and NN games, and the solo games differ in length
    assert (kinds != NN).any() and (kinds == NN).any() and len(np.unique(frames[kinds != NN])) > 1
    _assert_solo_equals_base(ev, data, family, got[family], got[family + "+advance"], got["general"],
                             f"{family} {shape} {dtype}")


# ------------------------------------------------------------ 2 schedules ----
def _custom(gpu, family, shape, kinds, n_games=6, with_hall=True, n=None, hall=8):
    """(evaluator, device data) of test_gpu_advance's population under another schedule."""
    from pong_amd.device import Evaluator
    kinds = np.asarray(kinds, np.int32)
    n = kinds.shape[0] if n is None else n
    act = FAMILIES[family]
    genomes, members, _, opp, mult = population(shape, act, n, hall)
    ev = Evaluator(shape, device=gpu, activation=act, n_games=n_games)
    sched = [torch.tensor(np.ascontiguousarray(a[:, :n_games]), device=gpu) for a in (kinds, opp, mult)]
    data = dict(genomes=dev_genomes(genomes, gpu), opponents=dev_genomes(members, gpu) if with_hall else None, sched=sched)
    return ev, data


def _all_kernels(ev, data, family, what):
    got = {k: _play(ev, data, k)[0] for k in (family, family + "+advance", "general")}
    return _assert_solo_equals_base(ev, data, family, got[family], got[family + "+advance"], got["general"], what)


@pytest.mark.parametrize("schedule", ["scripted", "nn", "one_solo"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_solo_schedules(gpu, family, schedule):
    """All scripted (no hall at all: generation 0), all NN (the solo queue is
    walked and holds nothing), and exactly one solo game among NN games."""
    n = 48
    if schedule == "scripted":
        kinds = np.tile(np.array([0, 1, 2, 0, 2, 1], np.int32), (n, 1))
    else:
        kinds = np.full((n, 6), NN, np.int32)
        if schedule == "one_solo":
            kinds[5, 2] = 1
    ev, data = _custom(gpu, family, ONE_SHAPE[family], kinds, with_hall=schedule != "scripted")
    _all_kernels(ev, data, family, f"{family} {schedule}")


@pytest.mark.parametrize("kind", [0, NN])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_solo_one_game_launch(gpu, family, kind):
    """One genome, one game: one block, and (kind 0) one half-group of it playing."""
    ev, data = _custom(gpu, family, ONE_SHAPE[family], [[kind]], n_games=1)
    solo, _ = _all_kernels(ev, data, family, f"{family} one game of kind {kind}")
    assert int(solo.counters[3]) == 1 and int(solo.frames[0, 0]) > 30


# -------------------------------------------------------------- 3 reloads ----
@pytest.mark.parametrize("family,shape,n", [("relu", [6, 2, 2], 4096), ("relu2", [6, 2, 2, 2], 4096),
                                            ("sig2", [6, 33, 64, 4], 1024)], ids=ids)
def test_groups_reload_and_pass_from_pair_to_solo_games(gpu, family, shape, n):
    """More NN games than the launch has lane groups, so groups reload pair
    games and later pass on to solo games, each half on its own.  No counter
    shows it, so the arithmetic: the grid is min(ceil(games / G), 2 CUs) blocks
    of G = 256 / (2 LN) groups -- on the MI355X's 256 CUs 512 blocks: 16 384
    groups of 8 lanes (LN = 4), 2 048 groups of 64 (LN = 32).  With the mixed
    schedule n x 6 games are n / 2 x 3 + n / 2 x 6 = 4.5 n NN games and 1.5 n
    solo games: n = 4 096 gives 18 432 NN games on 16 384 groups and 6 144 solo
    games on 32 768 half-groups; n = 1 024 gives 4 608 NN games on 2 048 groups
    and 1 536 solo games on 4 096 half-groups."""
    LN = 4 if max(shape[1:-1]) <= 16 else (16 if max(shape[1:-1]) <= 32 else 32)
    groups = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count * (256 // (2 * LN))
    if family == "relu":  # (not one of test_gpu_advance's reload populations: its outcome shares are not asserted)
        kinds = population(shape, "relu", n, 64)[2]
        ev, data = _custom(gpu, family, shape, kinds, hall=64)
        got = {k: _play(ev, data, k)[0] for k in (family, family + "+advance", "general")}
    else:
        ev, data, got = runs(gpu, family, shape, n=n, hall=64)
        kinds = data["host"][2]
    assert (kinds == NN).sum() > 1.1 * groups and (kinds != NN).sum() > 0
    _assert_solo_equals_base(ev, data, family, got[family], got[family + "+advance"], got["general"],
                             f"{family} {shape} n={n}")


# --------------------------------------------------------------- 4 limits ----
@pytest.mark.parametrize("limits", [SHORT, SERVE], ids=ids)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_solo_under_other_limits(gpu, family, limits):
    shape = SHAPES[family][0]
    ev, data, got = runs(gpu, family, shape, limits=limits)
    _assert_solo_equals_base(ev, data, family, got[family], got[family + "+advance"], got["general"],
                             f"{family} {shape} {limits}")


# ------------------------------------------------- 5 n_active, genome_rows ----
@pytest.mark.parametrize("family", list(FAMILIES))
def test_solo_n_active_and_permuted_rows(gpu, family):
    from pong_amd.device import EvalResult
    shape = SHAPES[family][0]
    ev, data, _ = runs(gpu, family, shape)
    n, active = data["genomes"].shape[0], 77
    rows = torch.tensor(np.random.default_rng(3).permutation(n).astype(np.int32), device=gpu)
    count = torch.tensor([active], dtype=torch.int32, device=gpu)

    def play(kernel):
        out = EvalResult(fitness=torch.full((n,), -7.0, dtype=torch.float64, device=gpu),
                         rewards=torch.full((n, 6), -7.0, dtype=torch.float64, device=gpu),
                         scores=torch.full((n, 6, 2), -7, dtype=torch.int32, device=gpu),
                         frames=torch.full((n, 6), -7, dtype=torch.int32, device=gpu),
                         total_frames=torch.full((n, 6), -7.0, dtype=torch.float64, device=gpu),
                         status=torch.full((n,), -7, dtype=torch.int32, device=gpu),
                         counters=torch.empty(16, dtype=torch.int64, device=gpu))
        return _play(ev, data, kernel, rows=rows, n_active=count, out=out)[0]

    got = {k: play(k) for k in (family, family + "+solo", family + "+advance", family + "+advance+solo")}
    torch.cuda.synchronize()
    for base, solo in ((family, family + "+solo"), (family + "+advance", family + "+advance+solo")):
        _equal(got[solo], got[base], solo)
        assert int(got[solo].counters[3]) == active * 6
        for name in FIELDS:  # the rows past n_active keep the sentinel
            t = getattr(got[solo], name)
            assert bool((t[active:] == -7).all()) and not bool((t[:active] == -7).any()), (solo, name)


# ------------------------------------------------------ 6 traced launches ----
@pytest.mark.parametrize("family", list(FAMILIES))
def test_traced_solo_launch(gpu, family):
    """The first 96 games are 16 genomes' [0,1,2,3,3,3]: solo and NN games.  A
    traced launch keeps solo on and, with both bits, runs without the advance."""
    shape = SHAPES[family][0]
    ev, data, got = runs(gpu, family, shape)
    out = {k: _play(ev, data, k, trace_games=96, trace_cap=2048)
           for k in (family + "+solo", family + "+advance+solo", "general")}
    torch.cuda.synchronize()
    ref, ref_tr = out["general"]
    assert int(ref_tr.any())
    for k in (family + "+solo", family + "+advance+solo"):
        res, tr = out[k]
        _equal(res, ref, k, counters=False)
        assert torch.equal(tr, ref_tr), k
        assert torch.equal(res.counters, got[family].counters), k  # the stepping kernel's: [8] = [12] = 0
        assert int(res.counters[8]) == 0 and int(res.counters[12]) == 0


# ----------------------------------------------------------------- 7 AUTO ----
@pytest.mark.parametrize("family,shape", [("relu", [6, 2, 2]), ("relu2", [6, 2, 2, 2])], ids=ids)
def test_auto_solo_in_the_relu_scopes(gpu, family, shape):
    ev, data, got = runs(gpu, family, shape)
    for mods in ("+solo", "+advance+solo"):
        auto, _ = _play(ev, data, "auto" + mods)
        named, _ = _play(ev, data, family + mods)
        torch.cuda.synchronize()
        _equal(auto, named, mods)
        _equal(auto, got[family + "+advance"] if "advance" in mods else got[family], mods)


@pytest.mark.parametrize("activation,shape", [("sigmoid", [6, 64, 3]), ("relu", [6, 4, 4, 4, 2]),
                                              ("sigmoid", [6, 16, 16, 3])], ids=ids)
def test_auto_solo_changes_nothing_elsewhere(gpu, activation, shape):
    """Where AUTO resolves to SPLIT ([6,64,3] sigmoid) or GENERAL the bit changes nothing."""
    from pong_amd.device import Evaluator
    genomes, members, kinds, opp, mult = population(shape, activation, n=48, hall=8)
    ev = Evaluator(shape, device=gpu, activation=activation)
    args = [dev_genomes(genomes, gpu)] + [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    got = {k: ev.evaluate(*args, opponents=dev_genomes(members, gpu), kernel=k)[0]
           for k in ("auto+solo", "auto+advance+solo", "auto")}
    torch.cuda.synchronize()
    _equal(got["auto+solo"], got["auto"])
    _equal(got["auto+advance+solo"], got["auto"])


# ------------------------------------------------- 8 DeviceGA, the drop-in ----
def test_device_ga_auto_solo_generations(gpu):
    """Three generations from an empty hall, so generation 0 is all scripted."""
    from pong_amd.evolve import DeviceGA
    shape = [6, 16, 3]
    out = {}
    for kernel in ("auto+solo", "auto+advance+solo", "auto"):
        ga = DeviceGA(shape, 64, device=gpu, seed=9, activation="relu", kernel=kernel)
        assert ga.ev.kernel == kernel and ga.ev.activation == "relu"
        ga.initialize("normal", 1.0)
        history = [ga.step() for _ in range(3)]
        torch.cuda.synchronize()
        out[kernel] = (ga, history, ga.hall_of_fame.clone(), ga.hof_member_fitness)
    ga_b, hist_b, hall_b, hall_fit_b = out["auto"]
    for kernel in ("auto+solo", "auto+advance+solo"):
        ga, hist, hall, hall_fit = out[kernel]
        assert hist == hist_b
        assert torch.equal(hall, hall_b) and np.array_equal(hall_fit, hall_fit_b)
        assert torch.equal(ga.fitness, ga_b.fitness) and torch.equal(ga.population_full(), ga_b.population_full())
    assert torch.equal(out["auto+solo"][0].last.counters, ga_b.last.counters)
    assert int(out["auto+advance+solo"][0].last.counters[12]) > 0


@pytest.fixture
def relu_dropin():
    """config.ACTIVATION = "relu" as a user sets it; the test sets config.KERNEL."""
    with dropin_config(activation="relu"):
        import config
        yield config


def test_dropin_evaluate_equals_auto(gpu, relu_dropin):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on a [6,16,3] ReLU network with
    config.KERNEL = "auto+solo" and "auto+advance+solo" against "auto": the same
    hall, the same random seed, the same fitness."""
    import main
    import utils
    config = relu_dropin
    shape = [6, 16, 3]
    rng = np.random.default_rng(81)
    G = _genes(shape)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame)
    try:
        utils.NETWORK_SHAPE = shape
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]

        def fitness(kernel):  # (pick_hall_of_famer shuffles the hall in place: a fresh one, in the same order, per run)
            config.KERNEL = kernel
            ev = main._evaluator()
            assert ev.activation == "relu" and list(ev.nodes) == shape and ev.kernel == kernel
            return dropin_fitness(hall, inds)

        want = fitness("auto")
        assert len(set(want)) >= 3
        assert fitness("auto+solo") == want
        assert fitness("auto+advance+solo") == want
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame = saved
