"""PG_KERNEL_SOLO where PG_KERNEL_AUTO resolves to SPLIT, on the MI355X (run with
-m gpu): k_service's six solo instances ([6, 33..64, O] on 8-lane groups, O in
2..4, f32 / f64 genes) -- a game against a scripted opponent on
half a lane group, a game against a hall-of-fame row on a whole one -- against
the base instances and the CPU oracle.

"Equal" means torch.equal on fitness, rewards, scores, frames, total_frames and
status and on all 16 counters.  Every case first asks pg_eval_resolve
(Evaluator.resolved_kernel) which instance it is about to run.
"""

import numpy as np
import pytest
import torch

from _gpu_support import FIELDS, assert_same, dev_genomes, dropin_fitness, gene_count, ids
from test_gpu_advance import SERVE, SHORT, population
from test_gpu_service_instances import DTYPES, _as_stored, _special_rows

pytestmark = pytest.mark.gpu

NN = 3  # PG_OPP_NN
N, HALL = 192, 24
SHAPE = [6, 64, 3]


def _equal(a, b, what=""):
    for name in FIELDS:
        assert torch.equal(getattr(a, name), getattr(b, name)), (name, what)
    assert torch.equal(a.counters, b.counters), (what, a.counters.tolist(), b.counters.tolist())


def _mixed_kinds(n):
    """Rows below n / 2 play the reference schedule, the rest six hall-of-fame rows."""
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = NN
    return kinds


def _varied(shape, bias, dtype, n=N, hall=HALL, seed=0):
    """(genomes, hall, kinds, opp, mult): N(0,1), N(0,9), U[0,1) and N(0,81) genes by
    quarters, rows 0..4 the all-zero, over-cap, NaN and infinite networks."""
    rng = np.random.default_rng([*shape, int(bias), dtype == "f32", seed, 73])
    G = gene_count(shape, bias)
    genomes = np.empty((n, G))
    for q, rows in enumerate(np.array_split(np.arange(n), 4)):
        genomes[rows] = rng.random((len(rows), G)) if q == 2 else rng.standard_normal((len(rows), G)) * (1.0, 3.0, 0, 9.0)[q]
    _special_rows(genomes, rng)
    members = rng.standard_normal((hall, G)) * 3.0
    opp = rng.integers(0, hall, size=(n, 6)).astype(np.int32)
    mult = np.round(rng.normal(size=(n, 6)), 3)
    return _as_stored(genomes, dtype), _as_stored(members, dtype), _mixed_kinds(n), opp, mult


def _on_device(gpu, host, dt=torch.float64, with_hall=True, n_games=6):
    genomes, members, kinds, opp, mult = host
    return dict(genomes=dev_genomes(genomes, gpu, dt), opponents=dev_genomes(members, gpu, dt) if with_hall else None,
                sched=[torch.tensor(np.ascontiguousarray(a[:, :n_games]), device=gpu) for a in (kinds, opp, mult)])


def _play(ev, data, kernel, **kw):
    return ev.evaluate(data["genomes"], *data["sched"], opponents=data["opponents"], kernel=kernel, **kw)


def _solo_equals_base(ev, data, what, **kw):
    """auto+solo = auto (and auto+advance+solo, whose advance bit SPLIT ignores), on the solo instance."""
    assert ev.resolved_kernel("auto+solo") == "split+solo" == ev.resolved_kernel("auto+advance+solo"), what
    assert ev.resolved_kernel("auto") == "split", what
    base, _ = _play(ev, data, "auto", **kw)
    solo, _ = _play(ev, data, "auto+solo", **kw)
    both, _ = _play(ev, data, "auto+advance+solo", **kw)
    torch.cuda.synchronize()
    _equal(solo, base, what)
    _equal(both, base, what)
    return base, solo


# ------------------------------------------------ 1 every routed instance ----
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("O", [2, 3, 4])
@pytest.mark.parametrize("H", [33, 64])
def test_every_routed_instance(gpu, oracle, H, O, dtype, bias):
    from pong_amd.device import Evaluator
    shape = [6, H, O]
    host = _varied(shape, bias, dtype)
    genomes, members, kinds, opp, mult = host
    ev = Evaluator(shape, bias=bias, dtype=DTYPES[dtype], device=gpu)
    base, solo = _solo_equals_base(ev, _on_device(gpu, host, DTYPES[dtype]), f"{shape} {dtype} bias={bias}")
    ref = oracle.eval_population(genomes, shape, kinds, opp, mult, opponents=members, bias=bias, n_threads=8)
    assert_same(solo, ref)
    c = solo.counters.cpu().numpy()
    assert c[3] == N * 6 and c[0] + c[8] + c[12] == ref["frames"].sum() and c[12] > 0
    assert c[4] > 0 and c[2] > 0  # (the all-zero network reaches the numpy-order forward on every visible frame)


# ------------------------------------- 2 the cascade under 16 requesters ----
def test_cascade_under_sixteen_requesters(gpu):
    """U[0,1) genes (an initial population's): saturated sigmoids, near-tied
    outputs, so certificates fail in solo games of both halves of a group and
    serve_inline meets up to 16 requesting half-groups of a wave."""
    from pong_amd.device import Evaluator
    rng = np.random.default_rng(11)
    G = gene_count(SHAPE, True)
    host = (rng.random((N, G)), rng.random((HALL, G)), _mixed_kinds(N), rng.integers(0, HALL, size=(N, 6)).astype(np.int32),
            np.ones((N, 6)))
    ev = Evaluator(SHAPE, device=gpu)
    data = _on_device(gpu, host)
    base, _ = _play(ev, data, "auto")
    torch.cuda.synchronize()
    c = base.counters.cpu().numpy()
    print(f"base: certificate failures [4]={c[4]}, numpy-order f64 [2]={c[2]}, certified f64 [5]={c[5]}, in-wave [6]={c[6]}")
    assert c[4] > 0 and c[2] + c[5] > 0  # (the parent's code: serve_inline is reached)
    _solo_equals_base(ev, data, "uniform genes")


# ------------------------------------------------------------ 3 schedules ----
@pytest.mark.parametrize("schedule", ["scripted", "nn", "one_solo"])
def test_schedules(gpu, schedule):
    """All scripted with no hall at all (generation 0), all NN (the solo queue is
    walked and holds nothing), and exactly one solo game among NN games."""
    from pong_amd.device import Evaluator
    n = 48
    genomes, members, _, opp, mult = population(SHAPE, "sigmoid", n, 8)
    if schedule == "scripted":
        kinds = np.tile(np.array([0, 1, 2, 0, 2, 1], np.int32), (n, 1))
    else:
        kinds = np.full((n, 6), NN, np.int32)
        if schedule == "one_solo":
            kinds[5, 2] = 1
    ev = Evaluator(SHAPE, device=gpu)
    data = _on_device(gpu, (genomes, members, kinds, opp, mult), with_hall=schedule != "scripted")
    base, solo = _solo_equals_base(ev, data, schedule)
    assert int(solo.counters[3]) == n * 6 and len(np.unique(solo.frames.cpu().numpy())) > 1


@pytest.mark.parametrize("kind", [0, 1, 2, NN])
def test_one_game_launch(gpu, kind):
    """One genome, one game: one block, one half-group (a whole group for kind 3) of it playing."""
    from pong_amd.device import Evaluator
    genomes, members, _, opp, mult = population(SHAPE, "sigmoid", 1, 8)
    ev = Evaluator(SHAPE, device=gpu, n_games=1)
    data = _on_device(gpu, (genomes, members, np.array([[kind]], np.int32), opp, mult), n_games=1)
    base, solo = _solo_equals_base(ev, data, f"one game of kind {kind}")
    assert int(solo.counters[3]) == 1 and int(solo.frames[0, 0]) > 30


# --------------------------------------------------------------- 4 reload ----
def test_groups_reload_and_pass_from_pair_to_solo_games(gpu):
    """More NN games than the launch has lane groups, so groups reload pair games
    and later pass on to solo games, each half on its own.  The grid is
    min(ceil(games / 64), 2 CUs) blocks of 64 groups of 8 lanes: 32 768 groups on
    the MI355X's 256 CUs.  n = 8 192 under the mixed schedule gives 36 864 NN
    games and 12 288 solo games on 65 536 half-groups."""
    from pong_amd.device import Evaluator
    shape, n = [6, 33, 2], 8192
    groups = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count * 64
    host = _varied(shape, True, "f64", n=n, hall=64, seed=1)
    assert (host[2] == NN).sum() > 1.1 * groups and (host[2] != NN).sum() > 0
    ev = Evaluator(shape, device=gpu)
    base, solo = _solo_equals_base(ev, _on_device(gpu, host), f"{shape} n={n}")
    assert int(solo.counters[3]) == n * 6


# ------------------------------------------- 5 limits, n_active, genome_rows ----
@pytest.mark.parametrize("limits", [SHORT, SERVE], ids=ids)
def test_under_other_limits(gpu, limits):
    from pong_amd.device import Evaluator
    host = population(SHAPE, "sigmoid")
    ev = Evaluator(SHAPE, device=gpu, timeout_thresh=limits[0], win_score=limits[1])
    base, solo = _solo_equals_base(ev, _on_device(gpu, host), f"limits {limits}")
    if limits == SERVE:
        assert (solo.frames.cpu().numpy() == 34).all()


def test_n_active_and_permuted_rows(gpu):
    from pong_amd.device import EvalResult, Evaluator
    host = population(SHAPE, "sigmoid")
    ev = Evaluator(SHAPE, device=gpu)
    data = _on_device(gpu, host)
    active = 77
    rows = torch.tensor(np.random.default_rng(3).permutation(N).astype(np.int32), device=gpu)
    count = torch.tensor([active], dtype=torch.int32, device=gpu)
    assert ev.resolved_kernel("auto+solo") == "split+solo"

    def play(kernel):
        out = EvalResult(fitness=torch.full((N,), -7.0, dtype=torch.float64, device=gpu),
                         rewards=torch.full((N, 6), -7.0, dtype=torch.float64, device=gpu),
                         scores=torch.full((N, 6, 2), -7, dtype=torch.int32, device=gpu),
                         frames=torch.full((N, 6), -7, dtype=torch.int32, device=gpu),
                         total_frames=torch.full((N, 6), -7.0, dtype=torch.float64, device=gpu),
                         status=torch.full((N,), -7, dtype=torch.int32, device=gpu),
                         counters=torch.empty(16, dtype=torch.int64, device=gpu))
        return _play(ev, data, kernel, rows=rows, n_active=count, out=out)[0]

    base, solo = play("auto"), play("auto+solo")
    torch.cuda.synchronize()
    _equal(solo, base)
    assert int(solo.counters[3]) == active * 6
    for name in FIELDS:  # the rows past n_active keep the sentinel
        t = getattr(solo, name)
        assert bool((t[active:] == -7).all()) and not bool((t[:active] == -7).any()), name


# ----------------------------------------------------------------- 6 prep ----
def test_records_prepared_in_two_calls(gpu):
    """PG_PREP_GENOMES then PG_PREP_REST against one PG_PREP_ALL call: the lane records are the base's."""
    from pong_amd.device import Evaluator
    host = population(SHAPE, "sigmoid")
    ev = Evaluator(SHAPE, device=gpu)
    data = _on_device(gpu, host)
    base, solo = _solo_equals_base(ev, data, "prep all")
    _play(ev, data, "auto+solo", prep="genomes")
    two, _ = _play(ev, data, "auto+solo", prep="rest")
    torch.cuda.synchronize()
    _equal(two, base, "prep genomes + rest")


# ------------------------------------------------------------ 7 fallbacks ----
def test_traced_horizon_and_logged_launches_run_the_base_instance(gpu):
    from pong_amd.device import Evaluator
    host = population(SHAPE, "sigmoid")
    ev = Evaluator(SHAPE, device=gpu)
    data = _on_device(gpu, host)
    assert ev.resolved_kernel("auto+solo", traced=True) == "split" == ev.resolved_kernel("auto+advance+solo", traced=True)
    assert ev.resolved_kernel("auto+solo", horizon=37) == "split" == ev.resolved_kernel("auto+solo", hard_log=True)
    out = {k: _play(ev, data, k, trace_games=96, trace_cap=2048) for k in ("auto", "auto+solo")}
    torch.cuda.synchronize()
    _equal(out["auto+solo"][0], out["auto"][0], "traced")
    assert int(out["auto"][1].any()) and torch.equal(out["auto+solo"][1], out["auto"][1])
    hz = {k: _play(ev, data, k, horizon=37)[0] for k in ("auto", "auto+solo")}
    torch.cuda.synchronize()
    _equal(hz["auto+solo"], hz["auto"], "horizon")
    # the hard-case log: row 0 as the all-zero network, whose every visible frame is decided in numpy's order and
    # logged; the records are appended in the waves' order, so they are compared as sorted rows
    zeroed = (np.concatenate([np.zeros_like(host[0][:1]), host[0][1:]]),) + tuple(host[1:])
    data = _on_device(gpu, zeroed)
    cap = 1 << 16
    logs = {k: torch.zeros((cap, 8), dtype=torch.int32, device=gpu) for k in ("auto", "auto+solo")}
    logged = {k: _play(ev, data, k, hard_log=logs[k])[0] for k in logs}
    torch.cuda.synchronize()
    _equal(logged["auto+solo"], logged["auto"], "hard_log")
    n_logged = int(logged["auto"].counters[9])
    assert 0 < n_logged <= cap
    rows = {k: np.unique(logs[k][:n_logged].cpu().numpy(), axis=0, return_counts=True) for k in logs}
    assert np.array_equal(rows["auto"][0], rows["auto+solo"][0]) and np.array_equal(rows["auto"][1], rows["auto+solo"][1])


# ------------------------------------------------- 8 DeviceGA, the drop-in ----
def test_device_ga_auto_solo_generations(gpu):
    """Three generations from an empty hall, so generation 0 is all scripted."""
    from pong_amd.evolve import DeviceGA
    out = {}
    for kernel in ("auto+solo", "auto"):
        ga = DeviceGA(SHAPE, 64, device=gpu, seed=9, kernel=kernel)
        assert ga.ev.kernel == kernel and ga.ev.resolved_kernel() == ("split+solo" if "solo" in kernel else "split")
        ga.initialize("normal", 1.0)
        history = [ga.step() for _ in range(3)]
        torch.cuda.synchronize()
        out[kernel] = (ga, history, ga.hall_of_fame.clone(), ga.hof_member_fitness)
    (ga, hist, hall, hall_fit), (ga_b, hist_b, hall_b, hall_fit_b) = out["auto+solo"], out["auto"]
    assert hist == hist_b
    assert torch.equal(hall, hall_b) and np.array_equal(hall_fit, hall_fit_b)
    assert torch.equal(ga.fitness, ga_b.fitness) and torch.equal(ga.population_full(), ga_b.population_full())
    assert torch.equal(ga.last.counters, ga_b.last.counters)


def test_dropin_evaluate_equals_auto(gpu):
    """ga.toolbox.map(ga.toolbox.evaluate, ...) on the [6,64,3] sigmoid network with
    config.KERNEL = "auto+solo" against "auto": the same hall, the same random seed, the same fitness."""
    import config
    import main
    import utils
    rng = np.random.default_rng(81)
    G = gene_count(SHAPE, True)
    saved = (utils.NETWORK_SHAPE, main.hall_of_fame, config.KERNEL)
    try:
        utils.NETWORK_SHAPE = SHAPE
        hall = rng.standard_normal((4, G))
        inds = [list(g) for g in rng.standard_normal((24, G))]

        def fitness(kernel):  # (pick_hall_of_famer shuffles the hall in place: a fresh one, in the same order, per run)
            config.KERNEL = kernel
            ev = main._evaluator()
            assert list(ev.nodes) == SHAPE and ev.kernel == kernel
            assert ev.resolved_kernel() == ("split+solo" if "solo" in kernel else "split")
            return dropin_fitness(hall, inds)

        want = fitness("auto")
        assert len(set(want)) >= 3
        assert fitness("auto+solo") == want
    finally:
        utils.NETWORK_SHAPE, main.hall_of_fame, config.KERNEL = saved
