"""The CPU oracle with activation="relu" against the reference's own outputs
(CPU only), so that it can stand as the checker of the ReLU kernels' whole games:
  * NeuralNetwork.run with ReLU (tests/golden/relu_forward.npz and
    relu_forward_wide.npz, written by the real reference code): the argmax, and
    the output activations bit for bit up to the sign of zero -- no
    transcendental is involved, every pre-activation is np.dot's (or_blas_dot);
  * evaluate() with ReLU (relu_evaluate.json): the host schedule plus the oracle
    reproduce the reference fitness bit for bit;
  * whole games against the reference's per-frame numpy loop (oracle/numpy_loop.py
    with its activation replaced by np.maximum(0.0, .)): one, two and 64 + 33
    hidden units, at TIMEOUT_THRESH 119 / WIN_SCORE 1 and at the default 2000 / 3,
    a 2 000-frame timeout included;
  * NaN and inf genes against a plain numpy restatement (np.maximum keeps a NaN,
    np.argmax returns the first);
  * the seed table of tests/test_gpu_modifier_instances.py: every population
    meets its conditions on the oracle's result.
The sigmoid default is pinned, unchanged, by tests/test_oracle_golden.py.
"""
import hashlib
import random
import warnings

import numpy as np
import pytest

from _gpu_support import HoF, Member
from test_gpu_advance import population
from test_gpu_modifier_instances import (CELLS, _cell_id, all_cells, cell_population, check_cell_population,
                                         oracle_result)
from test_gpu_relu import _numpy_games


def _bits(a):
    """f64 bit patterns with -0 mapped to +0."""
    return (np.asarray(a, dtype=np.float64) + 0.0).view(np.int64)


def _gene_count(shape):
    return sum((shape[i] + 1) * shape[i + 1] for i in range(len(shape) - 1))


# ------------------------------------------------------------- 1 forward ----
@pytest.mark.parametrize("key", ["6x2x2", "6x16x2", "6x64x2", "6x64x64x2"])
def test_nn_forward_matches_reference(oracle, golden, key):
    g = golden("relu_forward.npz")
    shape = [int(v) for v in g[f"{key}__shape"]]
    genes, gidx, x = g[f"{key}__genes"], g[f"{key}__gidx"], g[f"{key}__x"]
    zero_ties = 0
    for s in range(len(x)):
        idx, act = oracle.nn_run(genes[gidx[s]], shape, x[s], activation="relu")
        assert idx == g[f"{key}__idx"][s]
        np.testing.assert_array_equal(_bits(act), _bits(g[f"{key}__act"][s]))
        zero_ties += bool((act <= 0).all())
    assert zero_ties > 0  # the all-zero tie (index 0) is among the fixture's passes


@pytest.mark.parametrize("key", ["6x100x130x2", "6x512x512x2"])
def test_nn_forward_wide_matches_reference(oracle, golden, key):
    """What tests/test_gpu_relu_wide.py reads: genes stored, or regenerated from
    their seeds and checked by their hash; inputs on the game's k / 320 grid."""
    g = golden("relu_forward_wide.npz")
    shape = [int(v) for v in g[f"{key}__shape"]]
    if f"{key}__genes" in g:
        genes = g[f"{key}__genes"]
    else:
        rows = []
        for seed, dist, sha in zip(g[f"{key}__seed"], g[f"{key}__dist"], g[f"{key}__genes_sha256"]):
            rng = np.random.default_rng(int(seed))
            row = rng.random(_gene_count(shape)) if str(dist) == "init" else rng.standard_normal(_gene_count(shape))
            row = row.astype(np.float32).astype(np.float64)
            assert hashlib.sha256(row.tobytes()).hexdigest() == str(sha)
            rows.append(row)
        genes = np.array(rows)
    k, gidx = g[f"{key}__k"], g[f"{key}__gidx"]
    for s in range(len(k)):
        idx, act = oracle.nn_run(genes[gidx[s]], shape, (k[s] / 2) / 160, activation="relu")
        assert idx == g[f"{key}__idx"][s]
        np.testing.assert_array_equal(_bits(act), _bits(g[f"{key}__act"][s]))


# ------------------------------------------------------------ 2 evaluate ----
def test_evaluate_matches_reference(oracle, golden):
    import utils
    from pong_amd import schedule
    for case in golden("relu_evaluate.json"):
        assert case["activation"] == "relu"
        hof = HoF([Member(g, f) for g, f in zip(case["hof_genes"], case["hof_fitness"])])
        random.seed(case["random_seed"])
        n = len(case["individuals"])
        kind, opp, mult, chosen = schedule.reference_schedule(n, 6, hof, utils.pick_hall_of_famer)
        opponents = np.array([list(m) for m in chosen]) if chosen else None
        r = oracle.eval_population(np.array(case["individuals"]), case["shape"], kind, opp, mult, opponents=opponents,
                                   activation="relu")
        np.testing.assert_array_equal(r["fitness"], np.array(case["fitness"]))
        games = case["games"]
        if games:
            np.testing.assert_array_equal(r["rewards"].ravel(), [g["reward"] for g in games])
            np.testing.assert_array_equal(r["frames"].ravel(), [g["frames"] for g in games])
        # the activation matters: the sigmoid oracle plays these individuals otherwise
        s = oracle.eval_population(np.array(case["individuals"]), case["shape"], kind, opp, mult, opponents=opponents)
        assert (s["fitness"] != r["fitness"]).any()


# ------------------------------------------- 3 whole games, the numpy loop ----
@pytest.fixture
def relu_loop(monkeypatch):
    """oracle/numpy_loop.py with ReLU as its activation; counts[1] of its counts[0]
    decisions had every output <= 0."""
    import numpy_loop as NL
    monkeypatch.setattr(NL, "_sigmoid", lambda x: np.maximum(0.0, x))
    counts = [0, 0]
    run0 = NL.NumpyNet.run

    def run(self, x):
        r = run0(self, x)
        counts[0] += 1
        counts[1] += bool(self.acts[-1][:-1].max() <= 0)
        return r

    monkeypatch.setattr(NL.NumpyNet, "run", run)
    return NL, counts


def _schedule(rng, n, hall):
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    opp = rng.integers(0, hall, size=(n, 6)).astype(np.int32)
    mult = np.ones((n, 6))
    mult[:, 3:] = np.round(rng.normal(size=(n, 3)), 3)
    mult[0, 3] = -0.625
    return kinds, opp, mult


def _assert_oracle_equals_loop(oracle, relu_loop, shape, genomes, opponents, sched, thresh, win):
    NL, counts = relu_loop
    kinds, opp, mult = sched
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # find_stuff's mean of an absent colour
        ref = _numpy_games(NL, shape, genomes, opponents, kinds, opp, mult, thresh, win)
    got = oracle.eval_population(genomes, shape, kinds, opp, mult, opponents=opponents, timeout_thresh=thresh,
                                 win_score=win, activation="relu")
    for name in ("scores", "frames", "total_frames", "rewards", "fitness"):
        np.testing.assert_array_equal(got[name], ref[name], err_msg=name)
    assert not got["status"].any()
    assert counts[1] > 0, counts
    print(f"{shape} at {thresh} / {win}: {int(ref['frames'].sum())} frames, {counts[1]} of {counts[0]} decisions had "
          f"every output <= 0")
    return got


@pytest.mark.parametrize("shape", [[6, 64, 3], [6, 33, 64, 4], [6, 1, 2]])
def test_short_games_equal_the_numpy_loop(oracle, relu_loop, shape):
    """Two genomes x 6 games at TIMEOUT_THRESH 119 / WIN_SCORE 1 against a hall of 3."""
    rng = np.random.default_rng(sum(shape))
    G = _gene_count(shape)
    genomes, opponents = rng.standard_normal((2, G)), rng.standard_normal((3, G))
    _assert_oracle_equals_loop(oracle, relu_loop, shape, genomes, opponents, _schedule(rng, 2, 3), 119, 1)


def test_default_limit_games_equal_the_numpy_loop(oracle, relu_loop):
    """One [6,64,3] genome x 6 games at the default 2000 / 3.  Random N(0, 1) ReLU
    networks mostly decide one index for ever and lose 0 : 3 in 180 frames, so the
    genome and the hall of 3 are test_gpu_advance's noisy trackers; seed 26 was
    chosen with the oracle among seeds 0..59 as the one whose six games (8 264
    frames) show the most: a timeout at 0 : 0, a timeout after a point, a timeout
    at 2 : 2 and games ended by score.  That is asserted."""
    shape = [6, 64, 3]
    genomes, members, _, opp, mult = population(shape, "relu", n=1, hall=3, seed=26)
    kinds = np.array([[0, 1, 2, 3, 3, 3]], np.int32)
    mult = np.where(kinds == 3, mult, 1.0)  # evaluate() scores its scripted games with multiplier 1 (main.py:39-53)
    got = _assert_oracle_equals_loop(oracle, relu_loop, shape, genomes, members, (kinds, opp, mult), 0, 0)
    scores = got["scores"].reshape(-1, 2)
    timed_out = (scores < 3).all(axis=1)
    assert (got["frames"].ravel()[timed_out] > 2000).all() and (~timed_out).any()
    assert (timed_out & (scores.sum(axis=1) == 0)).any() and (timed_out & (scores.sum(axis=1) > 0)).any()


# ------------------------------------------------------ 4 non-finite genes ----
def _numpy_run(genes, shape, x):
    """NeuralNetwork.run with ReLU, restated plainly (numpy_nn.py:120-137)."""
    a = np.append(np.asarray(x, dtype=np.float64), 1.0)
    off = 0
    for i in range(len(shape) - 1):
        n = (shape[i] + 1) * shape[i + 1]
        w = np.asarray(genes[off:off + n]).reshape(shape[i + 1], shape[i] + 1)
        off += n
        a = np.append(np.maximum(0.0, np.dot(w, a)), 1.0)
    return int(np.argmax(a[:-1])), a[:-1]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("shape", [[6, 16, 3], [6, 8, 8, 4]])
def test_non_finite_genes_equal_numpy(oracle, shape, bad):
    """A NaN pre-activation stays NaN through np.maximum and np.argmax returns the
    first NaN; +inf stays, -inf becomes 0; inf - inf and 0 * inf turn up as NaN
    further on.  One non-finite gene in turn in each layer's weights and biases."""
    rng = np.random.default_rng(len(shape))
    G = _gene_count(shape)
    first_layer = (shape[0] + 1) * shape[1]
    spots = [0, shape[0], first_layer - 1, first_layer, G - shape[-2] - 1, G - 1]
    xs = rng.integers(0, 321, size=(16, 6)) / 320.0
    xs[0] = 0.0  # 0 * inf
    nan_outputs = 0
    for spot in spots:
        genes = rng.standard_normal(G)
        genes[spot] = bad
        for x in xs:
            with np.errstate(invalid="ignore"):
                want_idx, want_act = _numpy_run(genes, shape, x)
            idx, act = oracle.nn_run(genes, shape, x, activation="relu")
            assert idx == want_idx, (spot, x, act, want_act)
            np.testing.assert_array_equal(np.isnan(act), np.isnan(want_act))
            fin = ~np.isnan(act)
            np.testing.assert_array_equal(_bits(act[fin]), _bits(want_act[fin]))
            nan_outputs += bool(np.isnan(act).any())
    if np.isnan(bad):
        assert nan_outputs > 0


def test_unknown_activation_is_refused(oracle):
    with pytest.raises(ValueError):
        oracle.nn_run(np.zeros(20), [6, 2, 2], np.zeros(6), activation="tanh")


# ------------------------ 5 the seed table of test_gpu_modifier_instances ----
def test_the_table_lists_every_cell():
    assert len(all_cells()) == 54 and set(CELLS) == set(all_cells())


@pytest.mark.parametrize("cell", all_cells(), ids=_cell_id)
def test_cell_population_meets_its_conditions(oracle, cell):
    """>= 5 % of the games timed out, >= 50 % ended by score, >= 1 % timed out after
    a point; the solo games differ in length; a ReLU cell shows the all-zero tie."""
    pop = cell_population(cell)
    shares = check_cell_population(oracle, cell, pop, oracle_result(oracle, cell, pop))
    print(f"{_cell_id(cell)}: seed {CELLS[cell]}, timed out {shares[0]:.3f}, by score {shares[1]:.3f}, "
          f"timed out after a point {shares[2]:.3f}")
