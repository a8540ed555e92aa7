"""Every "+advance" and "+solo" instance on the MI355X (run with -m gpu): the 54
cells family {relu, relu2, sig2} x lane layout x O {2, 3, 4} x genes {f64, f32},
each at the WIDEST shape of its layout, where register pressure is highest
(tests/test_gpu_advance.py and tests/test_gpu_solo.py keep the smallest shapes).

Per cell one population of test_gpu_advance's noisy trackers (96 genomes, a
hall of 24, rows below 48 playing kinds [0,1,2,3,3,3] and the rest all-NN) at
the default limits 2000 / 3 is played by X, X+advance, X+solo, X+advance+solo
and general, and by the CPU oracle (oracle.eval_population; for the ReLU
families with activation="relu").  Every comparison is exact equality.

The population must exercise what is tested, so on the ORACLE's result: >= 5 %
of the games timed out, >= 50 % ended by score, >= 1 % timed out after a point
(test_gpu_advance._check_population's conditions), the solo games' lengths are
not all equal, and in a ReLU cell some decision had every output <= 0 (the
all-zero tie, index 0).  CELLS holds one seed per cell, chosen on the CPU with
the oracle among seeds 0..25: the first that meets the stricter 6 % / 50 % /
1.5 %.  tests/test_oracle_relu.py recomputes the conditions for every row of the
table without a GPU.
"""
import numpy as np
import pytest
import torch

from _gpu_support import FIELDS, dev_genomes
from test_gpu_advance import DEFAULT, FAMILIES, _assert_advance_equals_stepping, outcome_shares, population
from test_gpu_solo import NN, _equal

N_CELL, HALL_CELL = 96, 24
# the widest shape of each lane layout, by the number of outputs O
WIDEST = {"relu": lambda O: [[6, 64, O], [6, 128, O], [6, 256, O]],
          "relu2": lambda O: [[6, 16, 16, O], [6, 32, 32, O], [6, 64, 64, O]],
          "sig2": lambda O: [[6, 16, 16, O], [6, 32, 32, O], [6, 64, 64, O]]}
GENES = ("f64", "f32")

# (family, shape) -> the population's seed; the f32-rounded genes meet the conditions under the f64 cell's seed
# (with the same three shares) in every cell, so both gene types of a shape share a row
SEEDS = {
    ("relu", (6, 64, 2)): 0, ("relu", (6, 128, 2)): 0, ("relu", (6, 256, 2)): 1,
    ("relu", (6, 64, 3)): 0, ("relu", (6, 128, 3)): 11, ("relu", (6, 256, 3)): 12,
    ("relu", (6, 64, 4)): 1, ("relu", (6, 128, 4)): 25, ("relu", (6, 256, 4)): 4,
    ("relu2", (6, 16, 16, 2)): 0, ("relu2", (6, 32, 32, 2)): 0, ("relu2", (6, 64, 64, 2)): 1,
    ("relu2", (6, 16, 16, 3)): 3, ("relu2", (6, 32, 32, 3)): 3, ("relu2", (6, 64, 64, 3)): 11,
    ("relu2", (6, 16, 16, 4)): 0, ("relu2", (6, 32, 32, 4)): 0, ("relu2", (6, 64, 64, 4)): 15,
    ("sig2", (6, 16, 16, 2)): 0, ("sig2", (6, 32, 32, 2)): 0, ("sig2", (6, 64, 64, 2)): 0,
    ("sig2", (6, 16, 16, 3)): 0, ("sig2", (6, 32, 32, 3)): 0, ("sig2", (6, 64, 64, 3)): 0,
    ("sig2", (6, 16, 16, 4)): 0, ("sig2", (6, 32, 32, 4)): 0, ("sig2", (6, 64, 64, 4)): 0,
}
# (family, shape, genes) -> the population's seed: the 54 cells
CELLS = {(family, shape, genes): seed for (family, shape), seed in SEEDS.items() for genes in GENES}


def _cell_id(cell):
    family, shape, genes = cell
    return f"{family}-{'x'.join(map(str, shape))}-{genes}"


def all_cells():
    """The 54 cells in a fixed order: family, layout, O, gene type."""
    return [(family, tuple(shape), genes) for family in FAMILIES for O in (2, 3, 4) for shape in WIDEST[family](O)
            for genes in GENES]


def cell_population(cell):
    """test_gpu_advance.population of a cell under its seed; an f32 cell's genes are
    the f32-rounded values, as f64, on both sides."""
    family, shape, genes = cell
    genomes, members, kinds, opp, mult = population(list(shape), FAMILIES[family], n=N_CELL, hall=HALL_CELL,
                                                    seed=CELLS[cell])
    if genes == "f32":
        genomes = genomes.astype(np.float32).astype(np.float64)
        members = members.astype(np.float32).astype(np.float64)
    return genomes, members, kinds, opp, mult


def oracle_result(oracle, cell, pop, base_seed=0):
    family, shape, _ = cell
    genomes, members, kinds, opp, mult = pop
    return oracle.eval_population(genomes, list(shape), kinds, opp, mult, opponents=members, base_seed=base_seed,
                                  n_threads=8, activation=FAMILIES[family])


def _c2(py):
    """Doubled centroid row of a paddle clipped to the playfield (pong_oracle.c paddle_c2)."""
    return max(py, 0) + min(py + 15, 159)


def first_zero_tie(oracle, shape, genes, kind, opp_genes, game_index, base_seed=0):
    """The first frame of one oracle game at which the right paddle's ReLU network
    had every output <= 0, or None.  The game is replayed on the oracle's physics
    from its traced actions; the inputs are or_play_slot's (inference, utils.py:139-153)."""
    seed = oracle.game_seed(base_seed, game_index)
    r = oracle.play_game(genes, shape, kind, opp_genes, 1.0, seed, trace_cap=1 << 15, activation="relu")
    env = oracle.Env(seed, one_player=kind == oracle.OPP_ROM_CPU)
    act_r = act_l = 0
    last = None
    for t in range(min(r["frames"], 1 << 15)):
        env.step4(act_r == 1, act_r == 2, act_l == 1, act_l == 2)
        s = env.state
        code = int(r["trace"][t])
        assert (code >> 4) & 1 == s.ball_visible
        if s.ball_visible:
            by2, bx2 = 2 * s.ball_y + 3, 2 * s.ball_x + 1
            pby2, pbx2 = last if last is not None else (by2, bx2)
            x = [(0.5 * bx2) / 160.0, (0.5 * by2) / 160.0, (0.5 * pbx2) / 160.0, (0.5 * pby2) / 160.0,
                 (0.5 * _c2(s.rpy)) / 160.0, (0.5 * _c2(s.lpy)) / 160.0]
            _, act = oracle.nn_run(genes, shape, x, activation="relu")
            if (act <= 0).all():
                return t
            last = (by2, bx2)
        else:
            last = None
        act_r, act_l = code & 3, (code >> 2) & 3
    return None


def check_cell_population(oracle, cell, pop, ref, floors=(0.05, 0.5, 0.01)):
    """The conditions a cell's population meets on the oracle's result; returns the three shares."""
    family, shape, _ = cell
    genomes, members, kinds, opp, mult = pop
    shares = outcome_shares(ref["scores"], DEFAULT)
    assert all(s >= f for s, f in zip(shares, floors)), (cell, shares)
    assert (kinds != NN).any() and (kinds == NN).any() and len(np.unique(ref["frames"][kinds != NN])) > 1, cell
    if FAMILIES[family] == "relu":
        tie = None
        for i in range(len(genomes)):  # the genomes' games, in order, until one shows the tie
            for g in range(6):
                k = int(kinds[i, g])
                tie = first_zero_tie(oracle, list(shape), genomes[i], k, members[opp[i, g]] if k == NN else None, g)
                if tie is not None:
                    break
            if tie is not None:
                break
        assert tie is not None, (cell, "no decision with every output <= 0")
    return shares


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cell", all_cells(), ids=_cell_id)
def test_modifier_instances_equal_the_oracle(gpu, oracle, cell):
    from pong_amd.device import Evaluator
    family, shape, genes = cell
    shape = list(shape)
    dtype = torch.float32 if genes == "f32" else torch.float64
    pop = cell_population(cell)
    genomes, members, kinds, opp, mult = pop
    ev = Evaluator(shape, device=gpu, dtype=dtype, activation=FAMILIES[family])
    kernels = (family, family + "+advance", family + "+solo", family + "+advance+solo", "general")
    for k in kernels:  # the instance asked for is the one that runs: no fallback to the base kernel
        assert ev.resolved_kernel(k) == k, (k, ev.resolved_kernel(k))
    args = [dev_genomes(genomes, gpu, dtype)] + [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    hall = dev_genomes(members, gpu, dtype)
    got = {k: ev.evaluate(*args, opponents=hall, kernel=k)[0] for k in kernels}
    torch.cuda.synchronize()
    ref = oracle_result(oracle, cell, pop, base_seed=ev.seed)
    shares = check_cell_population(oracle, cell, pop, ref)
    what = _cell_id(cell)
    print(f"{what}: seed {CELLS[cell]}, timed out {shares[0]:.3f}, by score {shares[1]:.3f}, "
          f"timed out after a point {shares[2]:.3f}")
    for k in kernels:
        for name in FIELDS:
            np.testing.assert_array_equal(getattr(got[k], name).cpu().numpy(), ref[name], err_msg=f"{what} {k} {name}")
    _assert_advance_equals_stepping(family, got[family + "+advance"], got[family], got["general"], DEFAULT, what)
    _equal(got[family + "+solo"], got[family], what + " +solo")
    _equal(got[family + "+advance+solo"], got[family + "+advance"], what + " +advance+solo")
