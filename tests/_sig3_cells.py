"""The game populations of k_sig3's tests (tests/test_sig3_host.py checks them on
the CPU oracle, tests/test_gpu_sig3.py plays them): per shape one population of
test_gpu_advance's noisy sigmoid trackers, built as tests/_relu3_cells.py builds
its cells -- 96 genomes, a hall of 24, the default limits.  Seed 0 meets that
file's conditions (>= 6 % of the games timed out, >= 50 % ended by score,
>= 1.5 % timed out after a point, solo games of different lengths) on the
oracle for every model shape, in f64 and in f32-rounded genes."""
import numpy as np

import _sig3_model as M
from test_gpu_advance import population
from test_gpu_modifier_instances import GENES, HALL_CELL, N_CELL

FLOORS = (0.06, 0.5, 0.015)
SEEDS = {tuple(shape): 0 for shape in M.SHAPES}
# test_gpu_modifier_instances' cells name a kernel family for its activation: every k_sig3 cell is a "sig2" one there
CELLS = [("sig2", shape, genes) for shape in SEEDS for genes in GENES]


def cell_id(cell):
    return f"sig3-{'x'.join(map(str, cell[1]))}-{cell[2]}"


def cell_population(cell, seed=None):
    """(genomes, hall, kinds, opp, mult) of a cell; an f32 cell's genes are the f32-rounded values, as f64."""
    _, shape, genes = cell
    genomes, members, kinds, opp, mult = population(list(shape), "sigmoid", n=N_CELL, hall=HALL_CELL,
                                                    seed=SEEDS[shape] if seed is None else seed)
    if genes == "f32":
        genomes = genomes.astype(np.float32).astype(np.float64)
        members = members.astype(np.float32).astype(np.float64)
    return genomes, members, kinds, opp, mult
