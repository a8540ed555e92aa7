"""Every instance of k_relu and k_relu_decide (csrc/pg_relu.hip: LN in {4, 8,
16} lanes per network x O in {2, 3, 4} x f32 / f64 genes) on the MI355X (run
with -m gpu), pinned to the host model of tests/_relu_model.py:

  (a) pg_relu_decide at every lane-count edge: z32 bit for bit the model's f32
      chain (exact fma), the bound the gcc-compiled pg_relu_bound_genome, the
      index numpy's;
  (b) the f64 fallback on networks whose exactly equal outputs are told apart
      by np.dot's summation order alone;
  (c) NaN, inf, the PG_RELU_CAP edge, f32-subnormal and all-zero genes;
  (d) whole games of every k_relu instance against the general kernel, with
      half-groups that always need the f64 forward beside ones that never do.
"""
import numpy as np
import pytest
import torch

from _relu_model import (RELU_CAP, TIE_CELLS, U32, _argmax64, _bounds, _genes, _relu_lanes, _s_max, _z32, _z64,
                         cap_net, systematic_net, tie_case, tie_net, tie_sensitivity, tiny_net)
from _gpu_support import dev_genomes, gene_count, same

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def bound_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("relu_bound")


def _relu_ev(shape, gpu, **kw):
    from pong_amd.device import Evaluator
    return Evaluator(shape, device=gpu, activation="relu", **kw)


def _as_stored(genomes, dtype):
    """The genes as the kernel reads them: f32 populations hold the rounded values."""
    g = np.asarray(genomes, np.float64)
    if dtype == "f32":
        with np.errstate(all="ignore"):
            g = g.astype(np.float32).astype(np.float64)
    return g


def _decide(ev, gpu, genomes, k, gidx, dtype):
    """pg_relu_decide and pg_forward(f64) on the same passes, as numpy arrays."""
    gt = dev_genomes(genomes, gpu, DTYPES[dtype])
    kt = torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage, z32, bound = ev.relu_decide(gt, kt, genome_index=it)
    ref_idx, act = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, stage, z32, bound, ref_idx, act))


def _host(H, O, genomes, k, gidx):
    """The model's z32, numpy's z64 and decision of every pass."""
    z32 = np.empty((len(k), O), np.float32)
    z64 = np.empty((len(k), O))
    for i in np.unique(gidx):
        m = gidx == i
        z32[m], z64[m] = _z32(H, O, genomes[i], k[m]), _z64(H, O, genomes[i], k[m])
    return z32, z64, _argmax64(z64)


def _bits(z):
    return np.ascontiguousarray(z, np.float32).view(np.int32)


# --------------------------------------------- (a) pg_relu_decide, all 18 ----
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("O", [2, 3, 4])
@pytest.mark.parametrize("H", [1, 2, 37, 63, 64, 65, 100, 127, 128, 129, 255, 256])
def test_decide_is_the_host_model(gpu, bound_dir, H, O, dtype):
    """6 networks (3 N(0,1), 2 U[0,1), systematic_net) x 37 passes = 222 passes,
    no multiple of the 16, 32 or 64 half-groups of a block, and one call with a
    single pass.  z32 is the model's chain bit for bit (the build has
    -ffp-contract=off and every butterfly step of group_sum commutes), the
    bound is pg_relu_bound_genome's up to the one f32 ulp its two f64
    summation orders can differ by, the index is numpy's."""
    rng = np.random.default_rng([H, O, dtype == "f32", 41])
    G = _genes(H, O)
    assert G == gene_count([6, H, O])
    nets = np.concatenate([rng.standard_normal((3, G)), rng.random((2, G)), systematic_net(H, O)[None]])
    nets = _as_stored(nets, dtype)
    per = 37
    k = rng.integers(0, 321, size=(6 * per, 6))
    k[5 * per], k[5 * per + 1] = 320, 0
    gidx = np.repeat(np.arange(6), per)
    ev = _relu_ev([6, H, O], gpu, dtype=DTYPES[dtype])
    index, stage, z32, bound, ref_idx, act = _decide(ev, gpu, nets, k, gidx, dtype)
    m32, z64, want = _host(H, O, nets, k, gidx)
    hb = _bounds(bound_dir, [(H, O, g) for g in nets]).astype(np.float32)[gidx]
    s = np.array([_s_max(H, O, g) for g in nets])[gidx]
    err = np.abs(z32.astype(np.float64) - z64).max(axis=1)
    print(f"[6,{H},{O}] {dtype}: largest |z32 - z64| / (u max S_o) on the device {np.max(err / (U32 * s)):.3f}, "
          f"systematic_net {np.max((err / (U32 * s))[gidx == 5]):.3f}; stage-0 share {np.mean(stage == 0):.3f}")
    np.testing.assert_array_equal(index, want)
    np.testing.assert_array_equal(index, ref_idx)
    np.testing.assert_array_equal(act + 0.0, np.maximum(0.0, z64) + 0.0)
    np.testing.assert_array_equal(_bits(z32), _bits(m32))
    assert np.isfinite(hb).all() and (np.abs(_bits(bound).astype(np.int64) - _bits(hb)) <= 1).all()
    assert (err <= bound).all()
    assert set(np.unique(stage)) <= {0, 1}
    top = -np.sort(-z64, axis=1)
    margin = np.where(top[:, 0] <= 0, -top[:, 0], top[:, 0] - np.maximum(top[:, 1], 0.0))
    large = margin > 1e-3 * s
    assert large.any() and (stage[large] == 0).all()
    # n = 1: a single half-group of a single block
    t = 5 * per
    i1, s1, z1, b1, r1, _ = _decide(ev, gpu, nets, k[t:t + 1], gidx[t:t + 1], dtype)
    assert (i1[0], s1[0], r1[0]) == (index[t], stage[t], want[t])
    assert (_bits(z1) == _bits(m32[t:t + 1])).all() and _bits(b1)[0] == _bits(bound)[t]


# --------------------------------------------- (b) the f64 fallback's order ----
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("H,O", TIE_CELLS)
def test_f64_fallback_follows_numpys_summation_order(gpu, H, O, dtype):
    """The tie network of the cell (every gene an f32 value): the exact outputs
    are equal, so the certificate never decides and np.argmax turns on the last
    bit of np.dot's sums, which depends on the row index, on O and on H + 1."""
    g, k = tie_case(H, O)
    differ, nonzero = tie_sensitivity(H, O, g, k)
    assert differ >= 8 and nonzero >= 1, (differ, nonzero)  # else this test would check nothing
    gidx = np.zeros(len(k), np.int64)
    ev = _relu_ev([6, H, O], gpu, dtype=DTYPES[dtype])
    index, stage, z32, bound, ref_idx, act = _decide(ev, gpu, g[None], k, gidx, dtype)
    z64 = _z64(H, O, g, k)
    assert (stage == 1).all() and np.isfinite(bound).all()
    np.testing.assert_array_equal(index, _argmax64(z64))
    np.testing.assert_array_equal(index, ref_idx)
    np.testing.assert_array_equal(act, np.maximum(0.0, z64))


# ------------------------------------------ (c) non-finite and extreme genes ----
def _gate_unit(g, H, j):
    """Hidden unit j: active (x0 - 0.5 > 0) on some inputs, zero on the others."""
    g[j * 7: j * 7 + 7] = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.5]


def _extreme_nets(H, O, dtype):
    """name -> genes of one network per special value ([6,16,3] and [6,100,2]
    have padding units, which load row 0 of W1)."""
    rng = np.random.default_rng([H, O, 43])
    G = _genes(H, O)
    w2 = H * 7
    nets = {}
    g = rng.standard_normal(G)
    g[(H // 2) * 7 + 2] = np.nan
    nets["nan_w1"] = g
    g = rng.standard_normal(G)
    g[w2 + (H + 1) + H // 3] = np.nan
    nets["nan_w2_row1"] = g
    g = rng.standard_normal(G)
    g[G - 1] = np.nan
    nets["nan_last_bias"] = g
    for name, v in (("pinf_w2", np.inf), ("ninf_w2", -np.inf)):
        g = rng.standard_normal(G)
        j = H - 1
        _gate_unit(g, H, j)
        g[w2 + (O - 1) * (H + 1) + j] = v
        nets[name] = g
    g = rng.standard_normal(G)
    g[1] = np.inf  # row 0 of W1: the row the padding units load
    nets["inf_w1_row0"] = g
    nets["cap_below"] = cap_net(H, O, RELU_CAP * (1 - 1e-3))
    nets["cap_above"] = cap_net(H, O, RELU_CAP * (1 + 1e-3))
    if dtype == "f64":
        nets["tiny"] = tiny_net(H, O, rng)  # (no such values in f32)
    nets["zero"] = np.zeros(G)
    return nets


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("H,O", [(16, 3), (100, 2), (256, 4)])
def test_nonfinite_and_extreme_genes(gpu, bound_dir, H, O, dtype):
    """np.argmax's NaN rule (the first NaN wins), inf x 0 = NaN, the cap's two
    sides, f32-subnormal genes and the all-zero genome, through pg_relu_decide
    and pg_forward(f64); the expectations are numpy's own on the host."""
    nets = _extreme_nets(H, O, dtype)
    names = list(nets)
    genomes = _as_stored(np.array([nets[n] for n in names]), dtype)
    per = 24
    rng = np.random.default_rng([H, O, 44])
    k = rng.integers(0, 321, size=(len(names) * per, 6))
    gidx = np.repeat(np.arange(len(names)), per)
    ev = _relu_ev([6, H, O], gpu, dtype=DTYPES[dtype])
    index, stage, z32, bound, ref_idx, act = _decide(ev, gpu, genomes, k, gidx, dtype)
    m32, z64, want = _host(H, O, genomes, k, gidx)
    hb = _bounds(bound_dir, [(H, O, g) for g in genomes]).astype(np.float32)
    row = {n: gidx == i for i, n in enumerate(names)}
    # what the cases are meant to be, by numpy
    assert np.isnan(z64[row["nan_w1"]]).all() and (want[row["nan_w1"]] == 0).all()
    assert (want[row["nan_w2_row1"]] == 1).all() and not np.isnan(z64[row["nan_w2_row1"]][:, 0]).any()
    assert (want[row["nan_last_bias"]] == O - 1).all()
    for name, active in (("pinf_w2", np.inf), ("ninf_w2", -np.inf)):
        last = z64[row[name]][:, O - 1]
        assert np.isnan(last).any() and (last == active).any() and (np.isnan(last) | (last == active)).all()
    assert (want[row["ninf_w2"]] != O - 1).any() and (want[row["ninf_w2"]] == O - 1).any()
    assert (want[row["zero"]] == 0).all()
    # the device
    np.testing.assert_array_equal(index, want)
    np.testing.assert_array_equal(ref_idx, want)
    np.testing.assert_array_equal(act + 0.0, np.maximum(0.0, z64) + 0.0)
    assert set(np.unique(stage)) <= {0, 1}
    finite = {"cap_below", "zero", "tiny"} & set(names)
    for i, name in enumerate(names):
        b = bound[row[name]]
        assert (_bits(b) == _bits(b[:1])).all(), name
        if name in finite:
            assert np.isfinite(hb[i]) and abs(int(_bits(b)[0]) - int(_bits(hb[i:i + 1])[0])) <= 1, name
            z = z32[row[name]]
            assert np.isfinite(z).all(), name
            assert (np.abs(z.astype(np.float64) - z64[row[name]]).max(axis=1) <= b).all(), name
            if name != "tiny":  # (the device's f32 denormal mode may differ from numpy's)
                assert (_bits(z) == _bits(m32[row[name]])).all(), name
        else:
            assert np.isinf(hb[i]) and np.isinf(b).all() and (b > 0).all(), name
            assert (stage[row[name]] == 1).all(), name


# ------------------------------------------------- (d) k_relu games, all 18 ----
def _game_cases():
    hs = {4: (1, 64, 37), 8: (65, 128, 100), 16: (129, 256, 200)}
    for d, dtype in enumerate(("f64", "f32")):
        for LN in (4, 8, 16):
            for o, O in enumerate((2, 3, 4)):
                yield pytest.param(LN, O, dtype, hs[LN][(o + d) % 3], id=f"LN{LN}-O{O}-{dtype}-H{hs[LN][(o + d) % 3]}")


PERMUTED = {(4, 3, "f64"), (8, 4, "f32"), (16, 2, "f64")}


@pytest.mark.parametrize("LN,O,dtype,H", list(_game_cases()))
def test_relu_games_every_instance(gpu, LN, O, dtype, H):
    """32 genomes x 6 games (scripted, ROM CPU, score-aware and hall-of-fame
    opponents; the second half of the rows all hall-of-fame) of one k_relu
    instance against the general kernel.  Genome rows 0..3 and opponent rows
    0..1 always need the f64 forward (a tie network, a 1e30 weight, the
    all-zero genome, for f64 a NaN gene) and share groups and waves with
    networks that almost never do."""
    assert _relu_lanes(H) == LN
    shape = [6, H, O]
    rng = np.random.default_rng([LN, O, dtype == "f32", 45])
    G = _genes(H, O)
    n, n_opp, games = 32, 8, 6
    genomes, opponents = rng.standard_normal((n, G)), rng.standard_normal((n_opp, G))
    genomes[0] = tie_net(H, O, rng)
    genomes[1, 5] = 1e30
    genomes[2] = 0.0
    always = [0, 1, 2]
    if dtype == "f64":
        genomes[3, H * 7 + H // 2] = np.nan
        always.append(3)
    opponents[0] = tie_net(H, O, rng)
    opponents[1, H * 7 - 2] = -1e30
    always_opp = [0, 1]
    genomes, opponents = _as_stored(genomes, dtype), _as_stored(opponents, dtype)
    assert np.isfinite(opponents).all() and np.isfinite(np.delete(genomes, 3, axis=0)).all()
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (n, 1))
    kinds[n // 2:] = 3
    opp = rng.integers(0, n_opp, size=(n, games)).astype(np.int32)
    mult = np.round(rng.normal(size=(n, games)), 3)
    assert (mult < 0).any() and (mult > 0).any()
    gt, ot = dev_genomes(genomes, gpu, DTYPES[dtype]), dev_genomes(opponents, gpu, DTYPES[dtype])
    sched = [torch.tensor(a, device=gpu) for a in (kinds, opp, mult)]
    ev = _relu_ev(shape, gpu, dtype=DTYPES[dtype], timeout_thresh=119, win_score=1)
    cap = 2048
    hot, hot_tr = ev.evaluate(gt, *sched, opponents=ot, kernel="relu", trace_games=n * games, trace_cap=cap)
    ref, ref_tr = ev.evaluate(gt, *sched, opponents=ot, kernel="general", trace_games=n * games, trace_cap=cap)
    torch.cuda.synchronize()
    same(hot, ref)
    assert torch.equal(hot_tr, ref_tr) and int(hot_tr.any())
    ch, cr = hot.counters.cpu().numpy(), ref.counters.cpu().numpy()
    assert (ch[[0, 1, 3]] == cr[[0, 1, 3]]).all() and ch[3] == n * games
    assert ch[2] == ch[4] <= ch[1]
    # the forwards of the rows that are never certified, from the general kernel's trace
    frames = ref.frames.cpu().numpy()
    assert frames.max() <= cap
    vis = ((ref_tr.cpu().numpy() >> 4) & 1).sum(axis=1).reshape(n, games)
    nn = kinds == 3
    assert ch[1] == cr[1] == (vis * (1 + nn)).sum()  # the idle left half of a scripted game counts no forward
    need = (vis[always].sum() + (vis * (nn & np.isin(opp, always_opp))).sum())
    assert need > 0 and ch[2] >= need, (ch[2], need)
    print(f"{shape} {dtype}: {ch[2]} f64 forwards of {ch[1]}, {need} of them by the rows that always need one")
    if (LN, O, dtype) in PERMUTED:
        perm = torch.tensor(rng.permutation(n).astype(np.int32), device=gpu)
        act = torch.tensor([19], dtype=torch.int32, device=gpu)
        hot2, _ = ev.evaluate(gt, *sched, opponents=ot, kernel="relu", rows=perm, n_active=act)
        ref2, _ = ev.evaluate(gt, *sched, opponents=ot, kernel="general", rows=perm, n_active=act)
        whole, _ = ev.evaluate(gt[perm.long()].contiguous(), *sched, opponents=ot, kernel="relu")
        torch.cuda.synchronize()
        same(hot2, ref2, 19)
        same(hot2, whole, 19)
        assert int(hot2.counters[3]) == 19 * games == int(ref2.counters[3])
