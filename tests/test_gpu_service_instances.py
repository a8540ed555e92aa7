"""Every instance of k_service (csrc/pg_service.hpp: 17 lane layouts (L, U) x
O in {2, 3, 4} x f32 / f64 genes = 102) and of k_decide (csrc/pg_decide.hip:
the 7 layouts of the auto choice x 3 x 2 = 42) on the MI355X (run with -m gpu),
bit for bit against the CPU oracle:

  (a) whole games of every k_service instance at the lowest and the highest
      hidden width it serves, with and without bias, on a population whose
      first rows are the all-zero network, a weight over kWeightCap, a NaN and
      the two infinities (pg_cascade.hpp's e = inf path); the traced launch
      (which steps every frame) against the general f64 kernel's trace; a
      single, mostly empty block; the refusals past each layout's width;
  (b) pg_decide on the same widths: the index against pg_forward(f64) and the
      oracle, and where each stage of the cascade may and must appear;
  (c) the lane records prepared in two calls off the bench layout.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from _gpu_support import assert_same, dev_genomes, gene_count

pytestmark = pytest.mark.gpu

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neuro-genetic-pong-self-play_amd",
                   "csrc", "pg_f64math.h")

DTYPES = {"f32": torch.float32, "f64": torch.float64}
OUTS = (2, 3, 4)
LANES = (8, 16, 32, 64)
# the lowest and the highest hidden width of every units-per-lane step of every lane count, and H = 3
HS = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256)
# the 17 layouts (lanes per game, hidden units per lane) the split dispatch instantiates
LAYOUTS = {(8, 1), (8, 2), (8, 4), (8, 8), (8, 16)} | {(L, U) for L in (16, 32, 64) for U in (1, 2, 4, 8)}
N, GAMES, N_OPP = 37, 6, 6  # 222 games: no multiple of any block's game count


def _service_units(L, H):
    """service_units() of csrc/pg_service.hpp: the units per lane the split
    dispatch instantiates for (L, H); 0 = no instance holds H on L lanes."""
    if L == 8 and 32 < H <= 64:
        return 16
    for u in (1, 2, 4, 8):
        if (L // 2) * u >= H:
            return u
    return 0


def _workspace_bytes(L, H, O):
    """pg_eval_workspace_bytes of a split launch of the N genomes and N_OPP
    opponents (csrc/pong_ga.hip): the game counters, a flag per game, then one
    lane record of rec_floats<U, O>() floats per half-group lane and network --
    sized for U = 16 on 8 lanes up to H = 64, else for the instance's U (one
    size for U = 1 and 2), so the library's own service_units() shows in it."""
    U = 16 if L == 8 and H <= 64 else _service_units(L, H)
    floats = ((U + 1) // 2 * 2 * (7 + O) + O + 1 + 3) // 4 * 4
    return 256 + -(-N * GAMES * 4 // 256) * 256 + -(-(N + N_OPP) * (L // 2) * floats * 4 // 256) * 256


def _decide_layout(H):
    """(L, U) of pg_decide: choose_split_lanes() of csrc/pong_ga.hip, then the
    first of launch_decide's layouts on L that holds H."""
    L = 8 if H <= 64 else (32 if H <= 128 else 64)
    for u in ((1, 2, 4, 8, 16) if L == 8 else (8,)):
        if (L // 2) * u >= H:
            return L, u
    return None


def _nobias_out(H, dtype):
    """The one O a (H, dtype) plays without bias: rotating, so that every O
    meets bias=False on every lane count (checked by test_cells_cover_...)."""
    return OUTS[(HS.index(H) + (dtype == "f32")) % 3]


def _cells():
    """(H, O, bias, dtype): bias on for every O and both gene types, bias off for one O each."""
    for H in HS:
        for dtype in ("f64", "f32"):
            for O in OUTS:
                yield H, O, True, dtype
            yield H, _nobias_out(H, dtype), False, dtype


def _game_params():
    for H, O, bias, dtype in _cells():
        for L in LANES:
            if _service_units(L, H):
                yield pytest.param(H, O, bias, dtype, L, id=f"H{H}-O{O}-{'bias' if bias else 'nobias'}-{dtype}-L{L}")


def _as_stored(a, dtype):
    """The genes as the kernel reads them: f32 populations hold the rounded values."""
    a = np.asarray(a, np.float64)
    if dtype == "f32":
        with np.errstate(all="ignore"):
            a = a.astype(np.float32).astype(np.float64)
    return a


def _special_rows(rows, rng):
    """Rows 0..4: all zeros; one gene 1e31 (over kWeightCap = 1e30, finite in
    f32); one gene NaN; one +inf; one -inf -- rows 1..4 get e = inf."""
    G = rows.shape[1]
    rows[0] = 0.0
    for r, v in ((1, 1e31), (2, np.nan), (3, np.inf), (4, -np.inf)):
        rows[r, rng.integers(G)] = v


def _population(H, O, bias, dtype):
    rng = np.random.default_rng([H, O, int(bias), dtype == "f32", 61])
    G = gene_count([6, H, O], bias)
    quarters = np.array_split(np.arange(N), 4)
    genomes = np.empty((N, G))
    genomes[quarters[0]] = rng.standard_normal((len(quarters[0]), G))
    genomes[quarters[1]] = rng.standard_normal((len(quarters[1]), G)) * 3.0
    genomes[quarters[2]] = rng.random((len(quarters[2]), G))
    genomes[quarters[3]] = rng.standard_normal((len(quarters[3]), G)) * 9.0
    _special_rows(genomes, rng)
    opponents = rng.standard_normal((N_OPP, G)) * 3.0
    kinds = np.tile(np.array([0, 1, 2, 3, 3, 3], np.int32), (N, 1))
    opp = rng.integers(0, N_OPP, size=(N, GAMES)).astype(np.int32)
    mult = np.ones((N, GAMES))
    mult[kinds == 3] = np.round(rng.normal(size=int((kinds == 3).sum())), 3)
    return _as_stored(genomes, dtype), _as_stored(opponents, dtype), kinds, opp, mult


def _sched(gpu, kinds, opp, mult, rows=slice(None)):
    return [torch.tensor(np.ascontiguousarray(a[rows]), device=gpu) for a in (kinds, opp, mult)]


_CELL = {}  # the last cell's population and references: the lane counts of a cell run back to back


def _cell(gpu, oracle, H, O, bias, dtype):
    """The cell's population on the device, the oracle's results for it (and
    for rows 0 and 2 alone) and the general f64 kernel's trace of every game."""
    key = (H, O, bias, dtype)
    if _CELL.get("key") == key:
        return _CELL
    from pong_amd.device import Evaluator
    shape, dt = [6, H, O], DTYPES[dtype]
    genomes, opponents, kinds, opp, mult = _population(H, O, bias, dtype)
    ref = oracle.eval_population(genomes, shape, kinds, opp, mult, opponents=opponents, bias=bias, n_threads=8)
    assert (ref["status"] == 0).all() and np.isfinite(ref["fitness"]).all()
    ones = {r: oracle.eval_population(genomes[[r]], shape, kinds[[r]], opp[[r]], mult[[r]], opponents=opponents,
                                      bias=bias, n_threads=8) for r in (0, 2)}
    gt, ot = dev_genomes(genomes, gpu, dt), dev_genomes(opponents, gpu, dt)
    sched = _sched(gpu, kinds, opp, mult)
    cap = int(ref["frames"].max()) + 1
    gen = Evaluator(shape, bias=bias, dtype=dt, device=gpu, kernel="general", precision="f64")
    res, trace = gen.evaluate(gt, *sched, opponents=ot, trace_games=N * GAMES, trace_cap=cap)
    torch.cuda.synchronize()
    assert_same(res, ref)
    assert int(trace.any())
    _CELL.clear()
    _CELL.update(key=key, genomes=genomes, kinds=kinds, opp=opp, mult=mult, ref=ref, ones=ones, gt=gt, ot=ot,
                 sched=sched, cap=cap, trace=trace)
    return _CELL


# ------------------------------------------- the cells reach every instance ----
def test_cells_cover_every_instance():
    """The union over the cells below: all 102 k_service and all 42 k_decide
    instances, and every O without bias on every lane count."""
    service = {(L, _service_units(L, H), O, dtype) for H, O, _, dtype in _cells() for L in LANES
               if _service_units(L, H)}
    assert service == {(L, U, O, dtype) for L, U in LAYOUTS for O in OUTS for dtype in DTYPES}
    assert len(service) == 102
    nobias = {(L, O) for H, O, bias, _ in _cells() if not bias for L in LANES if _service_units(L, H)}
    assert nobias == {(L, O) for L in LANES for O in OUTS}
    for L, U in LAYOUTS:  # each layout at the lowest and the highest width it serves
        lo, hi = (1 if U == 1 else (L // 2) * (U // 2) + 1), (L // 2) * U
        assert _service_units(L, lo) == _service_units(L, hi) == U and lo in HS and hi in HS, (L, U)
    decide = {_decide_layout(H) + (O, dtype) for H, O, dtype in _decide_cells()}
    assert {d[:2] for d in decide} == {(8, 1), (8, 2), (8, 4), (8, 8), (8, 16), (32, 8), (64, 8)}
    assert len(decide) == 42


# -------------------------------------- (a) whole games of every k_service ----
@pytest.mark.parametrize("H,O,bias,dtype,L", list(_game_params()))
def test_service_games_every_instance(gpu, oracle, H, O, bias, dtype, L):
    """37 genomes x 6 games (the reference schedule, 6 hall members) of one
    k_service instance at one hidden width against the oracle."""
    from pong_amd.device import Evaluator
    c = _cell(gpu, oracle, H, O, bias, dtype)
    ref, total = c["ref"], N * GAMES
    U = _service_units(L, H)
    ev = Evaluator([6, H, O], bias=bias, dtype=DTYPES[dtype], device=gpu, kernel="split", group_lanes=L)
    res, _ = ev.evaluate(c["gt"], *c["sched"], opponents=c["ot"])
    torch.cuda.synchronize()
    assert ev._ws.numel() == _workspace_bytes(L, H, O)  # the library's units per lane for (L, H) are this file's
    n = res.counters.cpu().numpy().astype(np.int64)
    print(f"[6,{H},{O}] bias={int(bias)} {dtype} L{L}U{U}: numpy-order f64 [2]={n[2]} certificate failures [4]={n[4]} "
          f"certified f64 [5]={n[5]} in-wave [6]={n[6]} rally frames [8]={n[8]} serve-delay frames [12]={n[12]} "
          f"of {int(ref['frames'].sum())} frames, longest game {c['cap'] - 1}")
    assert_same(res, ref)
    assert n[3] == total and n[0] + n[8] + n[12] == ref["frames"].sum(), n
    # the all-zero network's outputs are exactly equal on every frame: no f32 rule and no certified
    # f64 rule tells them apart, so every instance reaches the numpy-order forward
    assert n[4] > 0 and n[2] > 0, n
    # traced: every frame stepped, both paddles' actions of every frame the general f64 kernel's
    res_t, trace = ev.evaluate(c["gt"], *c["sched"], opponents=c["ot"], trace_games=total, trace_cap=c["cap"])
    torch.cuda.synchronize()
    t = res_t.counters.cpu().numpy().astype(np.int64)
    assert_same(res_t, ref)
    assert t[8] == 0 and t[12] == 0 and t[0] == ref["frames"].sum() and t[3] == total, t
    assert torch.equal(trace, c["trace"])
    # one genome: a single, mostly empty block
    for r in (0, 2):
        one, _ = ev.evaluate(c["gt"][r:r + 1].contiguous(), *_sched(gpu, c["kinds"], c["opp"], c["mult"], [r]),
                             opponents=c["ot"])
        torch.cuda.synchronize()
        assert_same(one, c["ones"][r])
        assert int(one.counters[3]) == GAMES


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("H,L", [(65, 8), (65, 16), (129, 32), (257, 8), (257, 16), (257, 32), (257, 64), (257, 0)])
def test_service_refuses_what_no_instance_holds(gpu, H, L, dtype):
    """A hidden width past what L lanes hold (L = 0: the auto choice) is
    refused with PG_ERR_UNSUPPORTED before anything is launched."""
    from pong_amd import _lib
    from pong_amd.device import EvalResult, Evaluator
    assert H > 256 or _service_units(L, H) == 0
    genomes, opponents, kinds, opp, mult = _population(H, 3, True, dtype)
    ev = Evaluator([6, H, 3], dtype=DTYPES[dtype], device=gpu, kernel="split", group_lanes=L)
    gt, ot = dev_genomes(genomes, gpu, DTYPES[dtype]), dev_genomes(opponents, gpu, DTYPES[dtype])
    sched = _sched(gpu, kinds, opp, mult)
    # marked result arrays: the refused call must leave them as they are

    def marked(shape, dt):
        return torch.full(shape, -3.5 if dt == torch.float64 else 7, dtype=dt, device=gpu)

    out = EvalResult(fitness=marked((N,), torch.float64), rewards=marked((N, GAMES), torch.float64),
                     scores=marked((N, GAMES, 2), torch.int32), frames=marked((N, GAMES), torch.int32),
                     total_frames=marked((N, GAMES), torch.float64), status=marked((N,), torch.int32),
                     counters=marked((16,), torch.int64))
    fields = [out.fitness, out.rewards, out.scores, out.frames, out.total_frames, out.status, out.counters]
    with pytest.raises(_lib.PongGAError) as err:
        ev.evaluate(gt, *sched, opponents=ot, out=out)
    assert err.value.code == _lib.PG_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool(torch.all(f == (-3.5 if f.dtype == torch.float64 else 7))) for f in fields)


# --------------------------------------------- (b) every k_decide instance ----
def _decide_cells():
    for H in HS:
        if H != 3:
            for O in OUTS:
                for dtype in ("f64", "f32"):
                    yield H, O, dtype


def _run_decide(ev, gpu, gt, k, gidx):
    kt = torch.tensor(k.astype(np.int32), device=gpu)
    it = torch.tensor(gidx.astype(np.int32), device=gpu)
    index, stage = ev.decide(gt, kt, genome_index=it)
    # the features as the kernels make them from the doubled centroids: (k / 2) / 160 (utils.inference)
    want, _ = ev.forward(gt, dev_genomes((k / 2) / 160, gpu), genome_index=it, precision="f64", want_act=False)
    torch.cuda.synchronize()
    return index.cpu().numpy(), stage.cpu().numpy(), want.cpu().numpy()


@pytest.mark.parametrize("H,O,dtype", list(_decide_cells()))
def test_decide_every_instance(gpu, oracle, H, O, dtype):
    """40 networks (eight each U[0,1), N(0,1), N(0,3), N(0,9), N(0,30); then
    the five special rows) x 37 passes through pg_decide: the decision is
    pg_forward(f64)'s and the oracle's, and each stage appears where the
    cascade allows it."""
    from pong_amd.device import Evaluator
    shape = [6, H, O]
    rng = np.random.default_rng([H, O, dtype == "f32", 67])
    G = gene_count(shape)
    nets = np.concatenate([rng.random((8, G))] + [rng.standard_normal((8, G)) * s for s in (1.0, 3.0, 9.0, 30.0)])
    _special_rows(nets, rng)
    nets = _as_stored(nets, dtype)
    n_nets, per = len(nets), 37
    k = rng.integers(0, 321, size=(n_nets * per, 6))
    k[0::per], k[1::per] = 0, 320
    gidx = np.repeat(np.arange(n_nets), per)
    ev = Evaluator(shape, dtype=DTYPES[dtype], device=gpu)
    gt = dev_genomes(nets, gpu, DTYPES[dtype])
    index, stage, want = _run_decide(ev, gpu, gt, k, gidx)
    hist = np.bincount(stage, minlength=5)
    print(f"{shape} {dtype} L{_decide_layout(H)[0]}U{_decide_layout(H)[1]}: stages 0..4 {hist.tolist()}, "
          f"N(0,1) networks {np.bincount(stage[(gidx >= 8) & (gidx < 16)], minlength=5).tolist()}")
    np.testing.assert_array_equal(index, want)
    sample = np.concatenate([np.flatnonzero(gidx < 5), rng.choice(np.flatnonzero(gidx >= 5), size=64, replace=False)])
    with np.errstate(all="ignore"):
        for t in sample:
            assert index[t] == oracle.nn_run(nets[gidx[t]], shape, (k[t] / 2) / 160)[0], (t, gidx[t])
    assert stage.min() >= 0 and stage.max() <= 4
    # stage 4 (the frame's own bound) exists on the bench layout L = 8, U = 16 alone
    assert 33 <= H <= 64 or hist[4] == 0
    # rows 1..4 have e = inf: no f32 rule may decide them, under either bound
    assert np.isin(stage[(gidx >= 1) & (gidx <= 4)], (2, 3)).all()
    # the all-zero network's equal outputs are told apart by no certified rule
    assert (stage[gidx == 0] == 3).all() and (index[gidx == 0] == 0).all()
    assert hist[3] > 0
    assert 2 * np.count_nonzero(stage[(gidx >= 8) & (gidx < 16)] == 0) > 8 * per
    # n = 1: one pass of one mostly empty wave
    t = 9 * per + 5
    i1, s1, w1 = _run_decide(ev, gpu, gt, k[t:t + 1], gidx[t:t + 1])
    assert (i1[0], s1[0], w1[0]) == (index[t], stage[t], want[t])


def _near_tie_nets(H, O, rng):
    """Eight networks whose first two outputs are (nearly) the same row of W2,
    so that the f32 certificate fails and the later stages decide: 0..3 on
    N(0,1) genes (outputs far below saturation), 4..7 with output biases of
    30 or 34 (the plateau regime, 22.2 <= z < 53 ln 2).  `step` is the relative
    change of the second row's largest weight; 0 = an exact copy."""
    G, w2, row = gene_count([6, H, O]), H * 7, H + 1
    nets = rng.standard_normal((8, G))
    cases = [(0.0, None), (2.0 ** -22, None), (2.0 ** -16, None), (2.0 ** -22, None),
             (0.0, 30.0), (2.0 ** -22, 30.0), (None, 30.0), (2.0 ** -12, 34.0)]
    for g, (step, c) in zip(nets, cases):
        if c is not None:
            g[w2:] /= np.sqrt(H)
            g[w2 + H::row] = c
    nets = nets.astype(np.float32).astype(np.float64)  # every gene an f32 value, whatever the gene type
    for i, (g, (step, c)) in enumerate(zip(nets, cases)):
        if step is None:
            continue
        first = g[w2: w2 + row].copy()
        if step == 0.0:  # every output the same row: equal outputs
            g[w2:] = np.tile(first, O)
            continue
        dup = O - 1 if i == 3 else 1  # (net 3: the last row copies the first)
        g[w2 + dup * row: w2 + (dup + 1) * row] = first
        j = int(np.argmax(np.abs(first[:H])))
        g[w2 + dup * row + j] = np.float32(first[j]) * np.float32(1.0 + step)
        if c is None:  # the other outputs far below the pair
            for o in range(1, O):
                if o != dup:
                    g[w2 + o * row + H] = -200.0
    return nets


@pytest.fixture(scope="module")
def host_sigmoid(tmp_path_factory):
    """pg_sigmoid_f64 (csrc/pg_f64math.h) compiled for the host, on an array."""
    d = tmp_path_factory.mktemp("f64math")
    src, exe = d / "s.c", d / "s"
    src.write_text(f'#include <stdio.h>\n#include "{HDR}"\n'
                   "int main(void){ double z; while (scanf(\"%la\", &z) == 1) "
                   "printf(\"%a\\n\", pg_sigmoid_f64(z)); return 0; }\n")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe), str(src), "-lm"])

    def run(z):
        out = subprocess.run([str(exe)], input="\n".join(float(v).hex() for v in np.ravel(z)), capture_output=True,
                             text=True, check=True).stdout.split()
        return np.array([float.fromhex(v) for v in out]).reshape(np.shape(z))
    return run


def _f64_model(oracle, host_sigmoid, g, H, O, x):
    """The device's numpy-order f64 forward on the host: every np.dot in
    OpenBLAS's order (oracle.blas_gemv, pinned to np.dot by test_blas_order.py),
    every sigmoid pg_sigmoid_f64, np.argmax."""
    w1, w2 = g[:H * 7].reshape(H, 7), g[H * 7:].reshape(O, H + 1)
    h = host_sigmoid(np.array([oracle.blas_gemv(w1, np.append(v, 1.0)) for v in x]))
    return np.argmax(host_sigmoid(np.array([oracle.blas_gemv(w2, np.append(v, 1.0)) for v in h])), axis=1)


@pytest.mark.parametrize("H,O,dtype", list(_decide_cells()))
def test_decide_near_ties_every_instance(gpu, oracle, host_sigmoid, H, O, dtype):
    """The random networks above fail the certificate on a pass in a thousand;
    these fail it on most, so the cell's k_decide instance runs its plateau
    rules and the certified f64 decision: every index pg_forward(f64)'s and the
    oracle's.  The two networks of equal rows excepted: their outputs differ by
    the last bits of np.dot's sums alone (the rows' places in dgemv_t), so the
    decision turns on single roundings of the hidden sigmoids, where
    pg_sigmoid_f64's correctly rounded pow and the C library's behind the
    oracle differ by design (pg_f64math.h; [6,64,3] f32 has such a pass) --
    those are held to the device's f64 forward restated on the host."""
    from pong_amd.device import Evaluator
    shape = [6, H, O]
    rng = np.random.default_rng([H, O, dtype == "f32", 69])
    nets = _as_stored(_near_tie_nets(H, O, rng), dtype)
    per = 37
    k = rng.integers(0, 321, size=(len(nets) * per, 6))
    gidx = np.repeat(np.arange(len(nets)), per)
    ev = Evaluator(shape, dtype=DTYPES[dtype], device=gpu)
    index, stage, want = _run_decide(ev, gpu, dev_genomes(nets, gpu, DTYPES[dtype]), k, gidx)
    print(f"{shape} {dtype} L{_decide_layout(H)[0]}U{_decide_layout(H)[1]}: stages 0..4 per near-tie network "
          f"{[np.bincount(stage[gidx == i], minlength=5).tolist() for i in range(len(nets))]}")
    np.testing.assert_array_equal(index, want)
    x = (k / 2) / 160
    by_oracle = np.array([oracle.nn_run(nets[gidx[t]], shape, x[t])[0] for t in range(len(k))])
    equal_rows = np.isin(gidx, (0, 4))
    np.testing.assert_array_equal(index[~equal_rows], by_oracle[~equal_rows])
    for i in (0, 4):
        np.testing.assert_array_equal(index[gidx == i], _f64_model(oracle, host_sigmoid, nets[i], H, O, x[gidx == i]))
    if (index != by_oracle).any():
        print(f"  the oracle's pow decides {np.count_nonzero(index != by_oracle)} of the {2 * per} equal-row passes "
              "otherwise")
    assert stage.min() >= 0 and stage.max() <= 4 and (33 <= H <= 64 or not (stage == 4).any())
    # equal rows give equal f32 outputs bit for bit (the same chain): no gap to certify, below saturation
    assert (stage[np.isin(gidx, (0, 4))] != 0).all()
    # a 2^-22 step of one weight w moves the output by <= 2.4e-7 |w|, under the f32 bound's 2 u |w| (3 R + 5 + ...)
    # >= 1.2e-6 |w| and ~1e5 times the certified f64 bound: the f64 rules decide it
    assert 2 * np.count_nonzero(stage[np.isin(gidx, (1, 3))] == 2) > 2 * per


# ------------------------------- (c) two-call prep off the bench layout ----
@pytest.mark.parametrize("L,dtype", [(8, "f64"), (16, "f32"), (32, "f64"), (64, "f32")])
def test_prep_in_two_calls_off_the_bench_layout(gpu, L, dtype):
    """prep="genomes" then prep="rest" on [6,17,3] (L8U8, L16U4, L32U2, L64U1),
    with rows a permutation and n_active = n - 5: the games one call plays."""
    from pong_amd.device import Evaluator
    H, O = 17, 3
    genomes, opponents, kinds, opp, mult = _population(H, O, True, dtype)
    dt = DTYPES[dtype]
    ev = Evaluator([6, H, O], dtype=dt, device=gpu, kernel="split", group_lanes=L)
    gt, ot = dev_genomes(genomes, gpu, dt), dev_genomes(opponents, gpu, dt)
    sched = _sched(gpu, kinds, opp, mult)
    rng = np.random.default_rng([L, 71])
    rows = torch.tensor(rng.permutation(N).astype(np.int32), device=gpu)
    m = N - 5
    count = torch.tensor([m], dtype=torch.int32, device=gpu)

    def fields(r):
        return [r.fitness, r.rewards, r.scores, r.frames, r.total_frames, r.status, r.counters]

    one, _ = ev.evaluate(gt, *sched, opponents=ot, rows=rows, n_active=count)
    one = [t.clone() for t in fields(one)]
    out, _ = ev.evaluate(gt, *sched, opponents=ot, rows=rows, n_active=count)
    for t in fields(out):
        t.fill_(-3.5 if t.dtype == torch.float64 else 7)  # the counters too: the call zeroes them
    res, _ = ev.evaluate(gt, *sched, opponents=ot, rows=rows, n_active=count, out=out, prep="genomes")
    assert all(bool(torch.all(t == (-3.5 if t.dtype == torch.float64 else 7))) for t in fields(res))  # no games yet
    res, _ = ev.evaluate(gt, *sched, opponents=ot, rows=rows, n_active=count, out=out, prep="rest")
    torch.cuda.synchronize()
    for a, b in zip(one, fields(res)):
        if a.shape[0] == N:
            assert torch.equal(a[:m], b[:m])  # entries >= n_active are left untouched
        else:
            assert torch.equal(a, b)
    assert int(res.counters[3]) == m * GAMES
    # and the games are those of the permuted rows played as a plain population
    whole, _ = ev.evaluate(gt[rows.long()].contiguous(), *sched, opponents=ot)
    torch.cuda.synchronize()
    for a, b in zip(fields(whole)[:6], fields(res)[:6]):
        assert torch.equal(a[:m], b[:m])
