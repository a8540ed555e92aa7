"""The certified f32 families' refusals, word for word, without a GPU.

test_eval_refusals.py walks kernels 0..9; this test walks the seven certified
families (RELU, RELU2, SIG2, RELU2_BLOCK, SIG2_BLOCK, RELU3, SIG3) through
pg_eval_population and pg_eval_resolve, and each family's pg_*_decide entry
point, and compares every call's (return code, pg_last_error()) with
tests/golden/family_refusals.json.  The fixture holds the distinct outcomes
once and one index per case (the grid run-length encoded in walking order).
It was recorded from the library as it stood before the families' host sides
became one template behind one table:

    python tests/test_family_refusals.py --record

No call reaches a device.  Every pg_eval_population call has workspace = NULL,
so it ends at or before the workspace check; every pg_*_decide call is refused
or empty (n <= 0), so none reaches a launch.  A successful call is recorded as
(0, ""): pg_last_error() keeps an earlier call's text then.  A grid outcome is
[rc, message, resolve's rc, resolve's message]: pg_eval_resolve's value for the
same arguments is the kernel with the modifier bits in effect, or its refusal.

Per family the shapes are one inside scope, the widest one in scope, each width
one past its upper edge and one below its lower edge, O = 5, O = 1 and a wrong
layer count."""
import ctypes
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "family_refusals.json")

SIGMOID, RELU = 0, 1
# name: (pg_kernel, activation, a shape inside scope, each hidden width's (lower, upper) edge)
FAMILIES = {
    "relu": (6, RELU, [6, 20, 3], ((1, 256),)),
    "relu2": (7, RELU, [6, 20, 12, 3], ((2, 64), (2, 64))),
    "sig2": (9, SIGMOID, [6, 20, 12, 3], ((2, 64), (2, 64))),
    "relu2_block": (10, RELU, [6, 100, 70, 3], ((2, 128), (2, 128))),
    "sig2_block": (11, SIGMOID, [6, 100, 70, 3], ((2, 128), (2, 128))),
    "relu3": (12, RELU, [6, 20, 12, 9, 3], ((2, 32), (2, 32), (2, 32))),
    "sig3": (13, SIGMOID, [6, 20, 12, 9, 3], ((2, 32), (2, 32), (2, 32))),
}
BITS = (0, 0x100, 0x800, 0x900)  # none, advance, solo, both
ACTIVATIONS = (SIGMOID, RELU)
PRECISIONS = (0, 1, 7)  # certified, f64, out of range
N_GENOMES = (0, 4)
HORIZONS = (0, 5)
HARD_LOG = (False, True)
TRACE = (False, True)
BIAS = (True, False)


def _shapes(inside, edges):
    """The family's shape grid, the one inside scope first."""
    shapes = [list(inside), [6] + [hi for _, hi in edges] + [4]]
    for i, (lo, hi) in enumerate(edges):
        for width in (hi + 1, lo - 1):
            s = list(inside)
            s[1 + i] = width
            shapes.append(s)
    shapes += [inside[:-1] + [5], inside[:-1] + [1]]
    shapes += [inside[:-1] + [7, inside[-1]], [6, inside[-1]] if len(inside) == 3 else inside[:1] + inside[2:]]
    return shapes


def _genes(shape):
    return sum((shape[i] + 1) * shape[i + 1] for i in range(len(shape) - 1))


def _library():
    for p in (os.path.join(REPO, "neuro-genetic-pong-self-play_amd"), REPO):
        if p not in sys.path:
            sys.path.insert(0, p)
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib, _lib.lib()


def _outcome(lib, rc):
    return [0, ""] if rc == 0 else [rc, lib.pg_last_error().decode()]


REQUIRED = ("genomes", "game_kind", "game_opp", "game_mult", "fitness", "rewards", "scores", "frames", "total_frames",
            "status")


def _walk_eval(_lib, lib, ptr):
    grid = []
    for name, (kernel, _, inside, edges) in FAMILIES.items():
        for shape, bits, act, bias in itertools.product(_shapes(inside, edges), BITS, ACTIVATIONS, BIAS):
            a = _lib.PgEvalArgs()
            a.net = _lib.make_net(shape, bias, _lib.PG_F64, activation=act)
            a.kernel = kernel | bits
            a.n_games, a.genome_stride, a.trace_games, a.trace_cap, a.hard_cap = 6, 1 << 20, 1, 4, 4
            ref = ctypes.byref(a)
            for prec, n, horizon, hard, trace in itertools.product(PRECISIONS, N_GENOMES, HORIZONS, HARD_LOG, TRACE):
                a.precision, a.n_genomes, a.horizon = prec, n, horizon
                a.hard_log = ptr if hard else None
                a.trace = ptr if trace else None
                for field in REQUIRED:
                    setattr(a, field, ptr if n else None)
                played = _outcome(lib, lib.pg_eval_population(ref, None))  # workspace NULL: no device is touched
                resolved = lib.pg_eval_resolve(ref)
                grid.append(played + [resolved, lib.pg_last_error().decode() if resolved < 0 else ""])
    return grid


def _walk_decide(_lib, lib, ptr):
    """label -> outcome of every pg_*_decide call; none of them reaches a launch."""
    out = {}
    for name, (_, act, inside, edges) in FAMILIES.items():
        fn = getattr(lib, f"pg_{name}_decide")

        def call(label, shape=inside, bias=True, dtype=_lib.PG_F64, activation=act, n=0, stride=1 << 20, **null):
            a = _lib.PgReluDecideArgs()
            a.net = _lib.make_net(shape, bias, dtype, activation=activation)
            a.n, a.genome_stride = n, stride
            for field in ("genomes", "k", "index"):
                setattr(a, field, None if null.get(field, "ptr") is None else ptr)
            assert n <= 0 or not (a.genomes and a.k and a.index) or stride < _genes(shape), "this call would launch"
            out[f"{name}: {label}"] = _outcome(lib, fn(ctypes.byref(a), None))

        out[f"{name}: args NULL"] = _outcome(lib, fn(None, None))
        call("dtype 7", dtype=7)
        call("dtype 7, wrong activation", dtype=7, activation=1 - act)
        call("wrong activation", activation=1 - act)
        call("wrong activation, out of shape", activation=1 - act, shape=[6, 300, 300, 300, 300, 3])
        call("activation 5", activation=5)
        for shape, bias, n in itertools.product(_shapes(inside, edges), BIAS, (-1, 0)):
            call(f"shape {shape} bias {int(bias)} n {n}", shape=shape, bias=bias, n=n)
        for dtype in (_lib.PG_F32, _lib.PG_F64):
            call(f"n 0, dtype {dtype}", dtype=dtype)
        for shape in _shapes(inside, edges)[:2]:
            for field in ("genomes", "k", "index"):
                call(f"shape {shape} n 3, {field} NULL", shape=shape, n=3, **{field: None})
            call(f"shape {shape} n 3, stride one short", shape=shape, n=3, stride=_genes(shape) - 1)
            call(f"shape {shape} n 3, stride 0, all NULL", shape=shape, n=3, stride=0, genomes=None, k=None, index=None)
    return out


def _walk():
    _lib, lib = _library()
    dummy = (ctypes.c_uint64 * 64)()  # behind every non-NULL pointer; nothing dereferences it
    ptr = ctypes.addressof(dummy)
    return _walk_eval(_lib, lib, ptr), _walk_decide(_lib, lib, ptr)


def _encode(grid, decide):
    outcomes, index = [], {}

    def idx(o):
        if tuple(o) not in index:
            index[tuple(o)] = len(outcomes)
            outcomes.append(o)
        return index[tuple(o)]

    runs = []  # [outcome, count, outcome, count, ...]
    for o in grid:
        i = idx(o)
        if runs and runs[-2] == i:
            runs[-1] += 1
        else:
            runs += [i, 1]
    return {"outcomes": outcomes, "grid_runs": runs, "decide": {label: idx(o) for label, o in decide.items()}}


def _decode_grid(fixture):
    runs = fixture["grid_runs"]
    return [i for i, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]


def test_refusals_match_the_recording():
    with open(FIXTURE) as fh:
        fixture = json.load(fh)
    outcomes = fixture["outcomes"]
    grid, decide = _walk()
    want = _decode_grid(fixture)
    assert len(grid) == len(want)
    wrong = [(n, got, outcomes[w]) for n, (got, w) in enumerate(zip(grid, want)) if got != outcomes[w]]
    assert not wrong, f"{len(wrong)} of {len(grid)} grid cases differ; the first (case, got, recorded): {wrong[:3]}"
    assert sorted(decide) == sorted(fixture["decide"])
    for label, got in decide.items():
        assert got == outcomes[fixture["decide"][label]], label


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_family_refusals.py --record")
    recorded = _encode(*_walk())
    with open(FIXTURE, "w") as fh:
        json.dump(recorded, fh, separators=(",", ":"))
        fh.write("\n")
    for outcome in recorded["outcomes"]:
        print(*outcome)
    print(f"{len(_decode_grid(recorded))} grid cases, {len(recorded['decide'])} decide calls, "
          f"{len(recorded['outcomes'])} distinct outcomes")
