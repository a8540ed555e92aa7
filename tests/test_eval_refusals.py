"""pg_eval_population's refusals, word for word, without a GPU.

Every call here has workspace = NULL, so it ends at or before the workspace
check, and the library touches no device on that path (test_solo_host.py relies
on the same).  The test walks a fixed grid of arguments, then a list of single
overrides of one base call, and compares each call's (return code,
pg_last_error()) with tests/golden/eval_refusals.json.  The fixture holds the
distinct outcomes once and one index per case (the grid run-length encoded in
walking order).  It was recorded from the library as it stood before the
evaluation path's scope checks moved into the kernel families' units:

    python tests/test_eval_refusals.py --record

A successful call (an empty launch) is recorded as (0, ""): pg_last_error()
keeps an earlier call's text then.  Where the kernel resolves to WIDE or
RELU_WIDE the digits of "workspace of N bytes required" are masked (k_wide's
scratch is sized by the device's CU count); everywhere else the size is pinned.

Grid and overrides together reach every fail() of pg_eval_population up to the
workspace check.  Exempt, because they need a device or lie behind the
workspace check: the PG_HIP failures (hipMemsetAsync, hipGetLastError), the
refusals at the launch (the shapes and precision of RELU, SPLIT and WIDE, the
retired RESIDENT / STAGED, the general kernel's LDS limit, "kernel=%d"),
anything inside a launch_* function, and the "sig2" wording of "activation
relu: the %s kernel evaluates sigmoid networks only", which the sig2 kernel's
own refusal of a ReLU network precedes."""
import ctypes
import itertools
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "eval_refusals.json")

KERNELS = tuple(range(10)) + (99,)
BITS = (0, 0x100, 0x800, 0x900, 0x200)  # none, advance, solo, both, an unknown bit
ACTIVATIONS = (0, 1)
SHAPES = (([6, 64, 3], True), ([6, 300, 3], True), ([6, 16, 16, 3], True), ([6, 65, 16, 3], True),
          ([6, 100, 100, 3], True), ([6, 600, 16, 3], True), ([6, 16, 16, 5], True), ([6, 4, 4, 4, 2], True),
          ([5, 8, 3], True), ([6, 64, 3], False), ([6, 16, 16, 3], False))
PRECISIONS = (0, 1, 7)
N_GENOMES = (0, 4)
N_GAMES = (6, 9)
HORIZONS = (0, 5)
HARD_LOG = (False, True)
TRACE = (False, True)
DTYPES = (0, 1)

# one field (or a few) of the base call changed: [6, 64, 3] sigmoid with bias, f64 genes, AUTO, certified, 4 genomes x 6 games
EXTRAS = (
    ("base", {}),
    ("args NULL", None),
    ("struct_size", {"struct_size": 8}),
    ("n_nodes 1", {"net.n_nodes": 1}),
    ("n_nodes 10", {"net.n_nodes": 10}),
    ("nodes[1] 0", {"nodes": [6, 0, 3]}),
    ("nodes[1] 70000", {"nodes": [6, 70000, 3]}),
    ("dtype 7", {"net.dtype": 7}),
    ("activation 5", {"net.activation": 5}),
    ("network too large", {"nodes": [6, 65536, 65536, 3]}),
    ("n_genomes -1", {"n_genomes": -1}),
    ("n_games 0", {"n_games": 0}),
    ("n_games 65", {"n_games": 65}),
    ("n_games 64", {"n_games": 64}),
    ("horizon -1", {"horizon": -1}),
    ("timeout_thresh 5", {"timeout_thresh": 5}),
    ("timeout_thresh 32", {"timeout_thresh": 32}),
    ("timeout_thresh 2^20+1", {"timeout_thresh": (1 << 20) + 1}),
    ("win_score -1", {"win_score": -1}),
    ("win_score 5", {"win_score": 5}),
    ("kernel -1", {"kernel": -1}),
    ("kernel 0x400", {"kernel": 0x400}),
    ("kernel 0x10003", {"kernel": 0x10003}),
    ("too many games", {"n_genomes": 0x7fffffff}),
    ("genomes NULL", {"genomes": None}),
    ("genome_stride 1", {"genome_stride": 1}),
    ("game_kind NULL", {"game_kind": None}),
    ("status NULL", {"status": None}),
    ("opponents NULL", {"n_opponents": 2}),
    ("opponent_stride 1", {"n_opponents": 2, "opponents": "ptr", "opponent_stride": 1}),
    ("opponents", {"n_opponents": 2, "opponents": "ptr", "opponent_stride": 1 << 20}),
    ("trace_cap 0", {"trace": "ptr", "trace_cap": 0}),
    ("trace_games -1", {"trace": "ptr", "trace_cap": 4, "trace_games": -1}),
    ("prep 3", {"prep": 3}),
    ("prep -1", {"prep": -1}),
    ("prep genomes", {"prep": 1}),
    ("prep genomes, general", {"prep": 1, "kernel": 1}),
    ("group_lanes 16", {"group_lanes": 16}),
    ("group_lanes 32", {"group_lanes": 32}),
    ("group_lanes 64", {"group_lanes": 64}),
    ("group_lanes 4", {"group_lanes": 4}),
    ("H 200", {"nodes": [6, 200, 3]}),
    ("H 20 O 4", {"nodes": [6, 20, 4]}),
    ("4096 genomes", {"n_genomes": 4096}),
    ("4096 genomes, general", {"n_genomes": 4096, "kernel": 1}),
    ("horizon on split", {"horizon": 5}),
    ("horizon on split, traced", {"horizon": 5, "trace": "ptr", "trace_cap": 4}),
)


def _library():
    for p in (os.path.join(REPO, "neuro-genetic-pong-self-play_amd"), REPO):
        if p not in sys.path:
            sys.path.insert(0, p)
    from pong_amd import _lib
    from pong_amd import build as B
    B.build()
    return _lib, _lib.lib()


def _resolves_wide(kernel, shape, activation):
    named = kernel & 0xff
    if named in (4, 8):
        return True
    return (named == 0 and activation == 0 and len(shape) == 4 and shape[0] == 6 and 2 <= shape[3] <= 4 and
            all(2 <= h <= 512 for h in shape[1:3]) and max(shape[1:3]) >= 64)


def _outcome(lib, rc, mask):
    if rc == 0:
        return [0, ""]
    msg = lib.pg_last_error().decode()
    if mask:
        msg = re.sub(r"workspace of \d+ bytes required", "workspace of N bytes required", msg)
    return [rc, msg]


REQUIRED = ("genomes", "game_kind", "game_opp", "game_mult", "fitness", "rewards", "scores", "frames", "total_frames",
            "status")


def _walk():
    """Every case's outcome: the grid in walking order, then the overrides by name."""
    _lib, lib = _library()
    dummy = (ctypes.c_uint64 * 64)()  # behind every non-NULL pointer; nothing dereferences it
    ptr = ctypes.addressof(dummy)
    grid = []
    for kernel, bits, act, (shape, bias), dtype in itertools.product(KERNELS, BITS, ACTIVATIONS, SHAPES, DTYPES):
        a = _lib.PgEvalArgs()
        a.net = _lib.make_net(shape, bias, dtype, activation=act)
        a.kernel = kernel | bits
        a.genome_stride, a.trace_games, a.trace_cap, a.hard_cap = 1 << 20, 1, 4, 4
        mask = _resolves_wide(kernel, shape, act)
        ref = ctypes.byref(a)
        for prec, n, games, horizon, hard, trace in itertools.product(PRECISIONS, N_GENOMES, N_GAMES, HORIZONS,
                                                                      HARD_LOG, TRACE):
            a.precision, a.n_genomes, a.n_games, a.horizon = prec, n, games, horizon
            a.hard_log = ptr if hard else None
            a.trace = ptr if trace else None
            for name in REQUIRED:
                setattr(a, name, ptr if n else None)
            grid.append(_outcome(lib, lib.pg_eval_population(ref, None), mask))
    extras = {}
    for label, over in EXTRAS:
        if over is None:
            extras[label] = _outcome(lib, lib.pg_eval_population(None, None), False)
            continue
        over = dict(over)
        a = _lib.PgEvalArgs()
        a.net = _lib.make_net(over.pop("nodes", [6, 64, 3]), True, _lib.PG_F64)
        a.n_genomes, a.n_games, a.genome_stride = 4, 6, 1 << 20
        for name in REQUIRED:
            setattr(a, name, ptr)
        for key, value in over.items():
            value = ptr if value == "ptr" else value
            if key.startswith("net."):
                setattr(a.net, key[4:], value)
            else:
                setattr(a, key, value)
        extras[label] = _outcome(lib, lib.pg_eval_population(ctypes.byref(a), None), False)
    return grid, extras


def _encode(grid, extras):
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
    return {"outcomes": outcomes, "grid_runs": runs, "extras": {label: idx(o) for label, o in extras.items()}}


def _decode_grid(fixture):
    runs = fixture["grid_runs"]
    return [i for i, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]


def test_refusals_match_the_recording():
    with open(FIXTURE) as fh:
        fixture = json.load(fh)
    outcomes = fixture["outcomes"]
    grid, extras = _walk()
    want = _decode_grid(fixture)
    assert len(grid) == len(want)
    wrong = [(n, got, outcomes[w]) for n, (got, w) in enumerate(zip(grid, want)) if got != outcomes[w]]
    assert not wrong, f"{len(wrong)} of {len(grid)} grid cases differ; the first (case, got, recorded): {wrong[:3]}"
    assert sorted(extras) == sorted(fixture["extras"])
    for label, got in extras.items():
        assert got == outcomes[fixture["extras"][label]], label


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_eval_refusals.py --record")
    recorded = _encode(*_walk())
    with open(FIXTURE, "w") as fh:
        json.dump(recorded, fh, separators=(",", ":"))
        fh.write("\n")
    for rc, msg in recorded["outcomes"]:
        print(rc, msg)
    print(f"{len(_decode_grid(recorded))} grid cases, {len(recorded['extras'])} overrides, "
          f"{len(recorded['outcomes'])} distinct outcomes")
