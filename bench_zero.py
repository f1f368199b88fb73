"""ZERO-term problems in graph form (problems.basis_pursuit / hinge_l1 / deadzone_l1 / logreg_l1): a fixed number
of sweeps on each route of the option "fused_zero" - "0" the generic operator path, "auto" the fused
sweep (one pass over the data matrix, one row kernel, the inverse apply) - on one GPU.

Both routes of a shape are timed in one process from live solver handles: after a warm-up, three
runs of --steps sweeps per route, the routes alternated; the figure is the median.  One JSON line
per shape:
  ms_per_sweep      {route: median loop time / steps}; "auto" is null where the shape cannot take
                    the fused sweep (it fell back to the generic path: no "zero_fused" launch in a
                    profiled sweep)
  spread            {route: (max - min) / median of the three runs}
  speedup           ms_per_sweep["0"] / ms_per_sweep["auto"]

    python bench_zero.py [--shapes bp,bp64,hinge,hinge64,hinge_big,deadzone,logreg,logreg64,logreg_big,floor,floor64]
                         [--steps 200] [--warmup 20]

Shapes: bp = basis pursuit 1000 x 3000 and hinge = hinge + l1 1500 x 5000, the reference's sizes
(bp64 / hinge64 the same in f64); hinge_big = hinge + l1 4096 x 16384; deadzone = deadzone + l1
1500 x 5000; logreg = logistic loss + l1 1500 x 5000 (logreg64 in f64), logreg_big = the same at
4096 x 16384; floor = hinge + l1 256 x 601, the smallest row count the route takes (floor64 in f64).

--path K1,K2,...: instead, a K-member lambda path (basis pursuit: K right-hand sides on one matrix)
through _solve.solve_batch, --steps sweeps with abs_tol = rel_tol = 0, per shape and K.  The members
share the data matrix, so they run as one batched group.  One JSON line per
(shape, K):
  ms_per_sweep      median over --runs calls of the batch's loop time / steps (all K members advance
                    one sweep); spread = (max - min) / median
  tags              launches per sweep of the batched kernels in a profiled call ({} where the
                    members were solved one by one)
--lib PATH loads another build of the library (say the parent commit's, built in a second checkout)
in place of this tree's: the same inputs through its solve_batch.
--against PATH runs this tree's library and the one at PATH in child processes of one job, the two
alternated --rounds times (each child: one warm-up call and --runs timed calls per cell), and prints
per (shape, K) the median over the rounds and the spread of either side, the speedup, and whether
the batched side wins by more than the two spreads combined (ZERO paragraph).

    python bench_zero.py --path 2,4,8 [--shapes hinge,logreg,bp,hinge_big,floor] [--steps 100]
                         [--runs 3] [--lib PATH | --against PATH [--rounds 3]]

Tall cells (more rows than columns; DESIGN.md 3.11 "Tall C"): the same measurement on the two
routes of the option "fused_zero_tall" - "0" the generic operator path, which is what these
problems took before the route existed, and "1" the fused sweep over a transposed copy of the data
matrix - with the routes under those names in ms_per_sweep / spread and sweeps_per_s beside them:
hinge_tall = hinge + l1 5000 x 1500 (hinge_tall64 in f64), hinge_tall_big = 16384 x 4096,
deadzone_tall = deadzone + l1 5000 x 1500, mnist_shape = hinge + l1 60000 x 784, and the ladder
ladder256 / ladder512 / ladder1024 / ladder2048 = hinge + l1 4n x n, which sets the floor of "auto":
the smallest n from which the fused median is at least 1.05 x the generic one.

    python bench_zero.py --shapes hinge_tall,hinge_tall64,hinge_tall_big,deadzone_tall,mnist_shape,ladder256,ladder512,ladder1024,ladder2048

Tall logistic cells (a smooth z term on the tall route: five launches per sweep, DESIGN.md 3.11 "Tall
C"): the routes are those of the option "fused_zero_tall_smooth" - "0" the generic operator path,
which is what these problems took before the route existed, and "1" - with "fused_zero_tall" = "1":
logreg_tall = logistic loss + l1 5000 x 1500 (logreg_tall64 in f64), logreg_mnist_shape = 60000 x 784,
and the ladder logreg_ladder512 / logreg_ladder1024 / logreg_ladder2048 = 4n x n, which sets the floor
of that option's "auto" by the same rule.  --resident KB sets the option "fused_resident" for every
handle (default auto); the line carries it.

    python bench_zero.py --shapes logreg_tall,logreg_tall64,logreg_ladder512,logreg_ladder1024,logreg_ladder2048
    python bench_zero.py --shapes logreg_tall --resident 29297

Ridge cells (a ridge term on x in place of the l1 term: problems.hinge_l2 / svr_l2 / logreg_l2 with
their default lambda; DESIGN.md 3.11 "A ridge term on x"): the routes are those of the option
"fused_zero_ridge" - "0" the generic operator path, which is what these problems took before the
option existed, and "1" - with "fused_zero_tall" = "fused_zero_tall_smooth" = "1", so that "1" is on
wherever the routes take the shape.  Per KIND in hinge_l2, svr_l2, logreg_l2: the 4n x n ladder
KIND_ladder256 / 512 / 1024 / 2048, KIND_tall = 5000 x 1500 (KIND_tall64 in f64), and the fat cells of
hinge + l1 above, KIND_floor = 256 x 601, KIND_fat = 1500 x 5000, KIND_fat_big = 4096 x 16384.  They
set the floors of that option's "auto", one per route.  --shapes ridge is all of them.

    python bench_zero.py --shapes ridge

Free-x cells (no penalty on x, so x lives in the ZERO term alone: problems.least_abs_dev and
problems.quantile with tau = 0.3; DESIGN.md 3.11 "x in the ZERO term alone"): the routes are those of
the option "fused_zero_xfree" - "0", its default, the generic operator path, which is what these
problems took before the option existed, and "1" the fused sweep - with "fused_zero_tall" = "1".  Per
KIND in lad, quantile: the 4n x n ladder KIND_ladder256 / 512 / 1024 / 2048 and KIND_tall = 5000 x 1500
(KIND_tall64 in f64).  --shapes xfree is all of them.  With --path K1,K2,... the cells are the quantile
ones and a member count K is a tau path (tau from 0.1 to 0.9 in K steps) on one matrix under
"fused_zero_xfree" = "1": the batch as one group ("batch_zero_tall" = "1") against the same solves run
one by one ("batch_zero_tall" = "0"), the two alternated --runs times; one JSON line per (shape, K)
with ms_per_sweep, spread and tags per side and the speedup of the group.

    python bench_zero.py --shapes xfree
    python bench_zero.py --shapes xfree --path 2,4,8 [--steps 100] [--runs 3]

LP cells (a linear term on x, the non-negative cone on z: problems.lp, and the cone with an l1 or ridge
term on x: problems.polyhedron; DESIGN.md 3.11 "A linear term on x, a cone on z"): the routes are those
of the option "fused_zero_lp" - "0", its default, the generic operator path, which is what these
problems took before the option existed, and "1" the fused sweep - with "fused_zero_tall" = "1".
lp_ladder256 / 512 / 1024 / 2048 = the 4n x n ladder, lp_tall = 5000 x 1500 (lp_tall64 in f64), and the
fat cells lp_floor = 256 x 601, lp_fat = 1500 x 5000; poly_l1_tall, poly_l1_fat, poly_l2_tall,
poly_l2_fat = the polyhedron problems at 5000 x 1500 and 1500 x 5000.  --shapes lp is all of them.

    python bench_zero.py --shapes lp

--check: the residual check of the fused ZERO-term routes (DESIGN.md 3.11 "The residual check"): the
two sides are those of the option "fused_zero_check" - "0", its default, the driver's generic check,
waited for, and "1" the route's one launch with the next epoch's sweeps enqueued behind it - with
every route option on, so that each cell is on its fused sweep on both sides.  Each side runs --steps
sweeps (a multiple of 10) from a live handle with epoch_iterations at its default, 10, and
ignore_stopping_criteria set: every tenth sweep is followed by a check and no solve stops early.  The
sides are alternated --runs times in one process.  One JSON line per shape:
  ms_per_sweep        {side: median loop time / steps}, the checks included; spread as above
  speedup             ms_per_sweep["0"] / ms_per_sweep["1"]
  verdict             "win" / "loss" where the medians differ by more than the two spreads combined
                      (ZERO paragraph), else "tie"
  launches_per_check  {side: {tag: count}} of one profiled check: the profile of one sweep with its
                      check less that of a sweep without one.  The generic check's vector kernels
                      carry no profile tag, so side "0" shows none of its launches.
  time_to_optimal_s   {side: median loop time of --runs solves at the default tolerances}, with
                      stop = {side: [state, stopping sweep]}
With --path K1,K2,... the same for a K-member group (the members of --path above) through
_solve.solve_batch under "batch_zero_tall" = "1": ms_per_sweep from solves of --steps sweeps, stop a
list over the members.

    python bench_zero.py --check --shapes hinge_tall,hinge_tall64,logreg_tall,lad_tall,hinge,logreg,bp,ladder256,floor
    python bench_zero.py --check --shapes hinge_tall --path 2,8
"""

import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

from epsilon_amd import _solve, ir, problems, wire

SHAPES = {
    "bp": ("basis_pursuit", 1000, 3000, "f32"),
    "bp64": ("basis_pursuit", 1000, 3000, "f64"),
    "hinge": ("hinge_l1", 1500, 5000, "f32"),
    "hinge64": ("hinge_l1", 1500, 5000, "f64"),
    "hinge_big": ("hinge_l1", 4096, 16384, "f32"),
    "deadzone": ("deadzone_l1", 1500, 5000, "f32"),
    "logreg": ("logreg_l1", 1500, 5000, "f32"),
    "logreg64": ("logreg_l1", 1500, 5000, "f64"),
    "logreg_big": ("logreg_l1", 4096, 16384, "f32"),
    "floor": ("hinge_l1", 256, 601, "f32"),
    "floor64": ("hinge_l1", 256, 601, "f64"),
    "hinge_tall": ("hinge_l1", 5000, 1500, "f32"),
    "hinge_tall64": ("hinge_l1", 5000, 1500, "f64"),
    "hinge_tall_big": ("hinge_l1", 16384, 4096, "f32"),
    "deadzone_tall": ("deadzone_l1", 5000, 1500, "f32"),
    "mnist_shape": ("hinge_l1", 60000, 784, "f32"),
    "ladder256": ("hinge_l1", 1024, 256, "f32"),
    "ladder512": ("hinge_l1", 2048, 512, "f32"),
    "ladder1024": ("hinge_l1", 4096, 1024, "f32"),
    "ladder2048": ("hinge_l1", 8192, 2048, "f32"),
    "logreg_tall": ("logreg_l1", 5000, 1500, "f32"),
    "logreg_tall64": ("logreg_l1", 5000, 1500, "f64"),
    "logreg_ladder512": ("logreg_l1", 2048, 512, "f32"),
    "logreg_ladder1024": ("logreg_l1", 4096, 1024, "f32"),
    "logreg_ladder2048": ("logreg_l1", 8192, 2048, "f32"),
    "logreg_mnist_shape": ("logreg_l1", 60000, 784, "f32"),
}
RIDGE_KINDS = ("hinge_l2", "svr_l2", "logreg_l2")
RIDGE_CELLS = (("ladder256", 1024, 256, "f32"), ("ladder512", 2048, 512, "f32"), ("ladder1024", 4096, 1024, "f32"),
               ("ladder2048", 8192, 2048, "f32"), ("tall", 5000, 1500, "f32"), ("tall64", 5000, 1500, "f64"),
               ("floor", 256, 601, "f32"), ("fat", 1500, 5000, "f32"), ("fat_big", 4096, 16384, "f32"))
for _kind in RIDGE_KINDS:
    for _cell, _m, _n, _dtype in RIDGE_CELLS:
        SHAPES["%s_%s" % (_kind, _cell)] = (_kind, _m, _n, _dtype)
XFREE_KINDS = {"lad": "least_abs_dev", "quantile": "quantile"}
XFREE_CELLS = RIDGE_CELLS[:6]  # the ladder and the two 5000 x 1500 cells: no fat ones (C^T C is singular there)
for _name, _kind in XFREE_KINDS.items():
    for _cell, _m, _n, _dtype in XFREE_CELLS:
        SHAPES["%s_%s" % (_name, _cell)] = (_kind, _m, _n, _dtype)
LP_KINDS = {"lp": problems.lp, "poly_l1": lambda m, n: problems.polyhedron(m, n, norm="l1"),
            "poly_l2": lambda m, n: problems.polyhedron(m, n, norm="l2")}
LP_CELLS = RIDGE_CELLS[:8]  # the ladder, the two 5000 x 1500 cells, and the fat cells 256 x 601 and 1500 x 5000
LP_NAMES = ["lp_%s" % c[0] for c in LP_CELLS] + ["%s_%s" % (k, c) for k in ("poly_l1", "poly_l2") for c in ("tall", "fat")]
for _name in LP_NAMES:
    _kind, _cell = _name.rsplit("_", 1)
    SHAPES[_name] = (_kind,) + [c[1:] for c in RIDGE_CELLS if c[0] == _cell][0]
ROUTES = ("0", "auto")
TALL_ROUTES = ("0", "1")  # of "fused_zero_tall", for the cells with more rows than columns


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="bp,bp64,hinge,hinge64,hinge_big,deadzone,logreg,logreg64")
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--path", default="", help="member counts of a batched lambda path, e.g. 2,4,8")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--lib", default="")
    p.add_argument("--against", default="")
    p.add_argument("--resident", default="auto", help="the option fused_resident: auto or a number of KiB")
    p.add_argument("--check", action="store_true", help="the sides of the option fused_zero_check")
    return p.parse_args()


PATH_FRACS = (0.5, 0.35, 0.25, 0.18, 0.13, 0.09, 0.065, 0.045)  # of the generators' lambda scale


def path_members(kind, m, n, K):
    """K members on one data matrix (seed 0): lambda falls along PATH_FRACS; basis pursuit has no
    lambda and takes K right-hand sides"""
    if kind == "basis_pursuit":
        A = problems.basis_pursuit(m, n)[1]["A"]
        rng = np.random.RandomState(1)
        return [problems.basis_pursuit(m, n, b=A.dot(rng.randn(n) * (rng.rand(n) < 0.2)))[0] for _ in range(K)]
    if kind == "deadzone_l1":
        return [problems.deadzone_l1(m, n, frac=f)[0] for f in PATH_FRACS[:K]]
    C = getattr(problems, kind)(m, n)[1]["C"]
    if kind == "hinge_l1":  # problems.hinge_l1's terms on its C, without drawing the matrix again per member
        scale = np.abs(C.sum(axis=0)).max()

        def terms(lam):
            return lambda x, z: [
                ir.prox(wire.ProxFunction.SUM_HINGE,
                        ir.add(ir.linear_map(ir.scalar(-1, m), z), ir.scalar_constant(1.0, (m, 1)))),
                ir.prox(wire.ProxFunction.NORM_1, x, alpha=lam)]
        return [problems._graph_form(terms(f * scale), C, None) for f in PATH_FRACS[:K]]
    scale = np.abs(C.T.dot(np.full(m, 0.5))).max()
    return [getattr(problems, kind)(m, n, lam=f * scale)[0] for f in PATH_FRACS[:K]]


def path_lines(a):
    """the --path cells of this process's library"""
    ks = sorted(int(k) for k in a.path.split(","))
    assert 2 <= ks[0] and ks[-1] <= len(PATH_FRACS), "--path takes member counts from 2 to %d" % len(PATH_FRACS)
    sb = wire.SolverParams(max_iterations=a.steps, abs_tol=0.0, rel_tol=0.0).SerializeToString()
    short = wire.SolverParams(max_iterations=10, abs_tol=0.0, rel_tol=0.0).SerializeToString()
    for name in a.shapes.split(","):
        kind, m, n, dtype = SHAPES[name]
        probs = path_members(kind, m, n, ks[-1])
        data = {}
        for p in probs:
            data.update(p.expression_data())
        pbs = [p.SerializeToString() for p in probs]
        _solve.set_option("dtype", dtype)
        try:
            for K in ks:
                _solve.profile_reset()
                _solve.profile_enable(True)
                try:
                    _solve.solve_batch(pbs[:K], None, short, data)  # warm-up, and the launch counts
                    tags = {}
                    for t, (c, _) in _solve.profile_dump().items():
                        if t.startswith("batch_"):
                            tags[t.split(":")[0]] = tags.get(t.split(":")[0], 0) + c / 10.0
                finally:
                    _solve.profile_enable(False)
                times = []
                for _ in range(a.runs):
                    res = _solve.solve_batch(pbs[:K], None, sb, data)
                    sts = [wire.SolverStatus.FromString(st) for st, _ in res]
                    assert all(s.num_iterations == a.steps for s in sts)
                    # a group's members all carry the group's loop time; members solved one by one
                    # carry their own
                    loops = [s.timing.total_time - s.timing.init_time for s in sts]
                    times.append((loops[0] if tags else sum(loops)) / a.steps)
                med = statistics.median(times)
                yield dict(bench="zero_path", shape=name, problem=kind, m=m, n=n, dtype=dtype, gpus=1, K=K,
                           steps=a.steps, runs=a.runs, ms_per_sweep=1e3 * med,
                           spread=(max(times) - min(times)) / med, tags=tags)
        finally:
            _solve.set_option("dtype", "f32")


def xfree_path_lines(a, names):
    """the --path cells of the free-x group: a tau path as one group against its members one by one"""
    ks = sorted(int(k) for k in a.path.split(","))
    assert 2 <= ks[0], "--path takes member counts from 2"
    sb = wire.SolverParams(max_iterations=a.steps, abs_tol=0.0, rel_tol=0.0).SerializeToString()
    short = wire.SolverParams(max_iterations=10, abs_tol=0.0, rel_tol=0.0).SerializeToString()
    sides = (("group", "1"), ("one_by_one", "0"))  # of "batch_zero_tall"
    for name in names:
        kind, m, n, dtype = SHAPES[name]
        if kind != "quantile":
            continue  # (least absolute deviations has no parameter to make a path of)
        _solve.set_option("dtype", dtype)
        _solve.set_option("fused_zero_tall", "1")
        _solve.set_option("fused_zero_xfree", "1")
        try:
            for K in ks:
                probs = [problems.quantile(m, n, tau=float(t))[0] for t in np.linspace(0.1, 0.9, K)]
                data = {}
                for p in probs:
                    data.update(p.expression_data())
                pbs = [p.SerializeToString() for p in probs]
                tags, times = {}, {side: [] for side, _ in sides}
                for side, word in sides:  # warm-up, and the launches per sweep
                    _solve.set_option("batch_zero_tall", word)
                    _solve.profile_reset()
                    _solve.profile_enable(True)
                    try:
                        _solve.solve_batch(pbs, None, short, data)
                        tags[side] = {}
                        for t, (c, _) in _solve.profile_dump().items():
                            if t.startswith(("batch_zero", "zero_tall")):
                                tags[side][t.split(":")[0]] = tags[side].get(t.split(":")[0], 0) + c / 10.0
                    finally:
                        _solve.profile_enable(False)
                assert "batch_zero_tall_free_cols" in tags["group"] and "zero_tall_free_cols" in tags["one_by_one"], tags
                for _ in range(a.runs):
                    for side, word in sides:
                        _solve.set_option("batch_zero_tall", word)
                        res = _solve.solve_batch(pbs, None, sb, data)
                        sts = [wire.SolverStatus.FromString(st) for st, _ in res]
                        assert all(s.num_iterations == a.steps for s in sts)
                        # a group's members all carry the group's loop time; members solved one by
                        # one carry their own
                        loops = [s.timing.total_time - s.timing.init_time for s in sts]
                        times[side].append((loops[0] if side == "group" else sum(loops)) / a.steps)
                med = {side: statistics.median(v) for side, v in times.items()}
                yield dict(bench="zero_xfree_path", shape=name, problem=kind, m=m, n=n, dtype=dtype, gpus=1, K=K,
                           steps=a.steps, runs=a.runs, ms_per_sweep={side: 1e3 * v for side, v in med.items()},
                           spread={side: (max(v) - min(v)) / med[side] for side, v in times.items()},
                           speedup=med["one_by_one"] / med["group"], tags=tags)
        finally:
            _solve.set_option("batch_zero_tall", "0")
            _solve.set_option("fused_zero_xfree", "0")
            _solve.set_option("fused_zero_tall", "auto")
            _solve.set_option("dtype", "f32")


def path_against(a):
    """this tree's library and --against, alternated in child processes"""
    cells = {}
    for r in range(a.rounds):
        for side, lib in (("this", ""), ("base", a.against)):
            print("round %d of %d, %s" % (r + 1, a.rounds, side), file=sys.stderr, flush=True)
            cmd = [sys.executable, os.path.abspath(__file__), "--path", a.path, "--shapes", a.shapes, "--steps",
                   str(a.steps), "--runs", str(a.runs)] + (["--lib", lib] if lib else [])
            out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
            for line in out.splitlines():
                d = json.loads(line)
                cells.setdefault((d["shape"], d["K"]), {"this": [], "base": [], "meta": d})[side].append(d["ms_per_sweep"])
    for (shape, K), c in cells.items():
        med = {s: statistics.median(c[s]) for s in ("this", "base")}
        spread = {s: (max(c[s]) - min(c[s])) / med[s] for s in ("this", "base")}
        d = c["meta"]
        print(json.dumps(dict(
            bench="zero_path_vs_base", shape=shape, problem=d["problem"], m=d["m"], n=d["n"], dtype=d["dtype"],
            gpus=1, K=K, steps=a.steps, rounds=a.rounds, runs=a.runs, ms_per_sweep=med, spread=spread,
            speedup=med["base"] / med["this"],
            wins=med["base"] - med["this"] > spread["this"] * med["this"] + spread["base"] * med["base"])),
            flush=True)


CHECK_SIDES = ("0", "1")  # of "fused_zero_check"
CHECK_ROUTES_ON = (("fused_zero_tall", "1", "auto"), ("fused_zero_tall_smooth", "1", "auto"),
                   ("fused_zero_ridge", "1", "auto"), ("fused_zero_xfree", "1", "0"))  # (option, on, default)


def profiled_counts(fn):
    """{tag without its shape: launches} of fn()"""
    _solve.profile_reset()
    _solve.profile_enable(True)
    try:
        fn()
        out = {}
        for t, (c, _) in _solve.profile_dump().items():
            out[t.split(":")[0]] = out.get(t.split(":")[0], 0) + c
        return out
    finally:
        _solve.profile_enable(False)


def less(a, b, times=1):
    """{tag: a[tag] - b[tag] / times} where that is not zero"""
    out = {t: a.get(t, 0) - b.get(t, 0) / float(times) for t in set(a) | set(b)}
    return {t: v for t, v in sorted(out.items()) if v != 0}


def check_line(a, name, side_times, **more):
    kind, m, n, dtype = SHAPES[name]
    med = {side: statistics.median(v) for side, v in side_times.items()}
    spread = {side: (max(v) - min(v)) / med[side] for side, v in side_times.items()}
    gap, room = med["0"] - med["1"], spread["0"] * med["0"] + spread["1"] * med["1"]
    return dict(bench="zero_check", shape=name, problem=kind, m=m, n=n, dtype=dtype, gpus=1, steps=a.steps,
                warmup=a.warmup, runs=a.runs, epoch_iterations=10,
                ms_per_sweep={side: 1e3 * v for side, v in med.items()}, spread=spread, speedup=med["0"] / med["1"],
                verdict="win" if gap > room else "loss" if -gap > room else "tie", **more)


def check_lines(a, names):
    """the --check cells: single solves, or with --path groups"""
    assert a.steps % 10 == 0 and a.warmup % 10 == 0, "--check takes --steps and --warmup in whole epochs"
    ks = sorted(int(k) for k in a.path.split(",")) if a.path else [0]
    loop = lambda st: st.timing.total_time - st.timing.init_time
    for name in names:
        kind, m, n, dtype = SHAPES[name]
        _solve.set_option("dtype", dtype)
        for option, on, _ in CHECK_ROUTES_ON:
            _solve.set_option(option, on)
        _solve.set_option("batch_zero_tall", "1")
        try:
            for K in ks:
                line = check_group(a, name, K, loop) if K else check_single(a, name, loop)
                print(json.dumps(line), flush=True)
        finally:
            _solve.set_option("fused_zero_check", "0")
            _solve.set_option("batch_zero_tall", "0")
            for option, _, default in CHECK_ROUTES_ON:
                _solve.set_option(option, default)
            _solve.set_option("dtype", "f32")


def check_single(a, name, loop):
    kind, m, n, dtype = SHAPES[name]
    prob = getattr(problems, kind)(m, n)[0]
    pb, data = prob.SerializeToString(), prob.expression_data()
    sb = wire.SolverParams(max_iterations=10 ** 9, ignore_stopping_criteria=True).SerializeToString()
    default = wire.SolverParams().SerializeToString()
    handles, launches = {}, {}
    try:
        for side in CHECK_SIDES:
            _solve.set_option("fused_zero_check", side)  # read at Init
            s = handles[side] = _solve.Solver(pb, sb, data)
            s.init()
            s.run(a.warmup)
            with_check = profiled_counts(lambda: s.run(1))  # sweep `warmup`, a multiple of the epoch
            nine = profiled_counts(lambda: s.run(9))
            assert any(t.startswith("zero_") for t in nine), (name, sorted(nine))  # on its fused sweep
            launches[side] = less(with_check, nine, 9)
        times = {side: [] for side in CHECK_SIDES}
        for _ in range(a.runs):
            for side, s in handles.items():
                before = s.timing()[1]
                s.run(a.steps)
                times[side].append((s.timing()[1] - before) / a.steps)
    finally:
        for s in handles.values():
            s.close()
    optimal, stop = {side: [] for side in CHECK_SIDES}, {}
    for r in range(a.runs + 1):  # (the first round: a warm-up)
        for side in CHECK_SIDES:
            _solve.set_option("fused_zero_check", side)
            st = wire.SolverStatus.FromString(_solve.solve(pb, [], default, data)[0])
            stop[side] = [st.state, st.num_iterations]
            if r > 0:
                optimal[side].append(loop(st))
    return check_line(a, name, times, launches_per_check=launches,
                      time_to_optimal_s={side: statistics.median(v) for side, v in optimal.items()}, stop=stop)


def check_group(a, name, K, loop):
    kind, m, n, dtype = SHAPES[name]
    probs = path_members(kind, m, n, K)
    data = {}
    for p in probs:
        data.update(p.expression_data())
    pbs = [p.SerializeToString() for p in probs]
    fixed = lambda sweeps: wire.SolverParams(max_iterations=sweeps, ignore_stopping_criteria=True).SerializeToString()
    default = wire.SolverParams().SerializeToString()
    launches = {}
    for side in CHECK_SIDES:
        _solve.set_option("fused_zero_check", side)
        # 20, 21 and 30 sweeps have 3, 4 and 4 checks: 21 less 20 is a sweep and a check, 30 less 21 nine sweeps
        _solve.solve_batch(pbs, None, fixed(20), data)
        c20, c21, c30 = (profiled_counts(lambda k=k: _solve.solve_batch(pbs, None, fixed(k), data)) for k in (20, 21, 30))
        assert any(t.startswith("batch_zero") for t in c20), (name, K, sorted(c20))  # one group
        launches[side] = less(less(c21, c20), less(c30, c21), 9)
    times = {side: [] for side in CHECK_SIDES}
    optimal, stop = {side: [] for side in CHECK_SIDES}, {}
    for r in range(a.runs):
        for side in CHECK_SIDES:
            _solve.set_option("fused_zero_check", side)
            sts = [wire.SolverStatus.FromString(st) for st, _ in _solve.solve_batch(pbs, None, fixed(a.steps), data)]
            assert all(s.num_iterations == a.steps for s in sts)
            times[side].append(loop(sts[0]) / a.steps)  # (a group's members all carry the group's loop time)
            sts = [wire.SolverStatus.FromString(st) for st, _ in _solve.solve_batch(pbs, None, default, data)]
            optimal[side].append(loop(sts[0]))
            stop[side] = [[s.state, s.num_iterations] for s in sts]
    return check_line(a, name, times, K=K, launches_per_check=launches,
                      time_to_optimal_s={side: statistics.median(v) for side, v in optimal.items()}, stop=stop)


def names_of_one_sweep(s):
    _solve.profile_reset()
    _solve.profile_enable(True)
    try:
        s.run(1)
        return {t.split(":")[0] for t in _solve.profile_dump()}
    finally:
        _solve.profile_enable(False)


def main():
    a = parse()
    if a.lib:
        _solve.LIB_PATH = os.path.abspath(a.lib)  # (before the first call loads the library)
    names = a.shapes.split(",")
    if "xfree" in names:
        at = names.index("xfree")
        names[at:at + 1] = ["%s_%s" % (k, c[0]) for k in XFREE_KINDS for c in XFREE_CELLS]
    if a.check:
        return check_lines(a, names)
    if a.path and all(SHAPES[name][0] in XFREE_KINDS.values() for name in names):
        for line in xfree_path_lines(a, names):
            print(json.dumps(line), flush=True)
        return
    if a.path:
        if a.against:
            return path_against(a)
        for line in path_lines(a):
            print(json.dumps(line), flush=True)
        return
    if "ridge" in names:
        at = names.index("ridge")
        names[at:at + 1] = ["%s_%s" % (k, c[0]) for k in RIDGE_KINDS for c in RIDGE_CELLS]
    if "lp" in names:
        at = names.index("lp")
        names[at:at + 1] = LP_NAMES
    for name in names:
        kind, m, n, dtype = SHAPES[name]
        tall = m > n
        ridge = kind in RIDGE_KINDS
        xfree = kind in XFREE_KINDS.values()
        lp = kind in LP_KINDS
        option, routes, tag = (("fused_zero_tall_smooth", TALL_ROUTES, "zero_tall_samples")
                               if tall and kind.startswith("logreg") else
                               ("fused_zero_tall", TALL_ROUTES, "zero_tall") if tall else
                               ("fused_zero", ROUTES, "zero_fused"))
        if ridge:  # the same tags show the route; the option that is switched is the ridge term's
            option, routes = "fused_zero_ridge", TALL_ROUTES
        if xfree:  # the x side's own launch shows the route
            option, routes, tag = "fused_zero_xfree", TALL_ROUTES, "zero_tall_free_cols"
        if lp:  # the same tags show the route; the option that is switched is the two heads'
            option, routes = "fused_zero_lp", TALL_ROUTES
        prob = (LP_KINDS[kind] if lp else getattr(problems, kind))(m, n)[0]
        pb, data = prob.SerializeToString(), prob.expression_data()
        sb = wire.SolverParams(max_iterations=10 ** 9, ignore_stopping_criteria=True).SerializeToString()
        _solve.set_option("dtype", dtype)
        _solve.set_option("fused_resident", a.resident)
        if option == "fused_zero_tall_smooth" or ridge or xfree or lp:
            _solve.set_option("fused_zero_tall", "1")
        if ridge:
            _solve.set_option("fused_zero_tall_smooth", "1")
        handles = {}
        try:
            for route in routes:
                _solve.set_option(option, route)  # read at Init
                s = _solve.Solver(pb, sb, data)
                s.init()
                s.run(a.warmup)
                fused = tag in names_of_one_sweep(s)
                assert not (route == "0" and fused)
                if route != "0" and not fused:
                    s.close()  # fell back: the generic path again
                else:
                    handles[route] = s
            times = {r: [] for r in handles}
            for _ in range(3):
                for r, s in handles.items():
                    before = s.timing()[1]
                    s.run(a.steps)
                    times[r].append((s.timing()[1] - before) / a.steps)
        finally:
            for s in handles.values():
                s.close()
            _solve.set_option(option, "0" if xfree or lp else "auto")
            _solve.set_option("fused_zero_tall", "auto")
            _solve.set_option("fused_zero_tall_smooth", "auto")
            _solve.set_option("fused_resident", "auto")
            _solve.set_option("dtype", "f32")
        ms = {r: (1e3 * statistics.median(times[r]) if r in times else None) for r in routes}
        spread = {r: ((max(times[r]) - min(times[r])) / statistics.median(times[r]) if r in times else None)
                  for r in routes}
        line = dict(bench="zero_routes", shape=name, problem=kind, m=m, n=n, dtype=dtype, gpus=1, steps=a.steps,
                    warmup=a.warmup, ms_per_sweep=ms, spread=spread,
                    speedup=(ms["0"] / ms[routes[1]] if ms[routes[1]] else None))
        if a.resident != "auto":
            line["fused_resident_kb"] = int(a.resident)
        if ridge or xfree or lp:
            line["option"] = option
        if tall:
            line["sweeps_per_s"] = {r: (1e3 / ms[r] if ms[r] else None) for r in routes}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
