"""Tall lasso (problems.lasso with more rows than columns): a fixed number of sweeps
on the two routes of the option "fused_tall" - "0" the generic operator path, which is what these
problems took before the route existed, and "1" the fused sweep (the tile launch of the packed
n x n inverse and the cols kernel; no pass over A) - on one GPU.

Both routes of a cell are timed in one process from live solver handles: after a warm-up, three
runs of --steps sweeps per route, the routes alternated; the figure is the median.  One JSON line
per cell:
  ms_per_sweep      {route: median loop time / steps}; "1" is null where the shape cannot take the
                    route (no "lasso_tall_cols" launch in a profiled sweep)
  spread            {route: (max - min) / median of the three runs}
  speedup           ms_per_sweep["0"] / ms_per_sweep["1"]

    python bench_tall.py [--shapes ladder256,...,ladder8192,big,ladder256_64,...,ladder4096_64]
                         [--steps 200] [--warmup 20]

Cells: ladderN = 4N x N in f32 for N = 256 ... 8192, which sets the floor of "auto" - the smallest N
from which every cell measures at least 1.05 x the generic path; ladderN_64 the same in f64 up to
4096; big = 50000 x 5000 in f32.

--path K1,K2,...: instead, a K-member lambda path on one matrix through _solve.solve_batch (the
members on the route form one group from n = 1024) against the same K members solved one by one on
the route, --steps sweeps each with abs_tol = rel_tol = 0, "fused_tall" = "1".  One JSON line per
(cell, K):
  ms_per_sweep      {"batch": ..., "singles": ...}: median over --runs of the loop time / steps for
                    all K members to advance one sweep (singles: the sum of the K solves)
  spread            (max - min) / median of either
  speedup           singles / batch
  tags              launches per sweep of the batched kernels in a profiled call

    python bench_tall.py --path 2,4,8 [--shapes ladder1024,ladder2048,big] [--steps 100] [--runs 3]
"""

import argparse
import json
import statistics

import numpy as np

from epsilon_amd import _solve, ir, problems, wire

LADDER = (256, 512, 1024, 2048, 4096, 8192)
SHAPES = {"big": (50000, 5000, "f32")}
SHAPES.update({"ladder%d" % n: (4 * n, n, "f32") for n in LADDER})
SHAPES.update({"ladder%d_64" % n: (4 * n, n, "f64") for n in LADDER if n <= 4096})
ROUTES = ("0", "1")
PATH_FRACS = (0.5, 0.35, 0.25, 0.18, 0.13, 0.09, 0.065, 0.045)  # of max|A^T b|


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default=",".join(["ladder%d" % n for n in LADDER] + ["big"] +
                                                ["ladder%d_64" % n for n in LADDER if n <= 4096]))
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--path", default="", help="member counts of a batched lambda path, e.g. 2,4,8")
    p.add_argument("--runs", type=int, default=3)
    return p.parse_args()


def names_of_one_sweep(s):
    _solve.profile_reset()
    _solve.profile_enable(True)
    try:
        s.run(1)
        return {t.split(":")[0] for t in _solve.profile_dump()}
    finally:
        _solve.profile_enable(False)


def route_line(name, a):
    m, n, dtype = SHAPES[name]
    prob = problems.lasso(m, n, seed=0)[0]
    pb, data = prob.SerializeToString(), prob.expression_data()
    sb = wire.SolverParams(max_iterations=10 ** 9, ignore_stopping_criteria=True).SerializeToString()
    _solve.set_option("dtype", dtype)
    handles = {}
    try:
        for route in ROUTES:
            _solve.set_option("fused_tall", route)  # read at Init
            s = _solve.Solver(pb, sb, data)
            s.init()
            s.run(a.warmup)
            fused = "lasso_tall_cols" in names_of_one_sweep(s)
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
        _solve.set_option("fused_tall", "auto")
        _solve.set_option("dtype", "f32")
    ms = {r: (1e3 * statistics.median(times[r]) if r in times else None) for r in ROUTES}
    spread = {r: ((max(times[r]) - min(times[r])) / statistics.median(times[r]) if r in times else None)
              for r in ROUTES}
    return dict(bench="tall_routes", shape=name, problem="lasso", m=m, n=n, dtype=dtype, gpus=1, steps=a.steps,
                warmup=a.warmup, ms_per_sweep=ms, spread=spread, speedup=(ms["0"] / ms["1"] if ms["1"] else None),
                sweeps_per_s={r: (1e3 / ms[r] if ms[r] else None) for r in ROUTES})


def path_lines(name, a):
    ks = sorted(int(k) for k in a.path.split(","))
    assert 2 <= ks[0] and ks[-1] <= len(PATH_FRACS), "--path takes member counts from 2 to %d" % len(PATH_FRACS)
    m, n, dtype = SHAPES[name]
    A, b = problems.regression_data(m, n, seed=0)
    lmax = np.abs(A.T.dot(b)).max()
    Amap, bexpr = ir.dense_matrix(A), ir.constant(b)
    probs = [problems.lasso_ir(Amap, bexpr, f * lmax, n) for f in PATH_FRACS[:ks[-1]]]
    data = {}
    for p in probs:
        data.update(p.expression_data())
    pbs = [p.SerializeToString() for p in probs]
    sb = wire.SolverParams(max_iterations=a.steps, abs_tol=0.0, rel_tol=0.0).SerializeToString()
    short = wire.SolverParams(max_iterations=10, abs_tol=0.0, rel_tol=0.0).SerializeToString()

    def loop(st):
        s = wire.SolverStatus.FromString(st)
        assert s.num_iterations == a.steps
        return s.timing.total_time - s.timing.init_time

    _solve.set_option("dtype", dtype)
    _solve.set_option("fused_tall", "1")
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
            _solve.solve(pbs[0], [], short, data)
            times = {"batch": [], "singles": []}
            for _ in range(a.runs):
                res = _solve.solve_batch(pbs[:K], None, sb, data)
                # a group's members all carry the group's loop time; members solved one by one their own
                loops = [loop(st) for st, _ in res]
                times["batch"].append((loops[0] if tags else sum(loops)) / a.steps)
                times["singles"].append(sum(loop(_solve.solve(pb, [], sb, data)[0]) for pb in pbs[:K]) / a.steps)
            med = {k: statistics.median(v) for k, v in times.items()}
            yield dict(bench="tall_path", shape=name, problem="lasso", m=m, n=n, dtype=dtype, gpus=1, K=K,
                       steps=a.steps, runs=a.runs, ms_per_sweep={k: 1e3 * v for k, v in med.items()},
                       spread={k: (max(v) - min(v)) / med[k] for k, v in times.items()},
                       speedup=med["singles"] / med["batch"], tags=tags)
    finally:
        _solve.set_option("fused_tall", "auto")
        _solve.set_option("dtype", "f32")


def main():
    a = parse()
    for name in a.shapes.split(","):
        if a.path:
            for line in path_lines(name, a):
                print(json.dumps(line), flush=True)
        else:
            print(json.dumps(route_line(name, a)), flush=True)


if __name__ == "__main__":
    main()
