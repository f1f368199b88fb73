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
"""

import argparse
import json
import statistics

from epsilon_amd import _solve, problems, wire

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
}
ROUTES = ("0", "auto")


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="bp,bp64,hinge,hinge64,hinge_big,deadzone,logreg,logreg64")
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    return p.parse_args()


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
    for name in a.shapes.split(","):
        kind, m, n, dtype = SHAPES[name]
        prob = getattr(problems, kind)(m, n)[0]
        pb, data = prob.SerializeToString(), prob.expression_data()
        sb = wire.SolverParams(max_iterations=10 ** 9, ignore_stopping_criteria=True).SerializeToString()
        _solve.set_option("dtype", dtype)
        handles = {}
        try:
            for route in ROUTES:
                _solve.set_option("fused_zero", route)  # read at Init
                s = _solve.Solver(pb, sb, data)
                s.init()
                s.run(a.warmup)
                fused = "zero_fused" in names_of_one_sweep(s)
                assert not (route == "0" and fused)
                if route == "auto" and not fused:
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
            _solve.set_option("fused_zero", "auto")
            _solve.set_option("dtype", "f32")
        ms = {r: (1e3 * statistics.median(times[r]) if r in times else None) for r in ROUTES}
        spread = {r: ((max(times[r]) - min(times[r])) / statistics.median(times[r]) if r in times else None)
                  for r in ROUTES}
        print(json.dumps(dict(
            bench="zero_routes", shape=name, problem=kind, m=m, n=n, dtype=dtype, gpus=1, steps=a.steps,
            warmup=a.warmup, ms_per_sweep=ms, spread=spread,
            speedup=(ms["0"] / ms["auto"] if ms["auto"] else None))), flush=True)


if __name__ == "__main__":
    main()
