"""Matrix-variable lasso and multi-task group lasso (problems.mv_lasso / problems.group_lasso): a
fixed number of sweeps on each route of the option "fused_matrix" - "0" the generic operator path,
"pass" the batched fused pass, "wide" the wide kernels (f32) - on one GPU.

All routes of a shape are timed in one process from live solver handles: after a warm-up, three
runs of --steps sweeps per route, the routes alternated; the figure is the median.  One JSON line
per shape:
  ms_per_sweep      {route: median loop time / steps}; a route that the shape cannot take (it fell
                    back to the generic path: no batched / wide launch in a profiled sweep) is null
  speedup           {route: ms_per_sweep["0"] / ms_per_sweep[route]}
  auto              the route the default picks for this shape

    python bench_mv.py [--shapes ref,ref64,sq4,sq8,sq16,group,big8,big16] [--steps 100] [--warmup 20]

Shapes: ref = the reference's mv_lasso row (1500 x 5000, k = 10; ref64 the same in f64), sqK =
2048 x 8192 with k = K, group = group lasso 1500 x 5000 with k = 5, bigK = the config-2 matrix
(10000 x 50000) with k = K.
"""

import argparse
import json
import statistics

from epsilon_amd import _solve, problems, wire

SHAPES = {
    "ref": ("mv", 1500, 5000, 10, "f32"),
    "ref64": ("mv", 1500, 5000, 10, "f64"),
    "sq4": ("mv", 2048, 8192, 4, "f32"),
    "sq8": ("mv", 2048, 8192, 8, "f32"),
    "sq16": ("mv", 2048, 8192, 16, "f32"),
    "group": ("group", 1500, 5000, 5, "f32"),
    "big8": ("mv", 10000, 50000, 8, "f32"),
    "big16": ("mv", 10000, 50000, 16, "f32"),
}
ROUTES = ("0", "pass", "wide")
FUSED_TAGS = {"pass": "batch_fused_pass", "wide": "wide_back"}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="ref,ref64,sq4,sq8,sq16,group")
    p.add_argument("--steps", type=int, default=100)
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
        kind, m, n, k, dtype = SHAPES[name]
        prob = (problems.mv_lasso(m, n, k) if kind == "mv" else problems.group_lasso(m, n, k))[0]
        pb, data = prob.SerializeToString(), prob.expression_data()
        sb = wire.SolverParams(max_iterations=10 ** 9, ignore_stopping_criteria=True).SerializeToString()
        _solve.set_option("dtype", dtype)
        handles, taken = {}, {}
        try:
            for route in ROUTES + ("auto",):
                _solve.set_option("fused_matrix", route)  # read at Init
                s = _solve.Solver(pb, sb, data)
                s.init()
                s.run(a.warmup)
                names = names_of_one_sweep(s)
                taken[route] = [r for r, t in FUSED_TAGS.items() if t in names]
                if route == "auto" or (route in FUSED_TAGS and not taken[route]):
                    s.close()  # auto is one of the three; a route not taken is the generic path again
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
            _solve.set_option("fused_matrix", "auto")
            _solve.set_option("dtype", "f32")
        ms = {r: (1e3 * statistics.median(times[r]) if r in times else None) for r in ROUTES}
        print(json.dumps(dict(
            bench="mv_routes", shape=name, problem=kind, m=m, n=n, k=k, dtype=dtype, gpus=1, steps=a.steps,
            warmup=a.warmup, ms_per_sweep=ms,
            speedup={r: (ms["0"] / ms[r] if ms[r] else None) for r in ROUTES},
            auto=(taken["auto"] or ["0"])[0])), flush=True)


if __name__ == "__main__":
    main()
