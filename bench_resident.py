"""Residency of the streamed lasso matrix in the Infinity Cache (DESIGN.md 3.7 "Residency", 4):
the two measurements behind `profiles/r09_resident_*.jsonl`.

    python bench_resident.py --probe OUT.jsonl
        eps_bench_stream_resident on a 2.0 GB buffer: resident sizes 0 ... 240 MiB, the four grids
        bench.py uses, three repetitions, with the bare streams (eps_bench_stream, modes 0 and 1)
        beside them.  One JSON line per launch shape.

    python bench_resident.py --sweep OUT.jsonl [--budgets 0,128,192,auto] [--rounds 3]
        `python bench.py` in a child process per value of the option "fused_resident" (MiB, or
        auto), the values alternated `rounds` times.  One JSON line per run.
"""

import argparse
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MIB = 1 << 20


def probe(path):
    import torch
    from epsilon_amd import _solve
    L = _solve.lib()
    nbytes = 10000 * 50000 * 4
    buf = torch.rand(nbytes // 4, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    ms = ctypes.c_double()
    with open(path, "w") as out:
        def emit(rec):
            rec.update(ms=ms.value, TBs=nbytes / ms.value / 1e9)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            print(rec, flush=True)
        for rep in range(3):
            for res in (0, 64, 128, 160, 192, 208, 224, 240):
                for grid in (512, 1024, 2048, 4096):
                    _solve._check(L.eps_bench_stream_resident(
                        ctypes.c_void_p(buf.data_ptr()), ctypes.c_size_t(nbytes), ctypes.c_size_t(res * MIB),
                        ctypes.c_int(grid), ctypes.c_int(20), ctypes.byref(ms)))
                    emit({"rep": rep, "resident_MiB": res, "grid": grid})
            for mode in (0, 1):
                for grid in (512, 1024, 2048, 4096):
                    _solve._check(L.eps_bench_stream(ctypes.c_void_p(buf.data_ptr()), ctypes.c_size_t(nbytes),
                                                     ctypes.c_int(mode), ctypes.c_int(grid), ctypes.c_int(20),
                                                     ctypes.byref(ms)))
                    emit({"rep": rep, "stream_mode": mode, "grid": grid})


def sweep(path, budgets, rounds):
    with open(path, "w") as out:
        for r in range(rounds):
            for b in budgets:
                env = dict(os.environ)
                env["EPSILON_HIP_FUSED_RESIDENT_KB"] = "auto" if b == "auto" else str(int(b) * 1024)
                res = subprocess.run([sys.executable, os.path.join(HERE, "bench.py")], env=env, cwd=HERE,
                                     capture_output=True, text=True, check=True)
                line = json.loads(res.stdout.strip().splitlines()[-1])
                rec = {"round": r, "fused_resident_MiB": b if b == "auto" else int(b),
                       "iter_per_s": round(line["value"], 1)}
                out.write(json.dumps(rec) + "\n")
                out.flush()
                print(rec, flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--probe", metavar="OUT")
    p.add_argument("--sweep", metavar="OUT")
    p.add_argument("--budgets", default="0,128,176,192,200,208,216,224,240,256,288,320,512,auto")
    p.add_argument("--rounds", type=int, default=3)
    a = p.parse_args()
    if not a.probe and not a.sweep:
        p.error("--probe OUT or --sweep OUT")
    if a.sweep:  # children first: this process has not touched the GPU yet
        sweep(a.sweep, a.budgets.split(","), a.rounds)
    if a.probe:
        probe(a.probe)


if __name__ == "__main__":
    main()
