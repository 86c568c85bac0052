#!/usr/bin/env python3
"""bench_popbubbles.py -- `popbubbles` on the MI355X (csrc/mcx_pop.h: mcx_graph_pop_bubbles).

Workload: the graph of tools/bench_clean.py -- the C2 shape of bench.py at k = 31, 10 M x 150 bp reads from its
200 Mbp genome, one colour, about 227 M k-mers.

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. kernel: 5 times, on a freshly built graph each time (popping changes it): mcx_graph_unitig_stats, then
     mcx_graph_pop_bubbles.  Device ms per kernel from the library's "profile" spans; medians of the decomposition,
     the bubble phases (sums and ends, pairs, resolution with its round count) and the prune.
  2. e2e: `mccortex31 popbubbles -m 16G -n 512M -o` (the table size of step 1) on the graph written as a .ctx, wall clock (process start to exit).
One JSON line on stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = {"sums": ("k_pop_sums", "k_pop_norm"), "pairs": ("k_pop_pairs",),
          "resolution": ("k_pop_mark", "k_pop_threats", "k_pop_settle", "k_pop_apply", "k_pop_count"),
          "prune": ("k_cl_prune_edges", "k_cl_tombstone")}


def step_kernel(ctx_path, runs):
    import bench_clean
    from oracle import ctxio
    rows, st, n = [], None, 0
    for i in range(runs):
        g = bench_clean.build_graph()
        n = g.nkmers
        if ctx_path and i == 0:
            with open(ctx_path, "wb") as f:
                f.write(ctxio.header_bytes(bench_clean.K, [ctxio.GraphInfo()]))
                f.write(g.export(sorted_=False))
        g.configure("profile", 1)
        p0 = g.profile()
        g.unitig_stats()
        p1 = g.profile()
        st = g.pop_bubbles()
        p2 = g.profile()
        d = lambda a, b, name: b.get(name, (0, 0.0))[1] - a.get(name, (0, 0.0))[1]  # noqa: E731
        row = {"decomposition": sum(d(p0, p1, name) for name in p1 if name.startswith(("k_cl_", "radix_sort_keys")))}
        for phase, names in PHASES.items():
            row[phase] = sum(d(p1, p2, name) for name in names)
        rows.append(row)
        g.close()
        del g
    med = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]}
    med["bubble_phases"] = round(med["sums"] + med["pairs"] + med["resolution"], 3)
    print(json.dumps({"nkmers": n, "runs": runs, "ms_median": med, "stats": st}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--ctx", default=None)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.step == "kernel":
        step_kernel(a.ctx, a.runs)
        return
    import shutil
    tmp = tempfile.mkdtemp(prefix="bench_pop_")
    try:
        ctx = os.path.join(tmp, "raw.ctx")
        p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--ctx", ctx,
                            "--runs", str(a.runs)], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(p.returncode)
        res = json.loads(p.stdout.strip().splitlines()[-1])
        t0 = time.time()
        q = subprocess.run(["timeout", "-k", "10", "600", os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "popbubbles", "-q", "-f",
                            "-m", "16G", "-n", "512M", "-o", os.path.join(tmp, "pop.ctx"), ctx])
        res["e2e_s"] = round(time.time() - t0, 3) if q.returncode == 0 else None
        res["ctx_bytes"] = os.path.getsize(ctx)
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)  # (the .ctx files are GBs; also when a step failed)


if __name__ == "__main__":
    main()
