#!/usr/bin/env python3
"""bench_clean.py -- `clean` on the MI355X (csrc/mcx_clean.h: mcx_graph_unitig_stats, mcx_graph_clean).

Workload: the C2 shape of bench.py at k = 31 -- 10 M x 150 bp reads (two of its 5 M-read batches) from its
200 Mbp genome -- built into a one-colour graph in HBM.

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. kernel: mcx_graph_unitig_stats 5 times (device ms per kernel from the library's "profile" spans, median),
     then mcx_graph_clean once with the picked threshold (or 2) and tips < 2k.
  2. e2e: `mccortex31 clean -o` on the graph written as a .ctx, wall clock (process start to exit).
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

K, READS, BATCH = 31, 10_000_000, 5_000_000


def build_graph():
    import bench
    import mccortex_amd as mcx
    genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", 1)
    g = mcx.Graph(K, 1, 1 << 29)
    for i in range(READS // BATCH):
        s = bench.make_batch(genome, BATCH, 1000 + i, "cuda:0")
        g.add_stream_dev(0, s, s.numel())
        del s
    g.sync()
    return g


def step_kernel(ctx_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import clean_restate as R
    from oracle import ctxio
    g = build_graph()
    n = g.nkmers
    if ctx_path:
        with open(ctx_path, "wb") as f:
            f.write(ctxio.header_bytes(K, [ctxio.GraphInfo()]))
            f.write(g.export(sorted_=False))
    g.configure("profile", 1)
    phases, totals = {}, []
    before = None
    for _ in range(5):
        p0 = g.profile()
        before = g.unitig_stats()
        p1 = g.profile()
        run = {name: p1[name][1] - p0.get(name, (0, 0.0))[1] for name in p1 if name.startswith(("k_cl_", "radix_sort_keys", "k_checksum"))}
        for name, ms in run.items():
            phases.setdefault(name, []).append(ms)
        totals.append(sum(run.values()))
    thr = R.pick_threshold([int(x) for x in before["kmer_covg"]])
    p0 = g.profile()
    st, _ = g.clean(thr if thr > 0 else 2, 2 * K)
    p1 = g.profile()
    clean_ms = {name: p1[name][1] - p0.get(name, (0, 0.0))[1] for name in p1
                if name in ("k_cl_decide", "k_cl_kmer_hist", "k_cl_prune_edges", "k_cl_tombstone", "k_checksum")}
    jumps = p1.get("k_cl_jump", (0, 0))[0] // 5 if "k_cl_jump" in p1 else 0
    print(json.dumps({"nkmers": n, "threshold": thr, "stats_ms_median": statistics.median(totals),
                      "stats_phase_ms_median": {k: round(statistics.median(v), 3) for k, v in phases.items()},
                      "jump_rounds": jumps, "clean_phase_ms": {k: round(v, 3) for k, v in clean_ms.items()},
                      "removed": st["nkmers_removed"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--ctx", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        step_kernel(a.ctx)
        return
    tmp = tempfile.mkdtemp(prefix="bench_clean_")
    ctx = os.path.join(tmp, "raw.ctx")
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--ctx", ctx],
                       stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    t0 = time.time()
    q = subprocess.run(["timeout", "-k", "10", "600", os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "clean", "-q", "-f",
                        "--fallback", "2", "-o", os.path.join(tmp, "clean.ctx"), ctx])
    res["e2e_s"] = round(time.time() - t0, 3) if q.returncode == 0 else None
    res["ctx_bytes"] = os.path.getsize(ctx)
    for f in ("raw.ctx", "clean.ctx"):
        if os.path.exists(os.path.join(tmp, f)):
            os.remove(os.path.join(tmp, f))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
