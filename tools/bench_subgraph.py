#!/usr/bin/env python3
"""bench_subgraph.py -- `subgraph` on the MI355X (csrc/mcx_subgraph.h: mcx_graph_subgraph_begin / _seed_stream_dev / _finish).

Workload: the graph of tools/bench_clean.py -- the C2 shape of bench.py at k = 31, 10 M x 150 bp reads from its
200 Mbp genome, one colour, about 227 M k-mers.  Seeds: the first 10^3 and the first 10^6 of those reads, as a
device stream.

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. kernel: for every (seeds, dist) in {10^3, 10^6} x {0, 10, 1000}, `--runs` times on a freshly built graph (the
     prune changes it): begin, seeds, finish.  Device ms per kernel from the library's "profile" spans (HIP events
     around every launch); medians.  From them: seed lookups per second (k_sg_seed), ms per wide level and probes per
     second at the largest frontier (k_sg_expand; 8 probes per entry is the upper bound the figure is quoted
     against), the prune (k_sg_prune_edges + k_sg_tombstone).
  2. narrow: 10^3 seeds, dist 1000, "subgraph_narrow" 0 against 256: levels per second of the extension either way.
  3. e2e: `mccortex31 subgraph -m 16G -n 512M --dist 10 -o` on the graph written as a .ctx with 10^3 seed reads in
     a FASTA file, wall clock (process start to exit).
One JSON line on stdout; `--out dir` also writes it to dir/subgraph_bench.json."""
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

NSEEDS, DISTS = (1000, 1000000), (0, 10, 1000)
SG = ("k_sg_seed", "k_sg_grab", "k_sg_open", "k_sg_expand", "k_sg_narrow", "k_sg_prune_edges", "k_sg_tombstone", "k_cl_compact")


def one_run(nseed, dist, narrow, ctx_path=None, fa_path=None):
    """-> ({kernel: (launches, ms)}, stats) of one subgraph on a fresh graph"""
    import bench
    import bench_clean
    from oracle import ctxio
    g = bench_clean.build_graph()
    if ctx_path:
        with open(ctx_path, "wb") as f:
            f.write(ctxio.header_bytes(bench_clean.K, [ctxio.GraphInfo()]))
            f.write(g.export(sorted_=False))
    genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", 1)
    reads = bench.make_batch(genome, bench_clean.BATCH, 1000, "cuda:0")  # the first batch the graph was built from
    seeds = reads[:nseed * (bench.READ_LEN + 1)].clone()
    del reads, genome
    if fa_path:
        with open(fa_path, "wb") as f:
            f.write(seeds.cpu().numpy().tobytes())
    g.configure("subgraph_narrow", narrow)
    g.configure("profile", 1)
    p0 = g.profile()
    g.subgraph_begin()
    g.subgraph_seed_stream_dev(seeds, seeds.numel())
    st = g.subgraph_finish(dist)
    p1 = g.profile()
    prof = {name: (p1[name][0] - p0.get(name, (0, 0.0))[0], p1[name][1] - p0.get(name, (0, 0.0))[1]) for name in SG if name in p1}
    g.close()
    return prof, st


def summarise(rows, nseed):
    """medians over the runs of one configuration"""
    prof = {name: (rows[0][0][name][0], round(statistics.median(r[0][name][1] for r in rows), 4)) for name in rows[0][0]}
    st = rows[0][1]
    out = {"kernels": prof, "stats": st}
    seed_ms = prof.get("k_sg_seed", (0, 0.0))[1]
    if seed_ms > 0:
        out["seed_lookups_per_s"] = st["num_seed_kmers"] / (seed_ms * 1e-3)
    calls, ms = prof.get("k_sg_expand", (0, 0.0))
    if calls and st["levels"]:
        out["wide_ms_per_launch"] = round(ms / calls, 5)
        out["wide_probes_per_s_upper"] = 8.0 * (st["nkmers_kept"] - st["num_seed_found"]) / (ms * 1e-3) if ms > 0 else None
    out["prune_ms"] = round(prof.get("k_sg_prune_edges", (0, 0.0))[1] + prof.get("k_sg_tombstone", (0, 0.0))[1], 3)
    return out


def step_kernel(runs, ctx_path, fa_path):
    res = {}
    for nseed in NSEEDS:
        for dist in DISTS:
            first = nseed == NSEEDS[0] and dist == 10
            rows = [one_run(nseed, dist, 0, ctx_path if first and i == 0 else None, fa_path if first and i == 0 else None) for i in range(runs)]
            res["seeds%d_dist%d" % (nseed, dist)] = summarise(rows, nseed)
    print(json.dumps({"runs": runs, "configs": res}))


def step_narrow(runs):
    out = {}
    for narrow in (0, 256):
        rows = [one_run(NSEEDS[0], 1000, narrow) for _ in range(runs)]
        name = "k_sg_narrow" if narrow else "k_sg_expand"
        ms = statistics.median(r[0].get("k_sg_narrow", (0, 0.0))[1] + r[0].get("k_sg_expand", (0, 0.0))[1] for r in rows)
        st = rows[0][1]
        out["narrow%d" % narrow] = {"extension_ms": round(ms, 3), "levels": st["levels"], "narrow_launches": st["narrow_launches"],
                                    "max_frontier": st["max_frontier"], "levels_per_s": st["levels"] / (ms * 1e-3) if ms > 0 else None,
                                    "main_kernel": name}
    print(json.dumps(out))


def child(args, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel", "narrow"], default=None)
    ap.add_argument("--ctx", default=None)
    ap.add_argument("--fa", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.ctx, a.fa)
    if a.step == "narrow":
        return step_narrow(a.runs)
    import shutil
    tmp = tempfile.mkdtemp(prefix="bench_subgraph_")
    try:
        ctx, fa = os.path.join(tmp, "raw.ctx"), os.path.join(tmp, "seeds.txt")
        res = child(["--step", "kernel", "--runs", str(a.runs), "--ctx", ctx, "--fa", fa], 1100)
        res["narrow"] = child(["--step", "narrow", "--runs", str(a.runs)], 900)
        t0 = time.time()
        q = subprocess.run(["timeout", "-k", "10", "600", os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "subgraph", "-q", "-f",
                            "-m", "16G", "-n", "512M", "--seq", fa, "--dist", "10", "-o", os.path.join(tmp, "sub.ctx"), ctx])
        res["e2e_s"] = round(time.time() - t0, 3) if q.returncode == 0 else None
        res["ctx_bytes"] = os.path.getsize(ctx)
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "subgraph_bench.json"), "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)  # (the .ctx files are GBs; also when a step failed)


if __name__ == "__main__":
    main()
