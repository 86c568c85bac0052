#!/usr/bin/env python3
"""bench_reads.py -- `reads` on the MI355X (csrc/mcx_reads.h: mcx_graph_reads_touch / _reads_touch_stream_dev).

Workload: the graph of tools/bench_clean.py -- the C2 shape of bench.py at k = 31, 10 M x 150 bp reads from its
200 Mbp genome, one colour, about 227 M k-mers -- and C2's reads: the first 5 M-read batch the graph was built from
(every read hits) and a batch of 5 M reads from another genome (next to none hits), as device streams.

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. kernel: for both batches, mcx_graph_reads_touch_stream_dev `--runs` times; device ms of k_rt_probe and k_rt_reads
     from the library's "profile" spans (HIP events around every launch), medians.  The k-mer counts come from one call
     of the host entry on the same reads (which is timed as well, wall clock).  From them: k-mers looked up per second
     by the probe pass, its ratio to `k_infer_records`' 5.47 G read-only lookups/s on the same graph (README), reads
     per second of the per-read pass.
  2. e2e: `mccortex31 reads -m 16G -n 512M --seq` on the graph written as a .ctx and the first 10^6 reads of the batch
     in a plain file (one read per line), wall clock (process start to exit).
One JSON line on stdout; `--out dir` also writes it to dir/reads_bench.json."""
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

INFER_LOOKUPS_PER_S = 5.47e9  # k_infer_records on this graph (README, tools/bench_inferedges.py)
E2E_READS = 1_000_000


def step_kernel(runs, ctx_path, reads_path):
    import torch
    import bench
    import bench_clean
    from oracle import ctxio
    g = bench_clean.build_graph()
    nk = g.nkmers
    if ctx_path:
        with open(ctx_path, "wb") as f:
            f.write(ctxio.header_bytes(bench_clean.K, [ctxio.GraphInfo()]))
            f.write(g.export(sorted_=False))
    n, width = bench_clean.BATCH, bench.READ_LEN + 1
    res = {"nkmers": nk, "runs": runs, "batch_reads": n}
    for what, gseed in (("own_reads", 1), ("other_genome", 2)):
        genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", gseed)
        s = bench.make_batch(genome, n, 1000, "cuda:0")
        del genome
        assert s.numel() == n * width
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * width
        hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        host = s.view(n, width)[:, :bench.READ_LEN].contiguous().cpu().numpy().reshape(-1)
        if what == "own_reads" and reads_path:
            with open(reads_path, "wb") as f:
                f.write(s[:E2E_READS * width].cpu().numpy().tobytes())
        import numpy as np
        hoff = np.arange(n + 1, dtype=np.uint64) * bench.READ_LEN
        g.reads_touch(host[:bench.READ_LEN * 1000], hoff[:1001])  # (the staging buffers are pinned by the first call)
        t0 = time.time()
        hhit, st = g.reads_touch(host, hoff)
        host_s = time.time() - t0
        g.configure("profile", 1)
        probe, reads = [], []
        for _ in range(runs):
            p0 = g.profile()
            g.reads_touch_stream_dev(s, s.numel(), off, n, hit)
            g.sync()
            p1 = g.profile()
            probe.append(p1["k_rt_probe"][1] - p0.get("k_rt_probe", (0, 0.0))[1])
            reads.append(p1["k_rt_reads"][1] - p0.get("k_rt_reads", (0, 0.0))[1])
        g.configure("profile", 0)
        assert bool((hit.cpu().numpy() == hhit).all()), "the device entry and the host entry disagree"
        pm, rm = statistics.median(probe), statistics.median(reads)
        res[what] = {"stats": st.as_dict(), "probe_ms": [round(x, 3) for x in probe], "probe_ms_median": round(pm, 3),
                     "probe_kmers_per_s": st.num_kmers / (pm * 1e-3), "probe_vs_infer_records": st.num_kmers / (pm * 1e-3) / INFER_LOOKUPS_PER_S,
                     "reads_ms": [round(x, 3) for x in reads], "reads_ms_median": round(rm, 3), "reads_per_s": n / (rm * 1e-3),
                     "host_entry_s": round(host_s, 3), "host_entry_kmers_per_s": st.num_kmers / host_s}
        del s, off, hit, host
    g.close()
    print(json.dumps(res))


def child(args, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--ctx", default=None)
    ap.add_argument("--reads", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.ctx, a.reads)
    import shutil
    tmp = tempfile.mkdtemp(prefix="bench_reads_")
    try:
        ctx, reads = os.path.join(tmp, "raw.ctx"), os.path.join(tmp, "reads.txt")
        extra = [] if a.no_e2e else ["--ctx", ctx, "--reads", reads]
        res = child(["--step", "kernel", "--runs", str(a.runs)] + extra, 500)
        if not a.no_e2e:
            t0 = time.time()
            q = subprocess.run(["timeout", "-k", "10", "400", os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "reads", "-f",
                                "-m", "16G", "-n", "512M", "--seq", "%s:%s" % (reads, os.path.join(tmp, "out")), ctx],
                               stderr=subprocess.PIPE, text=True)
            res["e2e_s"] = round(time.time() - t0, 3) if q.returncode == 0 else None
            res["e2e_reads"] = E2E_READS
            res["e2e_total_line"] = next((ln.strip() for ln in q.stderr.splitlines() if "Total printed" in ln), None)
            res["ctx_bytes"] = os.path.getsize(ctx)
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "reads_bench.json"), "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)  # (the .ctx file is GBs; also when a step failed)


if __name__ == "__main__":
    main()
