#!/usr/bin/env python3
"""bench_coverage.py -- `coverage` on the MI355X (csrc/mcx_coverage.h: mcx_graph_coverage*).

Workload: that of tools/bench_reads.py -- the C2 shape of bench.py at k = 31, 10 M x 150 bp reads from its 200 Mbp
genome, about 227 M k-mers -- with one colour and with three (the same reads added to each colour), and the same two
read sets: the first 5 M-read batch the graph was built from (every k-mer is found) and a batch of 5 M reads from
another genome (next to none is), as device streams.

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. kernel (once per colour count): for both batches, mcx_graph_coverage_stream_dev `--runs` times with and without
     edges, and mcx_graph_reads_touch_stream_dev as often: device ms of k_cv_probe and of k_rt_probe from the library's
     "profile" spans, medians; k-mers looked up per second from the k-mer count of one host call.  Then the host entries
     on the first `--host-reads` reads of the batch: mcx_graph_coverage (wall clock) and mcx_graph_coverage_text with
     edges and degrees (wall clock; device ms of k_cv_len and k_cv_emit, GB/s of text written by k_cv_emit).
  2. e2e: `mccortex31 coverage -m 16G -n 512M -e -1` on the one-colour graph written as a .ctx and the first 10^5 reads
     of the batch in a plain file, output to a file, wall clock (process start to exit).
One JSON line on stdout; `--out dir` also writes it to dir/coverage_bench.json."""
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

E2E_READS = 100_000


def build_graph(ncols):
    import bench
    import bench_clean
    import mccortex_amd as mcx
    genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", 1)
    g = mcx.Graph(bench_clean.K, ncols, 1 << 29)
    for i in range(bench_clean.READS // bench_clean.BATCH):
        s = bench.make_batch(genome, bench_clean.BATCH, 1000 + i, "cuda:0")
        for c in range(ncols):
            g.add_stream_dev(c, s, s.numel())
        del s
    g.sync()
    return g


def spans(g, fn, names):
    """device ms per kernel name of one call of fn"""
    p0 = g.profile()
    fn()
    g.sync()
    p1 = g.profile()
    return {n: p1.get(n, (0, 0.0))[1] - p0.get(n, (0, 0.0))[1] for n in names}


def step_kernel(ncols, runs, host_reads, ctx_path, reads_path):
    import numpy as np
    import torch
    import bench
    import bench_clean
    from oracle import ctxio
    g = build_graph(ncols)
    if ctx_path:
        with open(ctx_path, "wb") as f:
            f.write(ctxio.header_bytes(bench_clean.K, [ctxio.GraphInfo()] * ncols))
            f.write(g.export(sorted_=False))
    n, width = bench_clean.BATCH, bench.READ_LEN + 1
    res = {"ncols": ncols, "nkmers": g.nkmers, "runs": runs, "batch_reads": n, "host_reads": host_reads}
    for what, gseed in (("own_reads", 1), ("other_genome", 2)):
        genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", gseed)
        s = bench.make_batch(genome, n, 1000, "cuda:0")
        del genome
        assert s.numel() == n * width
        pitch = (s.numel() + 63) // 64 * 64
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * width
        hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        cv = torch.empty((ncols, pitch), dtype=torch.int32, device="cuda:0")
        ed = torch.empty((ncols, pitch), dtype=torch.uint8, device="cuda:0")
        host_all = s.view(n, width)[:, :bench.READ_LEN].contiguous().cpu().numpy().reshape(-1)
        host = host_all[:host_reads * bench.READ_LEN]
        hoff = np.arange(n + 1, dtype=np.uint64) * bench.READ_LEN
        if what == "own_reads" and reads_path:
            with open(reads_path, "wb") as f:
                f.write(s[:E2E_READS * width].cpu().numpy().tobytes())
        g.reads_touch(host[:bench.READ_LEN * 1000], hoff[:1001])  # (the staging buffers are pinned by the first call)
        kmers = int(g.reads_touch(host_all, hoff)[1].num_kmers)  # k-mer occurrences of the batch
        del host_all
        hoff = hoff[:host_reads + 1]
        g.configure("profile", 1)
        t = {"k_cv_probe_edges": [], "k_cv_probe": [], "k_rt_probe": []}
        for _ in range(runs):
            t["k_cv_probe_edges"].append(spans(g, lambda: g.coverage_stream_dev(s, s.numel(), cv, ed, pitch), ["k_cv_probe"])["k_cv_probe"])
            t["k_cv_probe"].append(spans(g, lambda: g.coverage_stream_dev(s, s.numel(), cv, None, pitch), ["k_cv_probe"])["k_cv_probe"])
            t["k_rt_probe"].append(spans(g, lambda: g.reads_touch_stream_dev(s, s.numel(), off, n, hit), ["k_rt_probe"])["k_rt_probe"])
        r = {"stream_kmers": kmers}
        for name, ms in t.items():
            m = statistics.median(ms)
            r[name] = {"ms": [round(x, 3) for x in ms], "ms_median": round(m, 3), "kmers_per_s": kmers / (m * 1e-3)}
        # the host entries
        t0 = time.time()
        hcv, hed, st = g.coverage(host, hoff, edges=True)
        r["host_arrays_s"] = round(time.time() - t0, 3)
        assert bool((hcv[0, :bench.READ_LEN] == cv[0, :bench.READ_LEN].cpu().numpy().view(np.uint32)).all())
        box = {}

        def text_call():
            t1 = time.time()
            box["text"], box["loff"], _ = g.coverage_text(host, hoff, edges=True, degrees=True)
            box["s"] = time.time() - t1
        sp = spans(g, text_call, ["k_cv_len", "k_cv_emit", "k_cv_probe", "k_cv_place"])
        r["host_text_s"] = round(box["s"], 3)
        r["text_bytes"] = len(box["text"])
        r["text_ms"] = {k: round(v, 3) for k, v in sp.items()}
        r["emit_GBps"] = len(box["text"]) / (sp["k_cv_emit"] * 1e-3) / 1e9 if sp["k_cv_emit"] else None
        r["host_stats"] = st.as_dict()
        g.configure("profile", 0)
        res[what] = r
        del s, off, hit, cv, ed, host, box
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
    ap.add_argument("--ncols", type=int, default=1)
    ap.add_argument("--ctx", default=None)
    ap.add_argument("--reads", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=500_000)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.ncols, a.runs, a.host_reads, a.ctx, a.reads)
    import shutil
    tmp = tempfile.mkdtemp(prefix="bench_coverage_")
    try:
        ctx, reads = os.path.join(tmp, "raw.ctx"), os.path.join(tmp, "reads.txt")
        common = ["--step", "kernel", "--runs", str(a.runs), "--host-reads", str(a.host_reads)]
        res = {"one_colour": child(common + ["--ncols", "1"] + ([] if a.no_e2e else ["--ctx", ctx, "--reads", reads]), 500)}
        res["three_colours"] = child(common + ["--ncols", "3"], 500)
        if not a.no_e2e:
            t0 = time.time()
            q = subprocess.run(["timeout", "-k", "10", "400", os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "coverage", "-f",
                                "-m", "16G", "-n", "512M", "-e", "-o", os.path.join(tmp, "out.txt"), "-1", reads, ctx],
                               stderr=subprocess.PIPE, text=True)
            res["e2e_s"] = round(time.time() - t0, 3) if q.returncode == 0 else None
            res["e2e_reads"] = E2E_READS
            res["e2e_line"] = next((ln.strip() for ln in q.stderr.splitlines() if "Printed graph coverage" in ln), None)
            res["e2e_out_bytes"] = os.path.getsize(os.path.join(tmp, "out.txt")) if q.returncode == 0 else None
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "coverage_bench.json"), "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)  # (the .ctx file is GBs; also when a step failed)


if __name__ == "__main__":
    main()
