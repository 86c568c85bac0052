#!/usr/bin/env python3
"""bench_join.py -- `join` on the MI355X: the sort-and-reduce engine (mcx_join_*) against the table route.

Workload: the C2 graph of tools/bench_inferedges.py at k = 31 -- the k-mers of 10 M x 150 bp reads from bench.py's
200 Mbp genome, one colour -- written as a .ctx; three copies of it are joined into three colours.

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. make:   build the graph, write the .ctx
  2. engine: Join.add of the three copies from pinned memory + finish into a sink that drops the bytes, 1 warm-up then
             5 timed runs; per phase (upload + key extraction, sort, runs, reduce + write-out) the median of the
             library's host-clock figures (mcx_join_phases)
  3. table:  the yardstick in the same session: mcx_graph_add_records of the same three copies into a table sized for
             them + mcx_graph_export(sorted) into the same kind of sink, 1 warm-up then 5 timed runs
  4. e2e:    `mccortex31 join -o` of the three files, wall clock (process start to exit)
One JSON line on stdout; `--out dir` also writes it to dir/join_bench.json."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, NCOLS, READS, BATCH, RUNS = 31, 3, 10_000_000, 5_000_000, 5


def make_ctx(path):
    import bench
    import mccortex_amd as mcx
    from oracle import ctxio
    genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", 1)
    g = mcx.Graph(K, 1, 1 << 29)
    for i in range(READS // BATCH):
        s = bench.make_batch(genome, BATCH, 1000 + i, "cuda:0")
        g.add_stream_dev(0, s, s.numel())
        del s
    body = g.export(sorted_=False)
    g.close()
    with open(path, "wb") as f:
        f.write(ctxio.header_bytes(K, [ctxio.GraphInfo()]))
        f.write(body)
    return len(body) // 13


def pinned_records(path):
    import numpy as np
    import torch
    from oracle import ctxio
    buf = open(path, "rb").read()
    _, hs = ctxio.read_header(buf)
    t = torch.empty(len(buf) - hs, dtype=torch.uint8).pin_memory()
    t.numpy()[:] = np.frombuffer(buf, dtype=np.uint8, offset=hs)
    return t.numpy()


def engine_step(path, out):
    import mccortex_amd as mcx
    recs = pinned_records(path)
    n = recs.size // 13
    runs, written = [], None
    for it in range(RUNS + 1):
        t0 = time.perf_counter()
        j = mcx.Join(K, NCOLS)
        for c in range(NCOLS):
            j.add(recs, 1, [(0, c)])
        _, st = j.finish(keep=False)
        ph = j.phases()
        j.close()
        ph["total_ms"] = (time.perf_counter() - t0) * 1e3
        assert written is None or written == st["kmers_written"]
        written = st["kmers_written"]
        assert sum(j.chunks) == written * (8 + 5 * NCOLS)
        if it:
            runs.append(ph)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    json.dump({"records_in": NCOLS * n, "kmers_written": written, "median": med, "runs": runs,
               "records_in_per_s": NCOLS * n / (med["total_ms"] * 1e-3)}, open(out, "w"))


def table_step(path, out):
    import mccortex_amd as mcx
    from mccortex_amd import graph
    recs = pinned_records(path)
    n = recs.size // 13
    runs, nk = [], None
    got = [0]
    sink = graph.SINK_FN(lambda _ctx, _ptr, nbytes: got.__setitem__(0, got[0] + nbytes) or 0)
    for it in range(RUNS + 1):
        t0 = time.perf_counter()
        g = mcx.Graph(K, NCOLS, int(n / 0.75) + 1)
        t1 = time.perf_counter()
        for c in range(NCOLS):
            g.add_records(recs, 1, [(0, c)])
        g.sync()
        t2 = time.perf_counter()
        got[0] = 0
        graph._check(g.L.mcx_graph_export(g.h, 1, sink, None))
        t3 = time.perf_counter()
        assert nk is None or nk == g.nkmers
        nk = g.nkmers
        assert got[0] == nk * (8 + 5 * NCOLS)
        g.close()
        if it:
            runs.append({"create_ms": (t1 - t0) * 1e3, "add_records_ms": (t2 - t1) * 1e3, "export_sorted_ms": (t3 - t2) * 1e3,
                         "total_ms": (t3 - t0) * 1e3})
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    json.dump({"records_in": NCOLS * n, "kmers_written": nk, "median": med, "runs": runs,
               "records_in_per_s": NCOLS * n / (med["total_ms"] * 1e-3)}, open(out, "w"))


def run_step(name, cmd, limit, results):
    """one GPU step in a child process under timeout; False (and nothing more runs) when it fails"""
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    results[name + "_s"] = round(time.perf_counter() - t0, 3)
    results[name + "_rc"] = p.returncode
    print("%s: rc %d, %.1f s" % (name, p.returncode, results[name + "_s"]), flush=True)
    if p.returncode != 0:
        results[name + "_tail"] = p.stderr.decode(errors="replace")[-2000:]
        return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="directory that also gets the JSON line (join_bench.json)")
    ap.add_argument("--step", choices=["make", "engine", "table"], help=argparse.SUPPRESS)  # (child processes)
    ap.add_argument("--ctx")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.step == "make":
        json.dump({"records": make_ctx(a.ctx)}, open(a.json, "w"))
        return
    if a.step == "engine":
        engine_step(a.ctx, a.json)
        return
    if a.step == "table":
        table_step(a.ctx, a.json)
        return
    work = tempfile.mkdtemp(prefix="join_")
    ctx, outctx = os.path.join(work, "c2.ctx"), os.path.join(work, "pop.ctx")
    exe = os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31")
    me = [sys.executable, os.path.abspath(__file__)]
    res = {"workload": "k=31, three copies of the one-colour graph of %d M x 150 bp C2 reads (bench.py's genome and batches) "
                       "into three colours" % (READS // 1_000_000)}
    try:
        ok = run_step("make", me + ["--step", "make", "--ctx", ctx, "--json", os.path.join(work, "m.json")], 240, res)
        for step in ("engine", "table"):
            ok = ok and run_step(step, me + ["--step", step, "--ctx", ctx, "--json", os.path.join(work, step + ".json")], 400, res)
            if ok:
                res[step] = json.load(open(os.path.join(work, step + ".json")))
        e2e = []
        for _ in range(RUNS):
            ok = ok and run_step("e2e", [exe, "join", "-q", "-f", "-m", "200G", "-o", outctx, ctx, ctx, ctx], 200, res)
            if ok:
                e2e.append(res["e2e_s"])
        if ok:
            res["e2e_s_runs"], res["e2e_s_median"] = e2e, statistics.median(e2e)
            res["ctx_bytes"], res["out_bytes"] = os.path.getsize(ctx), os.path.getsize(outctx)
        res["ok"] = bool(ok)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        open(os.path.join(a.out, "join_bench.json"), "w").write(line + "\n")
    print(line)
    sys.exit(0 if res.get("ok") else 1)


if __name__ == "__main__":
    main()
