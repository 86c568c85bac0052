#!/usr/bin/env python3
"""bench_inferedges.py -- `inferedges` on the MI355X (k_infer_records, mcx_graph_infer_edges_dev).

Workload: the C2 shape of bench.py at k = 31 -- 10 M x 150 bp reads (two of its 5 M-read batches) from its
200 Mbp genome -- built into a one-colour graph; then a 3-colour graph of the same k-mers: colour 0 is that
graph, colours 1 and 2 have the same coverage and no edges (so --all looks up every neighbour of every record).

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. kernel: mcx_graph_infer_edges_dev on the records in HBM, 3 warm-ups then 5 timed runs (device events around
     the kernel: the library's "profile" spans); records/s and neighbour lookups/s from the median.
  2. e2e: `mccortex31 inferedges --all -o` on the same .ctx, wall clock (process start to exit).
  3. rocprofv3 --kernel-trace --stats of the same command (a separate run: tracing slows the host).
One JSON line on stdout; the stats files land under --out."""
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

K, NCOLS, READS, BATCH = 31, 3, 10_000_000, 5_000_000


def make_ctx(path):
    """the 3-colour .ctx of the workload; returns its record count"""
    import numpy as np
    import bench
    import mccortex_amd as mcx
    from oracle import ctxio
    genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", 1)
    g = mcx.Graph(K, 1, 1 << 29)
    for i in range(READS // BATCH):
        s = bench.make_batch(genome, BATCH, 1000 + i, "cuda:0")
        g.add_stream_dev(0, s, s.numel())
        del s
    body = np.frombuffer(g.export(sorted_=False), dtype=np.uint8).reshape(-1, 13)
    g.close()
    n = body.shape[0]
    rs = 8 + 5 * NCOLS
    recs = np.zeros((n, rs), dtype=np.uint8)
    recs[:, :8] = body[:, :8]
    for c in range(NCOLS):
        recs[:, 8 + 4 * c:12 + 4 * c] = body[:, 8:12]
    recs[:, 8 + 4 * NCOLS] = body[:, 12]
    with open(path, "wb") as f:
        f.write(ctxio.header_bytes(K, [ctxio.GraphInfo() for _ in range(NCOLS)]))
        f.write(recs.tobytes())
    return n


def expected_lookups(recs):
    """lookups the kernel makes: per record, the edges in `add` that some colour with coverage lacks"""
    import numpy as np
    cov = recs[:, 8:8 + 4 * NCOLS].copy().view("<u4").reshape(-1, NCOLS)
    ed = recs[:, 8 + 4 * NCOLS:]
    iedges = np.bitwise_and.reduce(ed, axis=1)
    add = ~iedges
    want = np.zeros(len(recs), dtype=np.uint8)
    for c in range(NCOLS):
        want |= np.where(cov[:, c] > 0, ~ed[:, c], 0).astype(np.uint8)
    want &= add
    return int(np.unpackbits(want).sum())


def kernel_step(path, out):
    import numpy as np
    import torch
    import mccortex_amd as mcx
    from oracle import ctxio
    buf = open(path, "rb").read()
    _, hs = ctxio.read_header(buf)
    recs = np.frombuffer(buf, dtype=np.uint8, offset=hs).reshape(-1, 8 + 5 * NCOLS)
    n = recs.shape[0]
    lookups = expected_lookups(recs)
    g = mcx.Graph(K, NCOLS, int(n / 0.75) + 1)
    g.add_records(recs, NCOLS, [(c, c) for c in range(NCOLS)])
    g.sync()
    d0 = torch.from_numpy(recs.reshape(-1).copy()).to("cuda:0")
    d = torch.empty_like(d0)
    g.configure("profile", 1)
    ms, wall, nmod = [], [], None
    for it in range(8):
        d.copy_(d0)
        torch.cuda.synchronize()
        before = g.profile().get("k_infer_records", (0, 0.0))[1]
        t0 = time.perf_counter()
        nm = g.infer_edges_dev(d, n)
        t1 = time.perf_counter()
        after = g.profile()["k_infer_records"][1]
        assert nmod is None or nm == nmod
        nmod = nm
        if it >= 3:
            ms.append(after - before)
            wall.append((t1 - t0) * 1e3)
    med = statistics.median(ms)
    r = {"records": n, "lookups": lookups, "nmodified": nmod, "kernel_ms_median": med, "kernel_ms_min": min(ms),
         "kernel_ms_max": max(ms), "kernel_ms_runs": ms, "call_ms_median": statistics.median(wall),
         "records_per_s": n / (med * 1e-3), "lookups_per_s": lookups / (med * 1e-3)}
    g.close()
    json.dump(r, open(out, "w"))


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
    ap.add_argument("--out", default="bench_inferedges_out", help="directory for the JSON line and the rocprofv3 stats")
    ap.add_argument("--step", choices=["make", "kernel"], help=argparse.SUPPRESS)  # (child processes)
    ap.add_argument("--ctx")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.step == "make":
        json.dump({"records": make_ctx(a.ctx)}, open(a.json, "w"))
        return
    if a.step == "kernel":
        kernel_step(a.ctx, a.json)
        return
    os.makedirs(a.out, exist_ok=True)
    work = tempfile.mkdtemp(prefix="inferedges_")
    ctx, outctx = os.path.join(work, "c2x3.ctx"), os.path.join(work, "out.ctx")
    exe = os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31")
    me = [sys.executable, os.path.abspath(__file__)]
    res = {"workload": "k=31, %d colours, the k-mers of %d M x 150 bp C2 reads (bench.py's genome and batches); "
                       "colours 1, 2: same coverage, no edges; --all" % (NCOLS, READS // 1_000_000)}
    try:
        ok = run_step("make", me + ["--step", "make", "--ctx", ctx, "--json", os.path.join(work, "m.json")], 240, res)
        ok = ok and run_step("kernel", me + ["--step", "kernel", "--ctx", ctx, "--json", os.path.join(work, "k.json")], 240, res)
        if ok:
            res["kernel"] = json.load(open(os.path.join(work, "k.json")))
        ok = ok and run_step("e2e", [exe, "inferedges", "-q", "--all", "-m", "64G", "-o", outctx, ctx], 150, res)
        if ok:
            os.remove(outctx)
            res["ctx_bytes"] = os.path.getsize(ctx)
        prof = os.path.join(a.out, "rocprof")
        ok = ok and run_step("rocprof", ["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "infer", "--",
                                         exe, "inferedges", "-q", "--all", "-m", "64G", "-o", outctx, ctx], 240, res)
        res["ok"] = bool(ok)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(res)
    open(os.path.join(a.out, "bench_inferedges.json"), "w").write(line + "\n")
    print(line)
    sys.exit(0 if res.get("ok") else 1)


if __name__ == "__main__":
    main()
