#!/usr/bin/env python3
"""bench_correct.py -- `correct` on the MI355X (csrc/mcx_correct.h: mcx_graph_correct*).

Workload: the C2 graph of tools/bench_reads.py (bench.py's shape at k = 31, 10 M x 150 bp reads from its 200 Mbp
genome, about 227 M k-mers, one colour) and the first 5 M-read batch it was built from with 1 % of the bases
substituted, as a device stream.

One child process under `timeout -k 10`:
  mcx_graph_correct_stream_dev `--runs` times (one-way; `--two-way` for the other mode) and
  mcx_graph_reads_touch_stream_dev as often on the same batch in the same session: device ms of k_cr_probe, the two
  k_cr_tasks passes, k_cr_walk, k_cr_len and of k_rt_probe from the library's "profile" spans, medians.  Rates: k-mers
  looked up per second by k_cr_probe and by k_rt_probe (the yardstick), walker steps per second of k_cr_walk (a step
  is one round of up to four neighbour lookups; mcx_graph_correct_walk_steps counts them).  Then the host entry
  mcx_graph_correct on the first `--host-reads` reads (wall clock; device ms of k_cr_emit; bytes of records).
One JSON line on stdout; `--out dir` also writes dir/correct_bench.json and dir/correct_bench.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ["k_cr_probe", "k_cr_tasks<false>", "k_cr_tasks<true>", "k_cr_walk", "k_cr_len"]


def step_kernel(runs, host_reads, two_way, error_rate):
    import numpy as np
    import torch
    import bench
    import bench_clean
    import bench_coverage
    g = bench_coverage.build_graph(1)
    n, width = bench_clean.BATCH, bench.READ_LEN + 1
    genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", 1)
    s = bench.make_batch(genome, n, 1000, "cuda:0")
    del genome
    assert s.numel() == n * width
    # substitutions: a base in `error_rate` of the positions becomes the next of A, C, G, T (separators stay)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    hit = torch.rand(s.numel(), device="cuda:0", generator=gen) < error_rate
    nxt = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    is_base = nxt[s.long()] != 0
    s = torch.where(hit & is_base, nxt[s.long()], s)
    nsub = int((hit & is_base).sum())
    del hit, is_base
    pitch = (s.numel() + 63) // 64 * 64
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * width
    d_hit = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    node = torch.empty(pitch, dtype=torch.int64, device="cuda:0")
    dlen = torch.empty(n, dtype=torch.int64, device="cuda:0")
    res = {"nkmers": g.nkmers, "runs": runs, "batch_reads": n, "substitutions": nsub, "two_way": bool(two_way), "host_reads": host_reads}
    g.correct_stream_dev(s, s.numel(), off, n, node, pitch, dlen, two_way=two_way)  # (warm-up: the first launch loads the code)
    g.configure("profile", 1)
    t = {k: [] for k in KERNELS + ["k_rt_probe"]}
    st = None
    for _ in range(runs):
        box = {}

        def call():
            box["st"] = g.correct_stream_dev(s, s.numel(), off, n, node, pitch, dlen, two_way=two_way)
        sp = bench_coverage.spans(g, call, KERNELS)
        for k in KERNELS:
            t[k].append(sp[k])
        st = box["st"]
        t["k_rt_probe"].append(bench_coverage.spans(g, lambda: g.reads_touch_stream_dev(s, s.numel(), off, n, d_hit), ["k_rt_probe"])["k_rt_probe"])
    steps = g.correct_walk_steps()
    res["stats"] = st.as_dict()
    res["walk_steps"] = steps
    res["kernels"] = {k: {"ms": [round(x, 3) for x in v], "ms_median": round(statistics.median(v), 3)} for k, v in t.items()}
    kmers = res["stats"]["num_kmers"]
    res["k_cr_probe_kmers_per_s"] = kmers / (statistics.median(t["k_cr_probe"]) * 1e-3)
    res["k_rt_probe_kmers_per_s"] = kmers / (statistics.median(t["k_rt_probe"]) * 1e-3)
    res["k_cr_walk_steps_per_s"] = steps / (statistics.median(t["k_cr_walk"]) * 1e-3)
    res["corrected_bytes"] = int(dlen.sum())
    # the host entry
    host = s.view(n, width)[:host_reads, :bench.READ_LEN].contiguous().cpu().numpy().reshape(-1)
    hoff = np.arange(host_reads + 1, dtype=np.uint64) * bench.READ_LEN
    g.correct(host[:bench.READ_LEN * 1000], hoff[:1001])  # (the staging buffers are pinned by the first call)
    box = {}

    def host_call():
        t0 = time.time()
        box["out"], _, _ = g.correct(host, hoff, two_way=two_way)
        box["s"] = time.time() - t0
    sp = bench_coverage.spans(g, host_call, KERNELS + ["k_cr_place", "k_cr_emit"])
    res["host_s"] = round(box["s"], 3)
    res["host_bytes"] = len(box["out"])
    res["host_ms"] = {k: round(v, 3) for k, v in sp.items()}
    g.configure("profile", 0)
    g.close()
    print(json.dumps(res))


def markdown(res):
    k = res["kernels"]
    rows = ["# `correct`: measurements", "",
            "`tools/bench_correct.py`, %d reads of 150 bp of the graph's genome with %d substituted bases, %s gap filling, medians of %d." %
            (res["batch_reads"], res["substitutions"], "two-way" if res["two_way"] else "one-way", res["runs"]), "",
            "| kernel | ms (median) | rate |", "|---|---|---|"]
    rates = {"k_cr_probe": "%.2f G k-mers looked up per second" % (res["k_cr_probe_kmers_per_s"] / 1e9),
             "k_rt_probe": "%.2f G k-mers looked up per second (the yardstick, same batch, same session)" % (res["k_rt_probe_kmers_per_s"] / 1e9),
             "k_cr_walk": "%.3f G walker steps per second (%d steps)" % (res["k_cr_walk_steps_per_s"] / 1e9, res["walk_steps"])}
    for name in KERNELS + ["k_rt_probe"]:
        rows.append("| `%s` | %.3f | %s |" % (name, k[name]["ms_median"], rates.get(name, "")))
    rows += ["", "Stats of one call: `%s`" % json.dumps(res["stats"]), "",
             "Host entry on the first %d reads: %.3f s for %d bytes of records; device ms `%s`." %
             (res["host_reads"], res["host_s"], res["host_bytes"], json.dumps(res["host_ms"])), ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-reads", type=int, default=500_000)
    ap.add_argument("--two-way", action="store_true")
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.host_reads, a.two_way, a.error_rate)
    args = ["--step", "kernel", "--runs", str(a.runs), "--host-reads", str(a.host_reads), "--error-rate", str(a.error_rate)]
    p = subprocess.run(["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__)] + args + (["--two-way"] if a.two_way else []),
                       stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    line = p.stdout.strip().splitlines()[-1]
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "correct_bench.json"), "w") as f:
            f.write(line + "\n")
        with open(os.path.join(a.out, "correct_bench.md"), "w") as f:
            f.write(markdown(json.loads(line)))


if __name__ == "__main__":
    main()
