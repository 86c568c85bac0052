#!/usr/bin/env python3
"""bench_thread.py -- `thread` on the MI355X (csrc/mcx_thread.h: mcx_graph_thread, mcx_graph_links_*).

Workload: the C2 graph of tools/bench_reads.py (bench.py's shape at k = 31, 10 M x 150 bp reads from its 200 Mbp
genome, about 227 M k-mers, one colour) and the first `--reads` reads of the first batch it was built from with 1 % of
the bases substituted, given to the host entry (`thread` has no device-stream entry).

One child process under `timeout -k 10`:
  a warm-up call, then `--runs` times links_reset + mcx_graph_thread (one-way; `--two-way` for the other mode): wall
  clock of the call and device ms of every pass from the library's "profile" spans, medians; then the same reads in
  `--calls` calls without a reset in between (the store's merges amortised); then mcx_graph_links_info and
  mcx_graph_links_text (wall clock, device ms of the two k_th_text passes, bytes of text).
One JSON line on stdout; `--out dir` also writes dir/thread_bench.json and dir/thread_bench.md."""
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

KERNELS = ["k_cr_probe", "k_cr_place", "k_th_tasks_count", "k_th_tasks_write", "k_cr_walk", "k_th_nodes<false>", "k_th_nodes<true>", "k_th_junc",
           "k_th_pack", "k_th_links", "k_th_word", "radix_sort_pairs", "k_th_heads", "k_th_runs", "k_th_reduce", "k_th_copy"]
TEXT_KERNELS = ["k_th_text<len>", "k_th_text<emit>"]


def step_kernel(runs, reads, calls, two_way, error_rate):
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
    assert s.numel() == n * width and reads <= n
    # substitutions: a base in `error_rate` of the positions becomes the next of A, C, G, T (separators stay)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    hit = torch.rand(s.numel(), device="cuda:0", generator=gen) < error_rate
    nxt = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    is_base = nxt[s.long()] != 0
    s = torch.where(hit & is_base, nxt[s.long()], s)
    host = s.view(n, width)[:reads, :bench.READ_LEN].contiguous().cpu().numpy().reshape(-1)
    del s, hit, is_base
    hoff = np.arange(reads + 1, dtype=np.uint64) * bench.READ_LEN
    res = {"nkmers": g.nkmers, "runs": runs, "reads": reads, "calls": calls, "two_way": bool(two_way)}
    g.thread(host[:bench.READ_LEN * 1000], hoff[:1001], two_way=two_way)  # (warm-up: code objects, pinned staging buffers)
    g.links_text()
    g.configure("profile", 1)
    t = {k: [] for k in KERNELS}
    wall, st = [], None
    for _ in range(runs):
        g.links_reset()
        box = {}

        def call():
            t0 = time.time()
            box["st"] = g.thread(host, hoff, two_way=two_way)
            box["s"] = time.time() - t0
        sp = bench_coverage.spans(g, call, KERNELS)
        for k in KERNELS:
            t[k].append(sp[k])
        wall.append(box["s"])
        st = box["st"]
    res["stats"] = st.as_dict()
    res["thread_s"] = [round(x, 4) for x in wall]
    res["thread_s_median"] = round(statistics.median(wall), 4)
    res["kernels"] = {k: {"ms": [round(x, 3) for x in v], "ms_median": round(statistics.median(v), 3)} for k, v in t.items()}
    res["reads_per_s"] = reads / statistics.median(wall)
    res["links_generated_per_s"] = res["stats"]["links_added"] / statistics.median(wall)
    whole = g.links_info()
    # the same reads in `calls` calls: the batches' links wait as sorted segments and are merged as they outgrow the store
    g.links_reset()
    per = (reads + calls - 1) // calls
    t0 = time.time()
    for a in range(0, reads, per):
        b = min(reads, a + per)
        g.thread(host[a * bench.READ_LEN:b * bench.READ_LEN], hoff[:b - a + 1], two_way=two_way)
    res["in_calls_s"] = round(time.time() - t0, 4)
    assert g.links_info() == whole
    res["links"] = whole
    box = {}

    def text_call():
        t0 = time.time()
        box["text"] = g.links_text()
        box["s"] = time.time() - t0
    sp = bench_coverage.spans(g, text_call, TEXT_KERNELS)
    res["text_s"] = round(box["s"], 4)
    res["text_bytes"] = len(box["text"])
    res["text_ms"] = {k: round(v, 3) for k, v in sp.items()}
    g.configure("profile", 0)
    g.close()
    print(json.dumps(res))


def markdown(res):
    k = res["kernels"]
    rows = ["# `thread`: measurements", "",
            "`tools/bench_thread.py`, the host entry on %d reads of 150 bp of the graph's genome with 1 %% of the bases substituted, %s gap filling, "
            "medians of %d." % (res["reads"], "two-way" if res["two_way"] else "one-way", res["runs"]), "",
            "`mcx_graph_thread`: %.4f s per call (wall clock, the call ends synchronised): %.2f M reads and %.2f M generated links per second." %
            (res["thread_s_median"], res["reads_per_s"] / 1e6, res["links_generated_per_s"] / 1e6), "",
            "| kernel (all launches of a call) | ms (median) |", "|---|---|"]
    for name in KERNELS:
        rows.append("| `%s` | %.3f |" % (name, k[name]["ms_median"]))
    rows += ["", "Stats of one call: `%s`" % json.dumps(res["stats"]), "",
             "The same reads in %d calls without a reset in between: %.4f s (the links kept are the same: `%s`)." %
             (res["calls"], res["in_calls_s"], json.dumps(res["links"])), "",
             "`mcx_graph_links_text` with seq= and juncpos=: %.4f s for %d bytes; device ms `%s`." %
             (res["text_s"], res["text_bytes"], json.dumps(res["text_ms"])), ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--two-way", action="store_true")
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.reads, a.calls, a.two_way, a.error_rate)
    args = ["--step", "kernel", "--runs", str(a.runs), "--reads", str(a.reads), "--calls", str(a.calls), "--error-rate", str(a.error_rate)]
    p = subprocess.run(["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__)] + args + (["--two-way"] if a.two_way else []),
                       stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    line = p.stdout.strip().splitlines()[-1]
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "thread_bench.json"), "w") as f:
            f.write(line + "\n")
        with open(os.path.join(a.out, "thread_bench.md"), "w") as f:
            f.write(markdown(json.loads(line)))


if __name__ == "__main__":
    main()
