#!/usr/bin/env python3
"""bench_links.py -- `links` on the MI355X (csrc/mcx_links.h: mcx_links_*).

Workload: the C2 graph of tools/bench_thread.py (bench.py's shape at k = 31, one colour), `--reads` reads of 150 bp with
1 % of the bases substituted threaded through it, and the raw links of that as `links_text(seq=True)`: the body of the
.ctp file `thread` would write.  The body goes through one Links handle in pieces of `--piece` bytes (64 MB), cut where
the command cuts them (before a k-mer line).

One child process under `timeout -k 10`.  Three configurations -- the histogram at its defaults, clean 2, and both --
each with a warm-up pass and `--runs` timed passes over the whole body: the host-clock time of the calls, GB/s of input
text, and per phase the library's own figures (mcx_links_phases: host clock around each phase, every phase ends
synchronised, so a phase's figure is the device time of its kernels plus its launches and scans; the engine has no
per-kernel event spans).  As context, from the same session: a plain pinned host -> device copy of the same bytes.
One JSON line on stdout; `--out dir` also writes dir/links_bench.json and dir/links_bench.md."""
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

CONFIGS = [("hist", {"hist": (6, 100)}), ("clean2", {"clean": 2}), ("clean2_hist", {"clean": 2, "hist": (6, 100)})]


def pieces_of(text, piece):
    """cut before the last k-mer line that begins within each `piece` bytes"""
    out, at = [], 0
    while at < len(text):
        end = min(len(text), at + piece)
        if end < len(text):
            cut = end
            while True:
                cut = text.rfind(b"\n", at, cut)
                if cut < 0 or text[cut + 1:cut + 2] in (b"A", b"C", b"G", b"T"):
                    break
            end = cut + 1 if cut > at else len(text)
        out.append(text[at:end])
        at = end
    return out


def step_kernel(runs, reads, piece):
    import numpy as np
    import torch
    import bench
    import bench_clean
    import bench_coverage
    import mccortex_amd as mcx
    g = bench_coverage.build_graph(1)
    n, width = bench_clean.BATCH, bench.READ_LEN + 1
    genome = bench.make_genome(bench.GENOME_PER_GPU, "cuda:0", 1)
    s = bench.make_batch(genome, n, 1000, "cuda:0")
    del genome
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    hit = torch.rand(s.numel(), device="cuda:0", generator=gen) < 0.01
    nxt = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    is_base = nxt[s.long()] != 0
    s = torch.where(hit & is_base, nxt[s.long()], s)
    host = s.view(n, width)[:reads, :bench.READ_LEN].contiguous().cpu().numpy().reshape(-1)
    del s, hit, is_base
    g.thread(host, np.arange(reads + 1, dtype=np.uint64) * bench.READ_LEN)
    info = g.links_info()
    text = g.links_text(seq=True)
    g.close()
    torch.cuda.empty_cache()
    parts = pieces_of(text, piece)
    assert b"".join(parts) == text
    res = {"reads": reads, "runs": runs, "piece_bytes": piece, "pieces": len(parts), "text_bytes": len(text), "links_in_file": info, "configs": {}}
    for name, opt in CONFIGS:
        walls, phases, st = [], [], None
        for it in range(runs + 1):
            L = mcx.Links(31)
            t0 = time.perf_counter()
            for p in parts:
                L.add(p, ctp="clean" in opt, rows=False, **opt)
            w = time.perf_counter() - t0
            st = L.stats()
            ph = L.phases()
            L.close()
            if it:
                walls.append(w)
                phases.append(ph)
        med = statistics.median(walls)
        res["configs"][name] = {"wall_s": [round(x, 4) for x in walls], "wall_s_median": round(med, 4), "text_GBps": round(len(text) / med / 1e9, 3),
                                "phase_ms_median": {k: round(statistics.median(p[k] for p in phases), 3) for k in phases[0]}, "stats": st}
    # context: the same bytes from pinned memory to the device, nothing else
    pin = torch.empty(len(text), dtype=torch.uint8).pin_memory()
    pin.numpy()[:] = np.frombuffer(text, dtype=np.uint8)
    dev = torch.empty(len(text), dtype=torch.uint8, device="cuda:0")
    copies = []
    for it in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.copy_(pin, non_blocking=True)
        torch.cuda.synchronize()
        if it:
            copies.append(time.perf_counter() - t0)
    res["pinned_copy_s_median"] = round(statistics.median(copies), 5)
    res["pinned_copy_GBps"] = round(len(text) / statistics.median(copies) / 1e9, 2)
    print(json.dumps(res))


def markdown(res):
    rows = ["# `links`: measurements", "",
            "`tools/bench_links.py`: the raw links of %d reads of 150 bp threaded through the C2 graph (k = 31), %d bytes of .ctp body with seq= and "
            "juncpos= (%s), through one `Links` handle in %d pieces of at most %d bytes; a warm-up pass, then medians of %d passes.  The text comes "
            "from pageable host memory (Python bytes), the .ctp text is delivered where there is a cut-off, list rows are not made." %
            (res["reads"], res["text_bytes"], json.dumps(res["links_in_file"]), res["pieces"], res["piece_bytes"], res["runs"]), "",
            "| configuration | calls, wall clock s | GB/s of input text | " + " | ".join(k for k in next(iter(res["configs"].values()))["phase_ms_median"]) + " |",
            "|---|---|---|" + "---|" * len(next(iter(res["configs"].values()))["phase_ms_median"])]
    for name, c in res["configs"].items():
        rows.append("| %s | %.4f | %.3f | %s |" % (name, c["wall_s_median"], c["text_GBps"], " | ".join("%.2f" % v for v in c["phase_ms_median"].values())))
    rows += ["", "The phase columns are the library's host-clock milliseconds around each phase (`mcx_links_phases`); every phase ends synchronised, so a "
             "figure is the device time of the phase's kernels with their launches, scans and allocations.  There are no per-kernel event spans in this engine.",
             "", "Context from the same session: a plain pinned host-to-device copy of the same %d bytes takes %.5f s (%.2f GB/s)." %
             (res["text_bytes"], res["pinned_copy_s_median"], res["pinned_copy_GBps"]), "",
             "Stats of the last configuration: `%s`" % json.dumps(list(res["configs"].values())[-1]["stats"]), ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--piece", type=int, default=64 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.reads, a.piece)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--runs", str(a.runs), "--reads", str(a.reads),
                        "--piece", str(a.piece)], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "links_bench.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        with open(os.path.join(a.out, "links_bench.md"), "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
