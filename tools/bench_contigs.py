#!/usr/bin/env python3
"""bench_contigs.py -- `contigs` on the MI355X (csrc/mcx_contigs.h: mcx_graph_links_load_text, mcx_graph_contigs).

Workload: the C2 graph of tools/bench_thread.py (bench.py's shape at k = 31, one colour), `--reads` reads of 150 bp with
1 % of the bases substituted threaded through it, the links of that written as `links_text(seq=True)`, forgotten and
loaded again from the text in pieces of `--piece` bytes (the load phase), then `--seeds` seed k-mers taken from the
reads walked with reseeding (every seed gives a contig: the walks phase alone) and without (with the resolve phase).

One child process under `timeout -k 10`.  Per configuration a warm-up call and `--runs` timed calls: the host-clock time
of the call and, from the handle's profile spans ("profile" knob: device time per kernel), the phases
  load     k_lk_mark .. k_cg_parse, k_lk_store, k_cg_links and the sort and reduce of `thread`
  walks    k_cg_walk (all launches, the reruns included)
  resolve  k_cg_unvisited, k_cg_claim, k_cg_hits, k_cg_visit
  text     k_cg_text
One JSON line on stdout; `--out dir` also writes dir/contigs_bench.json."""
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

PHASES = {"walks": ("k_cg_walk",), "resolve": ("k_cg_unvisited", "k_cg_claim", "k_cg_hits", "k_cg_visit"), "text": ("k_cg_text",)}


def spans(g):
    """{kernel: ms} of the spans recorded since the profile was switched on (configure("profile", 1) clears them);
    a templated kernel's span carries its arguments (k_cg_claim<false>): they are folded into the kernel's name"""
    out = {}
    for name, (_calls, ms) in g.profile().items():
        name = name.split("<")[0]
        out[name] = out.get(name, 0.0) + ms
    return out


def phases_of(sp):
    """{phase: ms} from {kernel: ms}"""
    return {p: sum(sp.get(kn, 0.0) for kn in kns) for p, kns in PHASES.items()}


def step_kernel(runs, reads, piece, nseeds):
    import numpy as np
    import torch
    import bench
    import bench_clean
    import bench_coverage
    import bench_links
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
    clean = s.view(n, width)[:reads, :bench.READ_LEN].contiguous().cpu().numpy()
    s = torch.where(hit & is_base, nxt[s.long()], s)
    host = s.view(n, width)[:reads, :bench.READ_LEN].contiguous().cpu().numpy().reshape(-1)
    del s, hit, is_base
    g.thread(host, np.arange(reads + 1, dtype=np.uint64) * bench.READ_LEN)
    info = g.links_info()
    hist = dict(g.links_contig_hist())
    text = g.links_text(seq=True)
    parts = bench_links.pieces_of(text, piece)
    res = {"reads": reads, "runs": runs, "piece_bytes": piece, "text_bytes": len(text), "links": info, "seeds": nseeds}
    loads = []
    for it in range(runs + 1):
        g.links_reset()
        t0 = time.perf_counter()
        for p in parts:
            g.links_load_text(p)
        g.links_info()  # (merges what is pending)
        if it:
            loads.append(time.perf_counter() - t0)
    res["load_s_median"] = round(statistics.median(loads), 4)
    res["load_text_GBps"] = round(len(text) / statistics.median(loads) / 1e9, 3)
    # the confidence table as the command computes it, in Python here (tests/contigs_restate.py)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import contigs_restate
    conf = contigs_restate.conf_table(hist, int(g.nkmers))
    seeds = [bytes(clean[i * (reads // nseeds), 40:40 + 31]).decode() for i in range(nseeds)]
    seeds = [s for s in seeds if not set(s) - set("ACGT")]  # (the batch holds reads with N)
    res["seeds"] = len(seeds)
    res["configs"] = {}
    for name, kw in (("reseed", {"reseed": True}), ("no_reseed", {"reseed": False})):
        walls, ph, st = [], [], None
        for it in range(runs + 1):
            g.configure("profile", 1)
            t0 = time.perf_counter()
            _, _, st = g.contigs(conf, seeds=seeds, **kw)
            w = time.perf_counter() - t0
            sp = spans(g)
            g.configure("profile", 0)
            if it:
                walls.append(w)
                ph.append(phases_of(sp))
        res["configs"][name] = {"wall_s_median": round(statistics.median(walls), 4), "stats": st.as_dict(),
                                "phase_ms_median": {p: round(statistics.median(x[p] for x in ph), 3) for p in PHASES}}
    g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--piece", type=int, default=64 << 20)
    ap.add_argument("--seeds", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.reads, a.piece, a.seeds)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--runs", str(a.runs), "--reads", str(a.reads),
                        "--piece", str(a.piece), "--seeds", str(a.seeds)], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "contigs_bench.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
