#!/usr/bin/env python3
"""bench_bubbles.py -- `bubbles` on the MI355X (csrc/mcx_bubbles.h: mcx_graph_bubbles).

Workload: the C2 graph of tools/bench_clean.py (bench.py's shape at k = 31) as colour 0, and as colour 1 the reads of the
same genome with 0.1 % of its bases substituted and `--indels` short insertions and deletions (1 to 3 bases).  Both
colours hold the reads' own errors, so most forks are tips; the calls are the substitutions and indels between the two.

One child process under `timeout -k 10`.  A warm-up call (which also makes the decomposition and is reported apart) and
`--runs` timed calls of Graph.bubbles: the host-clock time of the call and, from the handle's profile spans ("profile"
knob: device time per kernel), the passes
  forks   k_bb_forks, k_bb_forklist, k_bb_hap (the key sort is reported as `sort`)
  walk    k_bb_walk_count, k_bb_walk_write
  group   k_bb_first, k_bb_group
  size    k_bb_size, k_bb_offsets
  emit    k_bb_emit
With `--command dir` the graph is written to dir/two.ctx and `mccortex31 bubbles` is timed end to end on it as well.
One JSON line on stdout; `--out dir` also writes dir/bubbles_bench.json."""
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

PHASES = {"forks": ("k_bb_forks", "k_bb_forklist", "k_bb_hap"), "walk": ("k_bb_walk_count", "k_bb_walk_write"), "group": ("k_bb_first", "k_bb_group"),
          "size": ("k_bb_size", "k_bb_offsets"), "emit": ("k_bb_emit",)}


def spans(g):
    """{kernel: ms} of the spans recorded since the profile was switched on; a templated kernel's span carries its
    arguments (k_bb_group<false>): they are folded into the kernel's name"""
    out = {}
    for name, (_calls, ms) in g.profile().items():
        name = name.split("<")[0]
        out[name] = out.get(name, 0.0) + ms
    return out


def phases_of(sp):
    """{pass: ms} from {kernel: ms}"""
    return {p: sum(sp.get(kn, 0.0) for kn in kns) for p, kns in PHASES.items()}


def mutate(genome, indels, seed):
    """0.1 % substitutions and `indels` insertions or deletions of 1 to 3 bases"""
    import torch
    gen = torch.Generator(device=genome.device)
    gen.manual_seed(seed)
    nxt = torch.zeros(256, dtype=torch.uint8, device=genome.device)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    hit = torch.rand(genome.numel(), device=genome.device, generator=gen) < 0.001
    out = torch.where(hit, nxt[genome.long()], genome)
    cuts = sorted(int(x) for x in torch.randint(1000, genome.numel() - 1000, (indels,), generator=gen, device=genome.device).cpu())
    parts, at = [], 0
    for i, c in enumerate(cuts):
        n = 1 + i % 3
        parts.append(out[at:c])
        if i % 2:
            parts.append(nxt[out[c:c + n].long()])  # an insertion
            at = c
        else:
            at = c + n                              # a deletion
    parts.append(out[at:])
    return torch.cat(parts)


def step_kernel(runs, genome_len, reads, indels, max_allele, max_flank, command_dir):
    import bench
    import bench_clean
    import mccortex_amd as mcx
    genome = bench.make_genome(genome_len, "cuda:0", 1)
    other = mutate(genome, indels, 11)
    batch = min(bench_clean.BATCH, reads)
    g = mcx.Graph(bench_clean.K, 2, 1 << 29)
    for c, gen in enumerate((genome, other)):
        for i in range(reads // batch):
            s = bench.make_batch(gen, batch, 1000 + i, "cuda:0")
            g.add_stream_dev(c, s, s.numel())
            del s
    g.sync()
    del genome, other
    res = {"k": bench_clean.K, "genome": genome_len, "reads_per_colour": reads, "indels": indels, "runs": runs, "kmers": int(g.nkmers),
           "max_allele": max_allele, "max_flank": max_flank}
    walls, ph, sorts, st, nbytes = [], [], [], None, 0
    for it in range(runs + 1):
        st = mcx.graph.BubblesStats()
        g.configure("profile", 1)
        t0 = time.perf_counter()
        _, text = g.bubbles(max_allele, max_flank, stats=st)
        w = time.perf_counter() - t0
        sp = spans(g)
        g.configure("profile", 0)
        nbytes = len(text)
        if it:
            walls.append(w)
            ph.append(phases_of(sp))
            sorts.append(sp.get("radix_sort_pairs", 0.0))
        else:
            res["first_call_s"] = round(w, 4)  # with the decomposition
    res["wall_s_median"] = round(statistics.median(walls), 4)
    res["phase_ms_median"] = {p: round(statistics.median(x[p] for x in ph), 3) for p in PHASES}
    res["sort_ms_median"] = round(statistics.median(sorts), 3)
    res["text_bytes"] = nbytes
    res["stats"] = st.as_dict()
    if command_dir:
        os.makedirs(command_dir, exist_ok=True)
        ctx, out = os.path.join(command_dir, "two.ctx"), os.path.join(command_dir, "two.bub.txt.gz")
        hdr = mcx.CtxHeader(bench_clean.K, 2)
        mcx.write_ctx(ctx, hdr, g.export(sorted_=False))
        g.close()
        cmd = [os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "bubbles", "-q", "-f", "-m", "16G", "-n", "512M", "-A", str(max_allele), "-F", str(max_flank), "-o", out, ctx]
        times = []
        for _ in range(runs):
            t0 = time.perf_counter()
            subprocess.run(["timeout", "-k", "10", "300"] + cmd, check=True)
            times.append(time.perf_counter() - t0)
        res["command_s_median"] = round(statistics.median(times), 3)
        res["command_out_bytes"] = os.path.getsize(out)
        os.remove(ctx)
    else:
        g.close()
    print(json.dumps(res))


def main():
    import bench
    import bench_clean
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--genome", type=int, default=bench.GENOME_PER_GPU)
    ap.add_argument("--reads", type=int, default=bench_clean.READS)
    ap.add_argument("--indels", type=int, default=20)
    ap.add_argument("--max-allele", type=int, default=2000)
    ap.add_argument("--max-flank", type=int, default=500)
    ap.add_argument("--command", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.genome, a.reads, a.indels, a.max_allele, a.max_flank, a.command)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--runs", str(a.runs), "--genome", str(a.genome),
                        "--reads", str(a.reads), "--indels", str(a.indels), "--max-allele", str(a.max_allele), "--max-flank", str(a.max_flank)]
                       + (["--command", a.command] if a.command else []), stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bubbles_bench.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
