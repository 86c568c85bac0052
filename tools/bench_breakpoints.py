#!/usr/bin/env python3
"""bench_breakpoints.py -- `breakpoints` on the MI355X (csrc/mcx_breakpoints.h: mcx_graph_breakpoints).

Workload: the C2 graph of tools/bench_clean.py (bench.py's shape at k = 31: reads of a random genome) as the sample
colour, and as the trusted reference that genome with 0.1 % of its bases substituted and `--indels` short insertions and
deletions planted (tools/bench_bubbles.py's `mutate`), one chromosome.  The graph is not cleaned, so most breaks are
sequencing errors.

One child process under `timeout -k 10`.  A first call, which loads the reference into the last colour and makes the
dense ids (reported apart), then `--runs` timed calls of Graph.breakpoints with ref_loaded: the host-clock time of the
call and, from the handle's profile spans ("profile" knob: device time per kernel), the passes
  index   k_bp_kmers_probe, k_bp_pack, k_bp_occ_sort (the stable sort of the occurrences by k-mer), k_bp_count
          (the key sort of the breaks is reported apart as `sort`)
  breaks  k_bp_breaks, k_bb_forklist
  walk    k_bp_walk_count, k_bp_walk_write
  merge   k_bp_merge, k_bp_calls
  size    k_bp_size, k_bp_offsets
  emit    k_bp_emit
With `--command dir` the sample graph and the reference are written to dir and `mccortex31 breakpoints` is timed end to
end on them as well.  One JSON line on stdout; `--out dir` also writes dir/breakpoints_bench.json."""
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

PHASES = {"index": ("k_bp_kmers_probe", "k_bp_pack", "k_bp_occ_sort", "k_bp_count"), "breaks": ("k_bp_breaks", "k_bb_forklist"), "walk": ("k_bp_walk_count", "k_bp_walk_write"),
          "merge": ("k_bp_merge", "k_bp_calls"), "size": ("k_bp_size", "k_bp_offsets"), "emit": ("k_bp_emit",)}


def spans(g):
    """{kernel: ms} of the spans recorded since the profile was switched on; a templated kernel's span carries its
    arguments (k_bp_calls<false>): they are folded into the kernel's name"""
    out = {}
    for name, (_calls, ms) in g.profile().items():
        name = name.split("<")[0]
        out[name] = out.get(name, 0.0) + ms
    return out


def phases_of(sp):
    """{pass: ms} from {kernel: ms}"""
    return {p: sum(sp.get(kn, 0.0) for kn in kns) for p, kns in PHASES.items()}


def step_kernel(runs, genome_len, reads, indels, min_ref, max_ref, command_dir):
    import bench
    import bench_bubbles
    import bench_clean
    import mccortex_amd as mcx
    genome = bench.make_genome(genome_len, "cuda:0", 1)
    ref = bytes(bench_bubbles.mutate(genome, indels, 11).cpu().numpy().tobytes())
    batch = min(bench_clean.BATCH, reads)
    g = mcx.Graph(bench_clean.K, 2, 1 << 29)
    for i in range(reads // batch):
        s = bench.make_batch(genome, batch, 1000 + i, "cuda:0")
        g.add_stream_dev(0, s, s.numel())
        del s
    g.sync()
    del genome
    res = {"k": bench_clean.K, "genome": genome_len, "reads": reads, "indels": indels, "runs": runs, "sample_kmers": int(g.nkmers), "min_ref": min_ref,
           "max_ref": max_ref}
    if command_dir:  # the sample graph as the command reads it, before the reference goes in
        os.makedirs(command_dir, exist_ok=True)
        ctx = os.path.join(command_dir, "sample.ctx")
        mcx.write_ctx(ctx, mcx.CtxHeader(bench_clean.K, 2), g.export(sorted_=False))  # (the command takes its colour 0: `sample.ctx:0`)
    walls, ph, sorts, st, nbytes = [], [], [], None, 0
    for it in range(runs + 1):
        st = mcx.graph.BreakpointsStats()
        g.configure("profile", 1)
        t0 = time.perf_counter()
        _, text = g.breakpoints([ref], ["chr1"], min_ref, max_ref, ref_loaded=it > 0, stats=st)
        w = time.perf_counter() - t0
        sp = spans(g)
        g.configure("profile", 0)
        nbytes = len(text)
        if it:
            walls.append(w)
            ph.append(phases_of(sp))
            sorts.append(sp.get("radix_sort_pairs", 0.0))
        else:
            res["first_call_s"] = round(w, 4)  # with the reference's load and the dense ids
            res["ref_added"] = int(st.ref_added)
    res["kmers"] = int(g.nkmers)
    res["wall_s_median"] = round(statistics.median(walls), 4)
    res["phase_ms_median"] = {p: round(statistics.median(x[p] for x in ph), 3) for p in PHASES}
    res["sort_ms_median"] = round(statistics.median(sorts), 3)
    res["text_bytes"] = nbytes
    res["stats"] = st.as_dict()
    g.close()
    if command_dir:
        fa, out = os.path.join(command_dir, "ref.fa"), os.path.join(command_dir, "calls.txt.gz")
        with open(fa, "wb") as f:
            f.write(b">chr1\n" + ref + b"\n")
        cmd = [os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "breakpoints", "-q", "-f", "-m", "16G", "-n", "512M", "-r", str(min_ref), "-R", str(max_ref),
               "-s", fa, "-o", out, ctx + ":0"]
        times = []
        for _ in range(runs):
            t0 = time.perf_counter()
            subprocess.run(["timeout", "-k", "10", "300"] + cmd, check=True)
            times.append(time.perf_counter() - t0)
        res["command_s_median"] = round(statistics.median(times), 3)
        res["command_out_bytes"] = os.path.getsize(out)
        os.remove(ctx)
        os.remove(fa)
    print(json.dumps(res))


def main():
    import bench
    import bench_clean
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--genome", type=int, default=bench.GENOME_PER_GPU)
    ap.add_argument("--reads", type=int, default=bench_clean.READS)
    ap.add_argument("--indels", type=int, default=20)
    ap.add_argument("--min-ref", type=int, default=5)
    ap.add_argument("--max-ref", type=int, default=1000)
    ap.add_argument("--command", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a.runs, a.genome, a.reads, a.indels, a.min_ref, a.max_ref, a.command)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--runs", str(a.runs), "--genome", str(a.genome),
                        "--reads", str(a.reads), "--indels", str(a.indels), "--min-ref", str(a.min_ref), "--max-ref", str(a.max_ref)]
                       + (["--command", a.command] if a.command else []), stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "breakpoints_bench.json"), "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
