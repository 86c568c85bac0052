#!/usr/bin/env python3
"""bench_unitigs.py -- `unitigs` on the MI355X (csrc/mcx_unitigs.h: mcx_graph_unitigs).

Workload: bench_clean.py's -- the C2 shape of bench.py at k = 31, 10 M x 150 bp reads from its 200 Mbp genome,
a one-colour graph in HBM.

Steps, each in a child process of its own under `timeout -k 10`, the next one only when the previous succeeded:
  1. kernel: mcx_graph_unitig_stats once (the decomposition is then cached), then Graph.unitigs 5 times per format
     into a sink that drops the text: device ms of the rank (k_cl_links, k_un_init .. k_un_reinit), order
     (k_un_heads .. k_un_edges, the radix sort) and emit (k_un_emit, k_un_text) kernels from the library's "profile"
     spans, median; wall clock of the call; output bytes; emit GB/s beside the device-to-device copy rate of the
     same box (mcx_ubench_stream).
  2. e2e: `mccortex31 unitigs -o` per format on the graph written as a .ctx, wall clock (process start to exit).
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RANK = ("k_cl_links", "k_un_init", "k_un_jump", "k_un_mark", "k_un_cyc_reset", "k_un_cyc_min", "k_un_cyc_keep", "k_un_cut", "k_un_reinit")
ORDER = ("k_un_heads", "k_un_keyword", "radix_sort_pairs", "k_un_number", "k_un_narrow", "k_un_place", "k_un_edges")
EMIT = ("k_un_emit<UnUnits>", "k_un_emit<UnEdges>", "k_un_text")


def step_kernel(ctx_path, runs):
    import bench_clean
    import mccortex_amd as mcx
    from mccortex_amd import graph as G
    from oracle import ctxio
    g = bench_clean.build_graph()
    n = g.nkmers
    if ctx_path:
        with open(ctx_path, "wb") as f:
            f.write(ctxio.header_bytes(bench_clean.K, [ctxio.GraphInfo()]))
            f.write(g.export(sorted_=False))
    L = mcx.lib()
    copy = [C.c_double(), C.c_double(), C.c_double()]
    L.mcx_ubench_stream(0, 1 << 30, *[C.byref(x) for x in copy])
    g.unitig_stats()
    g.configure("profile", 1)
    nbytes = [0]

    def sink(_ctx, _ptr, nb):
        nbytes[0] += nb
        return 0

    cb = G.SINK_FN(sink)
    res = {"nkmers": n, "copy_GBps": [round(x.value, 1) for x in copy]}
    for fmt in ("fasta", "gfa", "dot"):
        groups, walls = {"rank": [], "order": [], "emit": []}, []
        st = G.UnitigsStats()
        for _ in range(runs):
            p0 = g.profile()
            nbytes[0] = 0
            t0 = time.time()
            G._check(L.mcx_graph_unitigs(g.h, G.UNITIGS_FORMATS[fmt], 0, cb, None, C.byref(st)))
            walls.append((time.time() - t0) * 1e3)
            p1 = g.profile()
            d = {name: p1[name][1] - p0.get(name, (0, 0.0))[1] for name in p1}
            for grp, names in (("rank", RANK), ("order", ORDER), ("emit", EMIT)):
                groups[grp].append(sum(d.get(x, 0.0) for x in names))
            rounds = (p1.get("k_un_jump", (0, 0))[0] - p0.get("k_un_jump", (0, 0))[0])
        emit_ms = statistics.median(groups["emit"])
        res[fmt] = {"rank_ms": round(statistics.median(groups["rank"]), 2), "order_ms": round(statistics.median(groups["order"]), 2),
                    "emit_ms": round(emit_ms, 2), "call_wall_ms": round(statistics.median(walls), 1), "bytes": nbytes[0],
                    "emit_GBps": round(nbytes[0] / 1e6 / emit_ms, 1) if emit_ms else None, "jump_rounds": rounds}
        res.update(num_unitigs=int(st.num_unitigs), num_cycles=int(st.num_cycles))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--ctx", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    if a.step == "kernel":
        step_kernel(a.ctx, a.runs)
        return
    tmp = tempfile.mkdtemp(prefix="bench_unitigs_")
    ctx = None if a.no_e2e else os.path.join(tmp, "raw.ctx")
    cmd = ["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--runs", str(a.runs)]
    p = subprocess.run(cmd + (["--ctx", ctx] if ctx else []), stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    if ctx:
        for fmt, opt in (("fasta", "-F"), ("gfa", "-g"), ("dot", "-d")):
            out = os.path.join(tmp, "out." + fmt)
            t0 = time.time()
            q = subprocess.run(["timeout", "-k", "10", "600", os.path.join(ROOT, "mccortex_amd", "bin", "mccortex31"), "unitigs", "-q", "-f",
                                opt, "-m", "20G", "-n", "512M", "-o", out, ctx])
            if q.returncode != 0:
                break
            res[fmt]["e2e_s"] = round(time.time() - t0, 3)
            os.remove(out)
        os.remove(ctx)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
