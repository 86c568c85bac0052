#!/usr/bin/env python3
"""bench_pjoin.py -- `pjoin` on the MI355X (csrc/mcx_pjoin.h: mcx_pjoin_*).

Workload: `--files` synthetic one-colour .ctp bodies of about `--bytes` bytes each (random k-mers of k = 31 in blocks of 1
to 8 links of 1 to `--max-juncs` junctions, counts 1..3, no tags), a share `--shared` of every file's blocks taken from
the first file so that links meet; every file into a colour of its own through one Pjoin handle, then finish.

One child process under `timeout -k 10`.  A warm-up pass and `--runs` timed passes: the host-clock time of the adds and
of finish, GB/s of input text, and the library's six phases (mcx_pjoin_phases: host clock around each phase, every phase
ends synchronised).  The nearest comparable, from the same session: mcx_links_add_text on the same bytes (the files
with seq= and juncpos= tags added, which `links` requires; its histogram configuration, no text made).
One JSON line on stdout; `--out dir` also writes dir/pjoin_bench.json and dir/pjoin_bench.md."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 31


def make_blocks(rng, nbytes, max_juncs):
    """blocks of a body: [(plain text, the same with seq= and juncpos= tags)]"""
    out, size = [], 0
    while size < nbytes:
        kmer = "".join(rng.choice("ACGT") for _ in range(K))
        n = rng.randint(1, 8)
        plain, tagged = ["%s %d" % (kmer, n)], ["%s %d" % (kmer, n)]
        for _ in range(n):
            j = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, max_juncs)))
            ln = "%s %d %d %s" % (rng.choice("FR"), len(j), rng.randint(1, 3), j)
            plain.append(ln)
            tagged.append("%s seq=%s%s juncpos=%s" % (ln, kmer, j, ",".join(map(str, range(len(j))))))
        a, b = "\n".join(plain) + "\n", "\n".join(tagged) + "\n"
        out.append((a, b))
        size += len(a)
    return out


def make_files(nfiles, nbytes, max_juncs, shared, seed=1):
    rng = random.Random(seed)
    first = make_blocks(rng, nbytes, max_juncs)
    files = [first]
    for _ in range(nfiles - 1):
        own = make_blocks(rng, int(nbytes * (1 - shared)), max_juncs)
        blocks = own + rng.sample(first, int(len(first) * shared))
        rng.shuffle(blocks)
        files.append(blocks)
    return [("".join(a for a, _ in f).encode(), "".join(b for _, b in f).encode()) for f in files]


def step_kernel(a):
    import mccortex_amd as mcx
    files = make_files(a.files, a.bytes, a.max_juncs, a.shared)
    total = sum(len(p) for p, _ in files)
    res = {"files": a.files, "runs": a.runs, "bytes_per_file": [len(p) for p, _ in files], "text_bytes": total, "max_juncs": a.max_juncs, "shared": a.shared}
    adds, fins, phases, st = [], [], [], None
    for it in range(a.runs + 1):
        P = mcx.Pjoin(K, a.files)
        t0 = time.perf_counter()
        for c, (plain, _) in enumerate(files):
            P.add(plain, 1, [(0, c)])
        t1 = time.perf_counter()
        P.finish(keep=False)
        t2 = time.perf_counter()
        st, ph = P.stats(), P.phases()
        out_bytes = sum(P.chunks)
        P.close()
        if it:
            adds.append(t1 - t0)
            fins.append(t2 - t1)
            phases.append(ph)
    res["pjoin"] = {"add_s": [round(x, 4) for x in adds], "add_s_median": round(statistics.median(adds), 4), "finish_s_median": round(statistics.median(fins), 4),
                    "add_text_GBps": round(total / statistics.median(adds) / 1e9, 3), "out_bytes": out_bytes,
                    "phase_ms_median": {k: round(statistics.median(p[k] for p in phases), 3) for k in phases[0]}, "stats": st}
    walls, lph = [], []
    tagged_total = sum(len(t) for _, t in files)
    for it in range(a.runs + 1):
        L = mcx.Links(K)
        t0 = time.perf_counter()
        for _, tagged in files:
            L.add(tagged, hist=(6, 100), ctp=False, rows=False)
        w = time.perf_counter() - t0
        ph = L.phases()
        L.close()
        if it:
            walls.append(w)
            lph.append(ph)
    res["links_same_blocks"] = {"text_bytes": tagged_total, "wall_s_median": round(statistics.median(walls), 4),
                                "text_GBps": round(tagged_total / statistics.median(walls) / 1e9, 3),
                                "phase_ms_median": {k: round(statistics.median(p[k] for p in lph), 3) for k in lph[0]}}
    print(json.dumps(res))


def markdown(res):
    p, lk = res["pjoin"], res["links_same_blocks"]
    rows = ["# `pjoin`: measurements", "",
            "`tools/bench_pjoin.py`: %d synthetic one-colour bodies (k = 31, links of 1 to %d junctions, %.0f %% of every later file's blocks shared with the "
            "first), %d bytes of text in all, each file into a colour of its own through one `Pjoin` handle; a warm-up pass, then medians of %d passes.  The "
            "text comes from pageable host memory (Python bytes)." % (res["files"], res["max_juncs"], 100 * res["shared"], res["text_bytes"], res["runs"]), "",
            "| | wall clock s | GB/s of input text | " + " | ".join(p["phase_ms_median"]) + " |", "|---|---|---|" + "---|" * len(p["phase_ms_median"]),
            "| the adds (and finish: %.4f s, %d bytes out) | %.4f | %.3f | %s |" % (p["finish_s_median"], p["out_bytes"], p["add_s_median"], p["add_text_GBps"],
                                                                                    " | ".join("%.2f" % v for v in p["phase_ms_median"].values())), "",
            "The nearest comparable, same session: `mcx_links_add_text` (histogram, no text) on the same blocks with the seq= and juncpos= tags `links` "
            "requires, %d bytes: %.4f s, %.3f GB/s of its input; phases `%s`." % (lk["text_bytes"], lk["wall_s_median"], lk["text_GBps"], json.dumps(lk["phase_ms_median"])),
            "", "Stats: `%s`" % json.dumps(p["stats"]), ""]
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--bytes", type=int, default=32 << 20)
    ap.add_argument("--max-juncs", type=int, default=40)
    ap.add_argument("--shared", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a)
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--step", "kernel", "--runs", str(a.runs), "--files", str(a.files),
                        "--bytes", str(a.bytes), "--max-juncs", str(a.max_juncs), "--shared", str(a.shared)], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "pjoin_bench.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        with open(os.path.join(a.out, "pjoin_bench.md"), "w") as f:
            f.write(markdown(res))


if __name__ == "__main__":
    main()
