"""Graph.add_reads through the ASCII staging layout (MCX_PACKED=0) with small chunks: MCX_STAGE_BYTES = 1024 makes a
chunk of 128 carried bytes and at most 1024 new ones.  The reads here spread over many chunks and straddle their
seams, and one is longer than two chunks and goes in pieces with an N inside.  The records, the k-mer count and the
load statistics are compared with the dictionary restatement (clean_restate.build) and with the packed layout (the
default) fed the same reads.  Both variables are read once per process, so the device part runs in child processes
(this file, run as a script)."""
import json
import os
import random
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clean_restate as R  # noqa: E402

CHUNK = 1024
STATS = ("num_se_reads", "total_bases_read", "num_good_reads", "num_bad_reads", "total_bases_loaded", "contigs_parsed",
         "num_kmers_loaded", "num_kmers_novel")


def case(k):
    """the seeds of test_gpu_subgraph_seams and a read of 2101 bases, longer than two chunks, that holds an N"""
    from test_gpu_subgraph import rseq
    from test_gpu_subgraph_seams import case as seams_case
    _, reads = seams_case(k)
    rng = random.Random(900 + k)
    genome = reads[0] + rseq(rng, 700)
    return reads[:7] + [genome[:640] + rseq(rng, 260) + "N" + rseq(rng, 600) + genome[40:640]] + reads[7:]


def expected(reads, k):
    """what loading the reads into an empty one-colour graph leaves: the graph and the load statistics"""
    reads = [s.upper() for s in reads]  # (the loader takes lower case as the same bases)
    graph = R.build([reads], k)
    contigs = [[c for c in re.split("[^ACGT]+", s) if len(c) >= k] for s in reads]
    st = {"num_se_reads": len(reads), "total_bases_read": sum(len(s) for s in reads),
          "num_good_reads": sum(1 for cs in contigs if cs), "num_bad_reads": sum(1 for cs in contigs if not cs),
          "total_bases_loaded": sum(len(c) for cs in contigs for c in cs), "contigs_parsed": sum(len(cs) for cs in contigs),
          "num_kmers_loaded": sum(len(c) - k + 1 for cs in contigs for c in cs), "num_kmers_novel": len(graph)}
    return graph, st


def child(k, out):
    sys.path.insert(0, ROOT)
    import mccortex_amd as mcx
    from test_gpu_subgraph import arrays
    g = mcx.Graph(k, 1, 1 << 16)
    st = g.add_reads(0, *arrays(case(k))).as_dict()
    g.sync()
    dev = g.device_stats().as_dict()
    st.update({n: dev[n] for n in STATS[2:]})
    res = {"stats": {n: st[n] for n in STATS}, "body": g.export(True).hex(), "nkmers": int(g.nkmers)}
    g.close()
    json.dump(res, open(out, "w"))


def run_child(k, out, packed):
    env = dict(os.environ, MCX_STAGE_BYTES=str(CHUNK))
    env.pop("MCX_PACKED", None)
    if not packed:
        env["MCX_PACKED"] = "0"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(k), str(out)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return json.load(open(out))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 127])
def test_ascii_reads_over_small_staging_chunks(mcx, tmp_path, k):
    reads = case(k)
    assert sum(len(s) + 1 for s in reads) > 4 * CHUNK and max(len(s) for s in reads) > 2 * CHUNK
    assert "N" in max(reads, key=len)
    graph, est = expected(reads, k)
    assert est["num_bad_reads"] > 0 and est["contigs_parsed"] > est["num_good_reads"] and est["num_kmers_loaded"] > len(graph) > 1000
    ascii_ = run_child(k, tmp_path / "ascii.json", packed=False)
    packed = run_child(k, tmp_path / "packed.json", packed=True)
    for name, res in (("ascii", ascii_), ("packed", packed)):
        print(k, name, res["stats"], est)
        assert res["stats"] == est, name
        assert res["nkmers"] == len(graph) and res["body"] == R.pack(graph, k, 1).hex(), name
    assert ascii_ == packed


if __name__ == "__main__":
    child(int(sys.argv[1]), sys.argv[2])
