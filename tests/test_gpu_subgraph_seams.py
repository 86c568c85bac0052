"""Graph.subgraph_seed with small staging chunks: MCX_STAGE_BYTES = 1024 makes a staging buffer of 1040 bytes (the
packed layout of mcx_graph_add_reads, the default), so a chunk of seeds holds at most 848 new bytes.  The seeds here
spread over many chunks, straddle their seams, and one is longer than a chunk and goes in pieces; the k-mers that
start in the 128 carried bytes belong to the chunk that carries them.  k = 127 leaves one position of the carry unused.
MCX_STAGE_BYTES is read once per process, so the device part runs in a child process (this file, run as a script)."""
import json
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clean_restate as R  # noqa: E402
import subgraph_restate as S  # noqa: E402

DIST = 3
ROUTES = ("reads", "three")


def case(k):
    """a small graph (loading it goes through the same small chunks), seeds much longer than it"""
    from test_gpu_subgraph import rc, rseq
    rng = random.Random(400 + k)
    genome = rseq(rng, 1300)
    graph = R.build([[genome]], k)
    short = [genome[p:p + k + 59] for p in range(0, 600, 30)]  # 20 seeds of k + 59 bases
    long_ = rseq(rng, 300) + genome[200:700] + "N" + genome[701:1100] + rseq(rng, 500)  # 2100 bases: three pieces
    seeds = short[:10] + [long_] + [rc(s) for s in short[10:]] + ["ACGT", genome[1150:1150 + k].lower()]
    return graph, seeds


def child(k, out):
    sys.path.insert(0, ROOT)
    from test_gpu_subgraph import load_graph, seed_with
    graph, seeds = case(k)
    res = {}
    g, ncols = load_graph(graph, k)
    for how in ROUTES:  # the second route runs on what the first left: the same seeds, on the pruned graph
        g.subgraph_begin()
        seed_with(g, seeds, how)
        st = g.subgraph_finish(DIST)
        res[how] = {"stats": {n: int(v) for n, v in st.items()}, "body": g.export(True).hex(), "nkmers": int(g.nkmers)}
    g.close()
    json.dump(res, open(out, "w"))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 127])
def test_seeds_over_small_staging_chunks(mcx, tmp_path, k):
    graph, seeds = case(k)
    assert sum(len(s) + 1 for s in seeds) > 4 * 848 and max(len(s) for s in seeds) > 2 * 848
    expect = {}
    expect["reads"] = S.subgraph(graph, k, seeds, DIST)
    expect["three"] = S.subgraph(expect["reads"][0], k, seeds, DIST)
    assert 0 < len(expect["reads"][0]) < len(graph) and expect["reads"][1]["num_seed_found"] > 500
    assert expect["reads"][1]["num_seed_kmers"] > expect["reads"][1]["num_seed_found"]  # (some seed k-mers are not in the graph)
    out = tmp_path / "seams.json"
    env = dict(os.environ, MCX_STAGE_BYTES="1024")
    env.pop("MCX_PACKED", None)  # the default layout, whose buffers are the smaller ones
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(k), str(out)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    res = json.load(open(out))
    for how in ROUTES:
        exp, est = expect[how]
        print(k, how, res[how]["stats"], est)
        for name, value in est.items():
            assert res[how]["stats"][name] == value, (how, name)
        assert res[how]["nkmers"] == len(exp) and res[how]["body"] == R.pack(exp, k, 1).hex(), how


if __name__ == "__main__":
    child(int(sys.argv[1]), sys.argv[2])
