"""`unitigs` on the MI355X (Graph.unitigs, csrc/mcx_unitigs.h, `mccortex<K> unitigs`) against the CPU restatement in
unitigs_restate.py: the FASTA, GFA and DOT text byte for byte.  Graphs come from sequences built on the device, as in
test_gpu_clean.py: random genomes read with errors, closed cycles, hairpins, self-loops, branches, a chain of more
than 100 K k-mers, a closed cycle of more than 10 K k-mers, a table at 95 % load."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import unitigs_restate as U  # noqa: E402
import mccortex_amd as mcx  # noqa: E402
from test_gpu_clean import features, load, rc, rseq, sample  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = ("fasta", "gfa", "dot")
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mccortex_amd", "bin")


def expected(g, k, ncols):
    graph = R.parse(g.export(True), k, ncols)
    return graph, {f: U.text(graph, k, f) for f in FORMATS}


def check(g, k, ncols, formats=FORMATS):
    graph, exp = expected(g, k, ncols)
    for f in formats:
        st = {}
        got = g.unitigs(f, stats=st)
        assert got == exp[f], "%s k=%d: first difference at byte %d" % (
            f, k, next((i for i, (a, b) in enumerate(zip(got, exp[f])) if a != b), min(len(got), len(exp[f]))))
        assert st["num_kmers"] == len(graph) and st["num_bytes"] == len(got)
        assert st["num_unitigs"] == exp["fasta"].count(b">")
    return graph, exp


@pytest.mark.parametrize("k,ncols", [(3, 1), (5, 2), (7, 1), (21, 3), (31, 1), (33, 2), (63, 1), (65, 3), (95, 1), (97, 1), (127, 2)])
def test_random_graphs(k, ncols):
    rng = random.Random(k * 10 + ncols)
    cols = sample(rng, k, ncols, 400 + 20 * k, 60, 2 * k + 20, 0.01)
    g = load(k, ncols, cols)
    graph, exp = check(g, k, ncols)
    us = U.unitigs(graph, k)
    st = {}
    g.unitigs("dot", points=True, stats=st)
    assert g.unitigs("dot", points=True) == U.text(graph, k, "dot", points=True)
    assert st["num_cycles"] == sum(1 for u in us if U.is_cycle(graph, u, k))
    g.close()


def test_union_of_colours_decides_the_unitigs():
    # colour 0 alone is one chain; colour 1 adds a branch in its middle: the union splits it
    rng = random.Random(2)
    k = 31
    a = rseq(rng, 200)
    cols = [[a], [a[80:80 + k] + rseq(rng, 40)]]
    g = load(k, 2, cols)
    graph, exp = check(g, k, 2)
    alone = R.build([cols[0]], k)
    assert len(U.unitigs(alone, k)) == 1 and len(U.unitigs(graph, k)) > 2
    g.close()


@pytest.mark.parametrize("k", [5, 31, 63, 95, 127])
def test_feature_graphs(k):
    rng = random.Random(k)
    g = load(k, 1, [features(rng, k)])
    graph, exp = check(g, k, 1)
    us = U.unitigs(graph, k)
    assert any(U.is_cycle(graph, u, k) for u in us)
    assert exp["gfa"].count(b"L\t") >= 3
    g.close()


def test_long_chain_and_grid():
    rng = random.Random(5)
    cols = [[rseq(rng, 120000)] + features(rng, 31)]
    texts = []
    for grid in (0, 1, 3, 8):
        g = load(31, 1, cols, cap=1 << 18)
        g.configure("grid", grid)
        graph, exp = check(g, 31, 1)
        assert max(len(u) for u in U.unitigs(graph, 31)) > 100000
        texts.append(exp)
        g.close()
    assert all(t == texts[0] for t in texts)


def test_long_closed_cycle():
    rng = random.Random(6)
    k = 31
    cyc = rseq(rng, 12000)
    g = load(k, 1, [[cyc + cyc[:k]]], cap=1 << 16)
    graph, exp = check(g, k, 1)
    us = U.unitigs(graph, k)
    assert len(us) == 1 and len(us[0]) == 12000 and U.is_cycle(graph, us[0], k)
    g.close()
    # the same cycle in its other strand and entered elsewhere: the same text
    g = load(k, 1, [[rc(cyc[5000:] + cyc[:5000 + k])]], cap=1 << 16)
    for f in FORMATS:
        assert g.unitigs(f) == exp[f]
    g.close()


def test_table_at_95_percent_load():
    k = 31
    probe = mcx.Graph(k, 1, 1 << 14)
    slots = probe.capacity()[0] * 32 // 33
    probe.close()
    rng = random.Random(33)
    genome = rseq(rng, int(slots * 0.95) + k - 1)
    seqs = [genome[i:i + 80 + k] for i in range(0, len(genome) - k, 80)]
    g = load(k, 1, [seqs], cap=1 << 14)
    assert g.nkmers >= 0.94 * slots
    check(g, k, 1)
    g.close()


def test_table_size_and_input_order_do_not_matter():
    rng = random.Random(8)
    k = 33
    cols = sample(rng, k, 1, 1500, 60, 100, 0.01)
    texts = []
    for cap, seqs in ((1 << 14, cols[0]), (1 << 18, cols[0]), (1 << 14, cols[0][::-1])):
        g = load(k, 1, [seqs], cap=cap)
        texts.append({f: g.unitigs(f) for f in FORMATS})
        if len(texts) == 1:
            check(g, k, 1)
        g.close()
    assert texts[0] == texts[1] == texts[2]


@pytest.mark.parametrize("chunk", [1, 7, 16, 33, 100, 4096])
def test_chunk_seams(chunk):
    rng = random.Random(12)
    k = 21
    cols = sample(rng, k, 1, 500, 30, 70, 0.02)
    g = load(k, 1, cols)
    graph, exp = expected(g, k, 1)
    g.configure("unitigs_chunk", chunk)
    for f in FORMATS if chunk > 1 else ("gfa",):
        parts = list(g.unitigs_chunks(f))
        assert all(len(p) == chunk for p in parts[:-1]) and 0 < len(parts[-1]) <= chunk
        assert b"".join(parts) == exp[f]
    g.close()


def test_stale_decomposition_is_redone_and_clean_then_unitigs():
    rng = random.Random(21)
    k = 31
    cols = sample(rng, k, 1, 2000, 80, 90, 0.01)
    g = load(k, 1, cols)
    g.unitig_stats()
    check(g, k, 1, ("fasta",))  # the cached decomposition is used
    # new edges, same k-mers: a chain read again with a jump in it
    s = cols[0][0]
    more = [s[:40] + s[50:]] if len(s) > 60 + k else [s]
    extra = [cols[0][1][:k] + cols[0][2][-k:]]
    bases = np.frombuffer("".join(more + extra).encode(), dtype=np.uint8)
    offs = np.zeros(len(more + extra) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in more + extra])
    before = g.unitigs("gfa")
    g.add_reads(0, bases, offs)
    g.sync()
    graph, exp = check(g, k, 1)
    assert exp["gfa"] != before
    # clean, then unitigs of what is left, on the same handle
    g.clean(2, 2 * k)
    graph2, exp2 = check(g, k, 1)
    assert len(graph2) < len(graph)
    g.close()


def test_dev_arrays_against_restatement():
    rng = random.Random(17)
    for k in (5, 31, 65, 127):
        g = load(k, 1, [sample(rng, k, 1, 800, 40, 2 * k + 30, 0.01)[0]])
        graph = R.parse(g.export(True), k, 1)
        us = U.unitigs(graph, k)
        t, st = g.unitigs_dev()
        a = {name: v.cpu().numpy() for name, v in t.items()}
        assert st["num_kmers"] == len(graph) and st["num_unitigs"] == len(us)
        keys = []
        for row in a["keys"].view(np.uint64).reshape(-1, g.W):
            x = 0
            for w in row:
                x = (x << 64) | int(w)
            keys.append(x)
        assert sorted(keys) == sorted(graph)
        at = {key: i for i, key in enumerate(keys)}
        for j, u in enumerate(us):
            assert int(a["first"][j]) == at[u[0][0]] and int(a["length"][j]) == len(u)
            for r, (key, o) in enumerate(u):
                i = at[key]
                assert (int(a["unitig"][i]), int(a["rank"][i]), int(a["orient"][i])) == (j, r, o)
        g.close()


def test_refusals_and_empty_graph():
    g = mcx.Graph(31, 2, 1 << 16)
    g.configure("intersect", 1)
    with pytest.raises(Exception, match="intersect"):
        g.unitigs()
    g.close()
    g = mcx.Graph(31, 1, 1 << 16, nparts=2, part=0)
    with pytest.raises(Exception, match="split over devices"):
        g.unitigs("gfa")
    g.close()
    g = mcx.Graph(31, 1, 1 << 16)
    with pytest.raises(ValueError):
        g.unitigs("fastq")
    assert g.unitigs("fasta") == b"" and g.unitigs("gfa") == b"H\tVN:Z:1.0\n"
    assert g.unitigs("dot") == U.text({}, 31, "dot")
    g.close()


# ---- the command line: the three of the reference's tests/unitigs/Makefile, on a fixed sequence ---------------------
SEQ = ("ACGTTGCATGCCGATAGGCTAAGCTTCCGATCGGATATCGCGTTAACCGGTTAGCATCGATCGGCTAGCTAGGATCCGATTGCAAGCTTGGCCATATGCGCGATATCG"
       "TAGCTAGCATGCATCGTAGCTAGGCTAGGATCGATCGTTAGGCCAATTGGCCTAGGATCCTAGGCATGCTAGCTAGGCTTAGGCCTAAGGCT")


def cli(maxk, *args, **kw):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, **kw)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stdout, p.stderr.decode(errors="replace")


def test_cli_three_formats(tmp_path):
    assert len(SEQ) == 200
    k = 7
    fa = tmp_path / "seq.fa"
    fa.write_text(">s\n%s\n" % SEQ)
    ctx = tmp_path / "seq.k7.ctx"
    cli(31, "build", "-q", "-m", "1M", "-k", k, "--sample", "MsSample", "--seq", fa, ctx)
    graph = R.build([[SEQ]], k)
    n = len(U.unitigs(graph, k))
    # unitigs -m 1M seq.ctx > out.fa ; unitigs -m 1M --dot seq.ctx > out.dot ; unitigs -m 1M --gfa seq.ctx > out.gfa
    for opts, f in (([], "fasta"), (["--dot"], "dot"), (["--gfa"], "gfa")):
        out, err = cli(31, "unitigs", "-m", "1M", *opts, ctx)
        assert out == U.text(graph, k, f), f
        assert "Dumped %s unitigs" % format(n, ",") in err and "format to STDOUT" in err
    out, err = cli(31, "unitigs", "-q", "-m", "1M", "--dot", "--points", "-t", 3, "-o", tmp_path / "o.dot", ctx)
    assert out == b"" and "Dumped" not in err
    assert (tmp_path / "o.dot").read_bytes() == U.text(graph, k, "dot", points=True)
    # two files (one of them twice, with a colour filter) in either order: the union, the same bytes
    rng = random.Random(3)
    other = rseq(rng, 60) + SEQ[50:90] + rseq(rng, 60)
    fb = tmp_path / "b.fa"
    fb.write_text(">s\n%s\n" % other)
    ctxb = tmp_path / "b.k7.ctx"
    cli(31, "build", "-q", "-m", "1M", "-k", k, "--sample", "B", "--seq", fb, ctxb)
    both = {}
    for key in set(R.build([[SEQ]], k)) | set(R.build([[other]], k)):
        e = 0
        for gr in (R.build([[SEQ]], k), R.build([[other]], k)):
            if key in gr:
                e |= R.union_edges(gr, key)
        both[key] = ((1,), [e])
    for order in ([ctx, str(ctxb) + ":0"], [ctxb, ctx]):
        cli(31, "unitigs", "-q", "-g", "-f", "-o", tmp_path / "u.gfa", *order)
        assert (tmp_path / "u.gfa").read_bytes() == U.text(both, k, "gfa")
    # k > 31 through the wide binary
    big = rseq(rng, 400)
    fc = tmp_path / "c.fa"
    fc.write_text(">s\n%s\n" % big)
    cli(127, "build", "-q", "-k", 99, "--sample", "C", "--seq", fc, tmp_path / "c.ctx")
    out, _ = cli(127, "unitigs", "-q", "--gfa", tmp_path / "c.ctx")
    assert out == U.text(R.build([[big]], 99), 99, "gfa")
