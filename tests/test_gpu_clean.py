"""`clean` on the MI355X (Graph.unitig_stats / Graph.clean, csrc/mcx_clean.h) against the CPU restatement in
clean_restate.py: the cleaned records byte for byte (sorted), the six removal counters, the "before" and
"after" histograms, the table's k-mer count and checksum.  Graphs come from sequences built on the device:
random genomes read with errors (tips, bubbles), closed cycles, hairpins, self-loops, branches, a chain of
more than 100 K k-mers, and saturated coverage loaded as records."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

BASES = "ACGT"


def rseq(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def mutate(rng, s, err):
    return "".join(rng.choice(BASES) if rng.random() < err else ch for ch in s)


def features(rng, k):
    """sequences whose graphs hold a closed cycle, a hairpin, a self-loop and a branch"""
    cyc = rseq(rng, 3 * k)
    half = rseq(rng, (k + 1) // 2)
    pal = half + rc(half)  # a (k+1)-mer equal to its reverse complement: B -> B' (a hairpin)
    stem = rseq(rng, 2 * k)
    return [cyc + cyc[:k], rseq(rng, k) + pal + rseq(rng, k), "A" * (2 * k), stem + rseq(rng, k), stem + rseq(rng, k)]


def sample(rng, k, ncols, genome_len, nreads, readlen, err):
    genome = rseq(rng, genome_len)
    cols = []
    for c in range(ncols):
        seqs = []
        for _ in range(nreads):
            p = rng.randrange(0, max(1, genome_len - readlen))
            r = mutate(rng, genome[p:p + readlen], err)
            seqs.append(rc(r) if rng.random() < 0.5 else r)
        seqs += features(rng, k) * (c + 1)
        cols.append(seqs)
    return cols


def load(k, ncols, cols, cap=1 << 16):
    g = mcx.Graph(k, ncols, cap)
    for c, seqs in enumerate(cols):
        if not seqs:
            continue
        bases = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        g.add_reads(c, bases, offs)
    g.sync()
    return g


def check(g, k, ncols, threshold, tips):
    body = g.export(True)
    graph = R.parse(body, k, ncols)
    exp, est, ebefore, eafter = R.clean(graph, k, threshold, tips)
    before = g.unitig_stats()
    st, after = g.clean(threshold, tips)
    for name in ("kmer_covg", "unitig_covg", "unitig_len"):
        assert before[name].tolist() == ebefore[name], "before " + name
        assert after[name].tolist() == eafter[name], "after " + name
    for key, v in est.items():
        assert st[key] == v, key
    assert st["nkmers_before"] == len(graph) and st["nkmers_removed"] == len(graph) - len(exp)
    out = g.export(True)
    assert out == R.pack(exp, k, ncols)
    assert g.nkmers == len(exp)
    cs, n = g.checksum()
    assert n == len(exp) and cs == mcx.records_checksum(out, k, ncols)
    # unsorted export: the same records
    rs = 8 * ((2 * k + 63) // 64) + 5 * ncols
    un = g.export(False)
    assert sorted(un[i:i + rs] for i in range(0, len(un), rs)) == sorted(out[i:i + rs] for i in range(0, len(out), rs))
    return st


@pytest.mark.parametrize("k,ncols", [(3, 1), (5, 2), (21, 3), (31, 1), (33, 2), (63, 1), (65, 3), (95, 1), (127, 2)])
def test_random_graphs(k, ncols):
    rng = random.Random(k * 10 + ncols)
    cols = sample(rng, k, ncols, 400 + 20 * k, 60, 2 * k + 20, 0.01)
    for threshold, tips in ((2, 2 * k), (0, 2 * k), (3, 0), (0, 0)):
        g = load(k, ncols, cols)
        check(g, k, ncols, threshold, tips)
        g.close()


def test_reads_with_errors_1e5_kmers():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import synth
    bases, offs = synth.reads(20000, 100, genome_len=60000, seed=11, err=0.004, n_frac=0.0)
    g = mcx.Graph(31, 1, 1 << 19)
    g.add_reads(0, bases, offs)
    g.sync()
    st = check(g, 31, 1, 4, 62)
    assert st["num_tips"] + st["num_low_covg_unitigs"] + st["num_tip_and_low_unitigs"] > 100
    g.close()


def test_long_chain_and_grid():
    rng = random.Random(5)
    cols = [[rseq(rng, 120000)] + features(rng, 31)]
    for grid in (0, 1, 3, 8):
        g = load(31, 1, cols, cap=1 << 18)
        g.configure("grid", grid)
        st = check(g, 31, 1, 2, 62)
        assert st["nkmers_before"] > 100000
        g.close()


def test_saturated_coverage():
    rng = random.Random(9)
    k, ncols = 21, 2
    cols = sample(rng, k, ncols, 600, 40, 60, 0.01)
    g = load(k, ncols, cols)
    body = bytearray(g.export(True))
    g.close()
    rs = 8 + 5 * ncols
    for i in range(0, len(body), rs * 3):  # every third record: both colours near 2^32
        body[i + 8:i + 16] = np.array([2**32 - 5, 2**32 - 1], dtype=np.uint32).tobytes()
    g = mcx.Graph(k, ncols, 1 << 16)
    g.add_records(bytes(body), ncols, [(0, 0), (1, 1)])
    g.sync()
    check(g, k, ncols, 3, 2 * k)
    g.close()


def test_refusals():
    g = mcx.Graph(31, 2, 1 << 16)
    g.configure("intersect", 1)
    with pytest.raises(Exception, match="intersect"):
        g.unitig_stats()
    with pytest.raises(Exception, match="intersect"):
        g.clean(2, 62)
    g.close()
    g = mcx.Graph(31, 1, 1 << 16, nparts=2, part=0)
    with pytest.raises(Exception, match="split over devices"):
        g.unitig_stats()
    g.close()


def test_empty_graph():
    g = mcx.Graph(31, 1, 1 << 16)
    before = g.unitig_stats()
    assert all(int(v.sum()) == 0 for v in before.values())
    st, _ = g.clean(2, 62)
    assert st["nkmers_before"] == 0 and st["nkmers_removed"] == 0
    g.close()


def test_decomposition_paths_and_staleness():
    rng = random.Random(21)
    k = 31
    cols = sample(rng, k, 1, 2000, 80, 90, 0.01)
    # clean() without unitig_stats() first: it computes the decomposition itself
    g = load(k, 1, cols)
    graph = R.parse(g.export(True), k, 1)
    exp, est, _, eafter = R.clean(graph, k, 2, 2 * k)
    st, after = g.clean(2, 2 * k)
    assert g.export(True) == R.pack(exp, k, 1) and after["unitig_len"].tolist() == eafter["unitig_len"]
    # a second clean of the cleaned graph (tombstones in the table) is a clean of that graph
    check(g, k, 1, 3, 2 * k)
    g.close()
    # the graph changes between the two calls without changing its k-mer count: the decomposition is redone
    g = load(k, 1, cols)
    g.unitig_stats()
    more = [s for s in cols[0][:40]]
    bases = np.frombuffer("".join(more).encode(), dtype=np.uint8)
    offs = np.zeros(len(more) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in more])
    n0 = g.nkmers
    g.add_reads(0, bases, offs)
    g.sync()
    assert g.nkmers == n0
    graph = R.parse(g.export(True), k, 1)
    exp, est, _, _ = R.clean(graph, k, 2, 2 * k)
    st, _ = g.clean(2, 2 * k)
    for key, v in est.items():
        assert st[key] == v, key
    assert g.export(True) == R.pack(exp, k, 1)
    g.close()


def test_table_at_95_percent_load():
    k = 31
    probe = mcx.Graph(k, 1, 1 << 14)
    slots = probe.capacity()[0] * 32 // 33  # (the hash-addressed slots; the overflow area is 1/32 on top)
    probe.close()
    rng = random.Random(33)
    genome = rseq(rng, int(slots * 0.95) + k - 1)
    seqs = [genome[i:i + 80 + k] for i in range(0, len(genome) - k, 80)]
    g = load(k, 1, [seqs], cap=1 << 14)
    assert g.nkmers >= 0.94 * slots  # sub-tables this full spill keys into the overflow area
    check(g, k, 1, 2, 2 * k)
    g.close()


# ---- the command line: the reference's tests/clean_graph/clean{1,2,4} as command lines -------------------------
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mccortex_amd", "bin")


def cli(maxk, *args):
    import subprocess
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stderr.decode(errors="replace")


def ctx_body(path, k, ncols):
    from oracle import ctxio
    buf = open(path, "rb").read()
    hdr, size = ctxio.read_header(buf)
    assert hdr["kmer_size"] == k and hdr["num_cols"] == ncols
    return hdr, buf[size:]


def build_ctx(tmp, maxk, k, samples, name):
    """`build --sort` with one --sample per entry of samples: [(name, [sequences])]"""
    args = ["build", "-q", "-k", k, "--sort"]
    for i, (sname, seqs) in enumerate(samples):
        fa = tmp / ("%s.%d.fa" % (name, i))
        fa.write_text("".join(">r%d\n%s\n" % (j, s) for j, s in enumerate(seqs)))
        args += ["--sample", sname, "--seq", fa]
    out = tmp / (name + ".raw.ctx")
    cli(maxk, *args, out)
    return out


def replay(tmp, maxk, k, samples, name, clean_args, threshold, tips, csv=False):
    raw = build_ctx(tmp, maxk, k, samples, name)
    ncols = len(samples)
    _, body = ctx_body(raw, k, ncols)
    graph = R.parse(body, k, ncols)
    exp, _, before, after = R.clean(graph, k, threshold, tips)
    out = tmp / (name + ".clean.ctx")
    extra = []
    if csv:
        extra = ["--covg-before", tmp / "cb.csv", "--covg-after", tmp / "ca.csv", "--len-before", tmp / "lb.csv",
                 "--len-after", tmp / "la.csv"]
    err = cli(maxk, "clean", *clean_args, *extra, "--sort", "-o", out, raw)
    hdr, got = ctx_body(out, k, ncols)
    assert got == R.pack(exp, k, ncols)
    if "-q" not in clean_args:
        assert "Removed %s of %s" % (format(len(graph) - len(exp), ","), format(len(graph), ",")) in err
    if csv:
        assert (tmp / "cb.csv").read_text() == R.covg_csv(before["kmer_covg"], before["unitig_covg"])
        assert (tmp / "lb.csv").read_text() == R.len_csv(before["unitig_len"], k)
        assert (tmp / "ca.csv").read_text() == R.covg_csv(after["kmer_covg"], after["unitig_covg"])
        assert (tmp / "la.csv").read_text() == R.len_csv(after["unitig_len"], k)
    return hdr, exp, graph


def test_cli_clean1_clean2_clean4(tmp_path):
    seq1 = ["ACACAGAGAGTCCCT", "ACACAGAGAGTCACTCCCC", "ACACAGAGAGTCACTCCCC", "ACACAGAGACTCACTCCCC", "ACACAGAGACTCACTCCCC"]
    hdr, _, _ = replay(tmp_path, 31, 9, [("SeqJr", seq1)], "clean1", ["-q", "--unitigs=2", "--tips=62"], 2, 62, csv=True)
    c = hdr["ginfo"][0]["cleaning"] if isinstance(hdr["ginfo"][0], dict) else hdr["ginfo"][0].cleaning
    get = (lambda n: c[n]) if isinstance(c, dict) else (lambda n: getattr(c, n))
    assert get("cleaned_tips") and get("cleaned_unitigs") and get("clean_unitigs_thresh") == 2
    rep = "CAAAGGCCTCACGGGTA"
    seq2 = ["GTGAGGCCAAGCAAAGGCCTCACGGGTACAAAGGCCTCACGGGTAGAATCCCCTTTG"] + ["GTGAGGCCAAGCAAAGGCCTCACGGGTAGAATCCCCTTTG"] * 2 + \
           ["AAAAAAAAAAAAAAAAATAAAAAAAAAAAAAAAAA"]
    assert rep in seq2[0]
    # --unitigs=2 alone still clips tips shorter than 2k (ctx_clean.c passes min_keep_tip = 2k to clean_graph)
    hdr, _, _ = replay(tmp_path, 31, 17, [("SeqJr", seq2)], "clean2", ["--unitigs=2"], 2, 34)
    c = hdr["ginfo"][0]["cleaning"] if isinstance(hdr["ginfo"][0], dict) else hdr["ginfo"][0].cleaning
    get = (lambda n: c[n]) if isinstance(c, dict) else (lambda n: getattr(c, n))
    assert not get("cleaned_tips") and get("cleaned_unitigs")
    s = "GCTTCTTATTTGGCATAATCCAACTTCCCTACGGAAGCCCAATAGGATTAAATTGAAGCT"
    _, exp, _ = replay(tmp_path, 31, 31, [("sample1", ["A"]), ("sample2", [s])], "pop2", ["-q", "-m", "1M", "--unitigs=2", "--tips=0"], 2, 0)
    assert exp == {}
    _, exp, graph = replay(tmp_path, 31, 31, [("sample1", ["A"]), ("sample2", [s]), ("sample2", [s])], "pop3",
                           ["-q", "-m", "1M", "--unitigs=2", "--tips=0"], 2, 0)
    assert set(exp) == set(graph)
    out = tmp_path / "pop3b.clean.ctx"
    cli(31, "clean", "-q", "-m", "1M", "--unitigs=2", "--tips=0", "-o", out, str(tmp_path / "pop3.raw.ctx") + ":0,1")
    assert ctx_body(out, 31, 2)[1] == b""


def test_cli_k99_auto_threshold_fallback_and_stats_only(tmp_path):
    import synth
    bases, offs = synth.reads(3000, 150, genome_len=20000, seed=4, err=0.004, n_frac=0.0)
    seqs = [bytes(bases[int(offs[i]):int(offs[i + 1])]).decode() for i in range(len(offs) - 1)]
    for maxk, k in ((127, 99), (31, 31)):
        raw = build_ctx(tmp_path, maxk, k, [("s", seqs)], "r%d" % k)
        graph = R.parse(ctx_body(raw, k, 1)[1], k, 1)
        before = R.hists(graph, R.unitigs(graph, k))
        est = R.pick_threshold(before["kmer_covg"])
        thr = 7 if est < 7 else est  # --fallback 7 wins whenever the estimate is missing or lower
        exp, _, _, _ = R.clean(graph, k, thr, 2 * k)
        out = tmp_path / ("c%d.ctx" % k)
        err = cli(maxk, "clean", "--fallback", 7, "--sort", "-o", out, raw)
        assert ctx_body(out, k, 1)[1] == R.pack(exp, k, 1)
        assert ("Recommended cleaning threshold is: %d" % est) in err if est >= 0 else "Cannot find recommended" in err
        # stats only: no output graph, the "before" CSVs of the flattened graph
        cli(maxk, "clean", "--fallback", 7, "-c", tmp_path / "s.csv", "-l", tmp_path / "l.csv", raw)
        assert (tmp_path / "s.csv").read_text() == R.covg_csv(before["kmer_covg"], before["unitig_covg"])
        assert (tmp_path / "l.csv").read_text() == R.len_csv(before["unitig_len"], k)
