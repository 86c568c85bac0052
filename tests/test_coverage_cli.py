"""`mccortex<K> coverage`: the command-line contract of src/commands/ctx_coverage.c, and a replay of the reference's
tests/coverage (golden/coverage.json) on the device, compared byte for byte with coverage_restate.py."""
import gzip
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import coverage_restate as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
G31, G5 = os.path.join(GOLD, "tiny_k31.ctx"), os.path.join(GOLD, "tiny_k5.ctx")
CASE = json.load(open(os.path.join(GOLD, "coverage.json")))
K = CASE["k"]


def run(maxk, *args, stdin=None):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, input=stdin, timeout=300)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63, 95, 127):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


@pytest.fixture()
def fa(tmp_path):
    p = tmp_path / "in.fa"
    p.write_text(">a\nACAATGCAGCATT\n")
    return str(p)


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_help_and_dispatcher(built, maxk):
    for args in (["coverage", "-h"], ["coverage"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d coverage [options] <in.ctx> [in2.ctx ..]" % maxk in err
        assert "Print contig coverage" in err
        for opt in ("-h, --help           This help message", "-q, --quiet          Silence status output normally printed to STDERR",
                    "-f, --force          Overwrite output files", "-m, --memory <mem>   Memory to use (e.g. 1M, 20GB)",
                    "-n, --nkmers <N>     Number of hash table entries (e.g. 1G ~ 1 billion)",
                    "-e, --edges          Print edges as well. Uses hex encoding [TGCA|TGCA].",
                    "-E, --degree         Print edge degree: 00. 01/ 02[ 10\\ 11- 12{ 20] 21} 22X",
                    "-s, --seq <in>       Sequence file to get coverages for (can specify multiple times)",
                    "-o, --out <out.txt>  Save output [default: STDOUT]", "--device <N>"):
            assert opt in err, opt
        assert "not part of this build" not in err
    # the dispatcher knows the command; its own usage text and its list of commands are pinned by the transcripts of
    # tests/golden/cli_transcripts.json and stay as recorded
    rc, _, err = run(maxk, "coverage", "--nosuchoption")
    assert rc != 0 and "not part of this build" not in err and "coverage -h` for help. Bad option: --nosuchoption" in err


def test_argument_errors(built, tmp_path, fa):
    missing = str(tmp_path / "missing.fa")
    cases = [
        ([G31], "Require at least one --seq file"),
        (["--seq", fa], "Require input graph files (.ctx)"),
        (["-1", fa], "Require input graph files (.ctx)"),
        (["--seq", missing, G31], "Cannot read --seq file %s" % missing),
        (["-s", missing, G31], "Cannot read --seq file %s" % missing),
        (["-1", missing, G31], "Cannot read --seq file %s" % missing),
        (["-1", fa, "-f", "-f", G31], "-f, --force given twice"),
        (["-1", fa, "-e", "--edges", G31], "-e, --edges given twice"),
        (["-1", fa, "-E", "--degree", G31], "-E, --degrees given twice"),
        (["-1", fa, "-o", "a", "--out", "b", G31], "-o, --out given twice"),
        (["-1", fa, "-m", "1G", "-m", "1G", G31], "-m, --memory <M> specifed more than once"),
        (["-1", fa, "-n", "1M", "-n", "1M", G31], "-n, --nkmers <N> specifed more than once"),
        (["-1", fa, "-n", "banana", G31], "Invalid hash size: banana"),
        (["-1", fa, "--device", "x", G31], "--device requires an int x >= 0: x"),
        (["-1", fa, "--nosuchoption", G31], "coverage -h` for help. Bad option: --nosuchoption"),
        (["-1", fa, str(tmp_path / "missing.ctx")], "missing.ctx"),
        (["-1", fa, G31, G5], "Kmer sizes don't match [31 vs 5]"),
    ]
    for args, msg in cases:
        rc, out, err = run(31, "coverage", *args)
        assert rc != 0 and msg in err and out == b"", (args, err)
        assert sorted(os.listdir(tmp_path)) == ["in.fa"], args  # nothing was created


# ---- on the device ---------------------------------------------------------------------------------------------------
def fasta(reads):
    return "".join(">%s\n%s\n" % (n, s) for n, s in reads)


FLAGS = {"plain": [], "e": ["-e"], "E": ["-E"], "eE": ["--edges", "--degree"]}


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    """the files of the reference's tests/coverage, the graph built by this repository's own `build`"""
    d = tmp_path_factory.mktemp("coverage")
    (d / "seq.fa").write_text(fasta(CASE["seq_fa"]))
    (d / "rnd.fa").write_text(fasta(CASE["rnd_fa"]))
    ctx = d / "seq.k5.ctx"
    rc, _, err = run(31, "build", "-q", "-k", K, "--sample", "Wallace", "--sample", "Gromit", "--seq", d / "seq.fa",
                     "--sample", "Trousers", "--seq", d / "seq.fa", "--seq2", "%s:%s" % (d / "seq.fa", d / "seq.fa"), ctx)
    assert rc == 0, err
    seqs = [s for _, s in CASE["seq_fa"]]
    graph = R.build([[], seqs, seqs * 3], K)
    reads = [tuple(r) for r in CASE["rnd_fa"] + CASE["seq_fa"]]
    return d, ctx, graph, reads


@pytest.mark.gpu
def test_reference_k5(case):
    d, ctx, graph, reads = case
    for name, flags in FLAGS.items():
        rc, out, err = run(31, "coverage", *flags, "--seq", d / "rnd.fa", "-1", d / "seq.fa", ctx)
        assert rc == 0, err
        e, deg = name in ("e", "eE"), name in ("E", "eE")
        assert out.decode() == V.command_text(graph, K, 3, reads, e, deg) == CASE["expected"][name], name
        assert "Reading coverage..." in err and "Printed graph coverage for 3 reads" in err
    # the lines worked out by hand, in the device's output
    for line_name, line in CASE["by_hand"]["lines"].items():
        assert (">%s\n%s\n" % (line_name, line)).encode() in out
    rc, out, err = run(31, "coverage", "-q", "-e", "-s", d / "seq.fa", ctx)
    assert rc == 0 and err == "" and out.decode() == V.command_text(graph, K, 3, reads[2:], True, False)


@pytest.mark.gpu
def test_out_file_and_force(case):
    d, ctx, graph, reads = case
    o = d / "coverage.txt"
    want = V.command_text(graph, K, 3, reads, True, True)
    rc, out, err = run(31, "coverage", "-e", "-E", "-o", o, "--seq", d / "rnd.fa", "-1", d / "seq.fa", ctx)
    assert rc == 0 and out == b"" and o.read_text() == want, err
    o.write_text("keep")
    rc, out, err = run(31, "coverage", "-o", o, "--seq", d / "rnd.fa", ctx)
    assert rc != 0 and out == b"" and "File already exists: %s" % o in err and o.read_text() == "keep"
    rc, out, err = run(31, "coverage", "-f", "--out", o, "--seq", d / "rnd.fa", ctx)
    assert rc == 0 and out == b"" and o.read_text() == V.command_text(graph, K, 3, reads[:2]), err


@pytest.mark.gpu
def test_stacked_graphs_and_colour_filter(case):
    d, ctx, graph, reads = case
    # two files: the colours of the second follow those of the first (3 + 3)
    g6 = {key: (cv + cv, ed + ed) for key, (cv, ed) in graph.items()}
    rc, out, err = run(31, "coverage", "-e", "-E", "-1", d / "rnd.fa", ctx, ctx)
    assert rc == 0 and out.decode() == V.command_text(g6, K, 6, reads[:2], True, True), err
    # in.ctx:1 loads colour 1 alone, as colour 0
    g1 = {key: ((cv[1],), [ed[1]]) for key, (cv, ed) in graph.items()}
    rc, out, err = run(31, "coverage", "-e", "-1", d / "rnd.fa", "-1", d / "seq.fa", "%s:1" % ctx)
    assert rc == 0 and out.decode() == V.command_text(g1, K, 1, reads, True, False), err
    # a filter and a whole file: colour 2 of the first, then the three of the second
    g4 = {key: ((cv[2],) + cv, [ed[2]] + ed) for key, (cv, ed) in graph.items()}
    rc, out, err = run(31, "coverage", "-E", "-1", d / "seq.fa", "%s:2" % ctx, ctx)
    assert rc == 0 and out.decode() == V.command_text(g4, K, 4, reads[2:], False, True), err


@pytest.mark.gpu
def test_fasta_fastq_plain_and_gz(case):
    """the sequence is printed as read (case and N kept); plain input has empty names"""
    d, ctx, graph, reads = case
    seq = CASE["seq_fa"][0][1]
    rd = [("low er", seq[:20].lower()), ("n", seq[3:12] + "N" + seq[13:30]), ("short", "ACG"), ("empty", "")]
    (d / "r.fq").write_text("".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in rd))
    (d / "r.txt").write_text("".join(s + "\n" for _, s in rd[:3]))
    with gzip.open(d / "r.fa.gz", "wb") as f:
        f.write(fasta(rd).encode())
    rc, out, err = run(31, "coverage", "-e", "-E", "-1", d / "r.fq", ctx)
    assert rc == 0 and out.decode() == V.command_text(graph, K, 3, rd, True, True), err
    assert ">short\nACG\n>short_c0_edges\n\n>short_c0_degree\n\n>short_c0_covgs\n\n" in out.decode()
    rc, out2, err = run(31, "coverage", "-e", "-E", "-1", d / "r.fa.gz", ctx)
    assert rc == 0 and out2 == out, err
    rc, out, err = run(31, "coverage", "-1", d / "r.txt", ctx)
    assert rc == 0 and out.decode() == V.command_text(graph, K, 3, [("", s) for _, s in rd[:3]]), err
    # files in command-line order, reads in file order
    rc, out, err = run(31, "coverage", "-1", d / "r.txt", "--seq", d / "r.fq", ctx)
    assert rc == 0 and out.decode() == V.command_text(graph, K, 3, [("", s) for _, s in rd[:3]] + rd), err
    assert "Printed graph coverage for 7 reads" in err


@pytest.mark.gpu
def test_tiny_k31(built):
    """golden/tiny_k31.ctx (two colours, made of tiny_k31.colour0.txt and tiny_k31.colour1.txt, which hold lower case
    and N): the graph is the file's own records, the reads are the first three, the first two with lower case and the first with an N of each text file, as plain input"""
    sys.path.insert(0, ROOT)
    from oracle import ctxio
    buf = open(G31, "rb").read()
    hdr, hdr_size = ctxio.read_header(buf)
    keys, covgs, edges = ctxio.records(buf, hdr, hdr_size)
    assert hdr["num_cols"] == 2 and keys.shape[1] == 1 and len(keys) > 3000
    graph = {int(keys[i, 0]): (tuple(int(x) for x in covgs[i]), [int(x) for x in edges[i]]) for i in range(len(keys))}
    per = [open(os.path.join(GOLD, "tiny_k31.colour%d.txt" % c)).read().split() for c in (0, 1)]
    reads = [("", s) for p in per for s in p[:3] + [x for x in p if x != x.upper()][:2] + [x for x in p if "N" in x][:1]]
    assert len(reads) == 12 and any(ch.islower() for _, s in reads for ch in s) and any("N" in s for _, s in reads)
    rc, out, err = run(31, "coverage", "-e", "-E", "-1", "-", G31, stdin="".join(s + "\n" for _, s in reads).encode())
    assert rc == 0 and "Printed graph coverage for 12 reads" in err, err
    assert out.decode() == V.command_text(graph, 31, 2, reads, True, True)
