"""`mccortex<K> correct`: the command-line contract of src/commands/ctx_correct.c and read_thread_cmd.c without link
files, and a replay of the command lines of the reference's tests/correct (golden/correct.json) on the device, the
decoded .gz compared byte for byte with correct_restate.py."""
import gzip
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_restate as X  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
G31 = os.path.join(GOLD, "tiny_k31.ctx")
CASE = json.load(open(os.path.join(GOLD, "correct.json")))["tests_correct"]
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
def txt(tmp_path):
    p = tmp_path / "in.txt"
    p.write_text("ACAATGCAGCATT\n")
    return str(p)


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_help_and_dispatcher(built, maxk):
    for args in (["correct", "-h"], ["correct"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d correct [options] <input.ctx>" % maxk in err
        assert "Correct reads against a (population) graph. Uses paths if specified." in err
        assert "Bases are printed in lower case if they cannot be corrected." in err
        for opt in ("-p, --paths <in.ctp>     Load link file (can specify multiple times)",
                    "-1, --seq <in:out>       Correct reads (output: <out>.fa.gz)",
                    "-2, --seq2 <in1:in2:out> Correct reads (output: <out>{,.1,.2}.fa.gz)",
                    "-i, --seqi <in.bam:out>  Correct reads (output: <out>{,.1,.2}.fa.gz)",
                    "-F, --format <f>         Output format may be: FASTA or FASTQ",
                    "-w, --one-way            Use one-way gap filling (conservative)",
                    "-W, --two-way            Use two-way gap filling (liberal)",
                    "-D, --gap-diff-coeff <D>   abs(gap_exp - gap_seen) <= gap_exp*D + d",
                    "-Z, --fq-zero <char>     Replace zero'd quality score with character <char>",
                    "-P, --print-orig         Print original sequence in the read name ('orig=SEQ')",
                    "-c, --colour <col>       Sample graph colour to correct against", "--device <N>"):
            assert opt in err, opt
        assert "not part of this build" not in err
    # the dispatcher knows the command; its own usage text and its list of commands stay as the transcripts of
    # tests/golden/cli_transcripts.json recorded them
    rc, _, err = run(maxk, "correct", "--nosuchoption")
    assert rc != 0 and "not part of this build" not in err and "thread/correct -h` for help. Bad option: --nosuchoption" in err


def test_argument_errors_and_refusals(built, tmp_path, txt):
    o = "%s:%s" % (txt, tmp_path / "out")
    cases = [
        (["-1", o], "Expected exactly one graph file"),
        (["-1", o, G31, G31], "Expected only one graph file. What is this: '%s'" % G31),
        (["-1", o, "-W", G31], "Ignored arguments after last --seq"),
        (["-1", o, "-d", "3", G31], "Ignored arguments after last --seq"),
        (["-1", o, "-M", "FF", G31], "Ignored arguments after last --seq"),
        (["-M", "XX", "-1", o, G31], "-M,--matepair <orient> must be one of: FF,FR,RF,RR"),
        (["-d", "-1", "-1", o, G31], "-d, --gap-diff-const requires a double x >= 0: -1"),
        (["-D", "nan", "-1", o, G31], "-D, --gap-diff-coeff requires a double x >= 0: nan"),
        (["-D", "x", "-1", o, G31], "-D, --gap-diff-coeff requires a double x >= 0: x"),
        (["-X", "x", "-1", o, G31], "-X, --max-context requires an int x >= 0: x"),
        (["-l", "9", "-L", "3", "-1", o, G31], "--min-ins 9 is greater than --max-ins 3"),
        (["-Z", "ab", "-1", o, G31], "--fq-zero <c> requires a single char"),
        (["-Z", "a", "-Z", "b", "-1", o, G31], "-Z, --fq-zero given twice"),
        (["-P", "-P", "-1", o, G31], "-P, --print-orig given twice"),
        (["-F", "FASTA", "-F", "FASTA", "-1", o, G31], "-F, --format given twice"),
        (["-F", "banana", "-1", o, G31], "Invalid -F, --format {FASTA,FASTQ,PLAIN} option: banana"),
        (["-1", txt, G31], "Expected -1 <in>:<out>"),
        (["-2", o, G31], "Expected -2 <in1>:<in2>:<out>"),
        (["-1", "%s:%s" % (tmp_path / "missing.txt", tmp_path / "out"), G31], "Cannot open -1 file: %s" % (tmp_path / "missing.txt")),
        (["-c", "x", "-1", o, G31], "-c, --colour requires an int x >= 0: x"),
        (["-c", "2", "-1", o, G31], "-c, --colour 2: the graph has 2 colours"),
        (["--device", "x", "-1", o, G31], "--device requires an int x >= 0: x"),
        (["-1", o, str(tmp_path / "missing.ctx")], "missing.ctx"),
        # what this build leaves out, each by the option's name
        (["-p", "links.ctp", "-1", o, G31], "-p, --paths <in.ctp>: link files are not part of this build"),
        (["--paths", "links.ctp", "-1", o, G31], "-p, --paths <in.ctp>: link files are not part of this build"),
        (["-Q", "10", "-1", o, G31], "-Q, --fq-cutoff <Q> is not part of this build's `correct`"),
        (["-O", "33", "-1", o, G31], "-O, --fq-offset <N> is not part of this build's `correct`"),
        (["-H", "5", "-1", o, G31], "-H, --cut-hp <bp> is not part of this build's `correct`"),
        (["-g", "gaps.csv", "-1", o, G31], "-g, --gap-hist <o.csv> is not part of this build's `correct`"),
        (["-G", "frag.csv", "-1", o, G31], "-G, --frag-hist <o.csv> is not part of this build's `correct`"),
        (["-C", "contig.csv", "-1", o, G31], "-C, --contig-hist <.csv> is not part of this build's `correct`"),
    ]
    for args, msg in cases:
        rc, out, err = run(31, "correct", *args)
        assert rc != 0 and msg in err and out == b"", (args, err)
        assert sorted(os.listdir(tmp_path)) == ["in.txt"], args  # nothing was created


# ---- on the device ---------------------------------------------------------------------------------------------------
def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read().decode()


def want_text(graph, k, reads, fmt, print_orig=False, fq_zero=".", **kw):
    """reads = [(name, seq, qual)]"""
    out = []
    for name, seq, qual in reads:
        s, q = X.correct(graph, k, seq, qual, fq_zero=fq_zero, **kw)
        out.append(X.fmt_read(name, s, q, seq, fmt, print_orig, fq_zero))
    return "".join(out)


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    """the files of the reference's tests/correct, the graph built by this repository's own `build`"""
    d = tmp_path_factory.mktemp("correct")
    (d / "ref.txt").write_text("".join(s + "\n" for s in CASE["graph_seqs"]))
    bad = [c for c in CASE["cases"] if not c["qual"]]
    indels = [c for c in CASE["cases"] if c["qual"]]
    (d / "bad.txt").write_text("".join(c["read"] + "\n" for c in bad))
    (d / "indels.bad.fq").write_text("".join("@%s\n%s\n+\n%s\n" % (c["name"], c["read"], c["qual"]) for c in indels))
    ctx = d / "ref.k9.ctx"
    rc, _, err = run(31, "build", "-q", "-k", K, "-s", "ref", "-1", d / "ref.txt", ctx)
    assert rc == 0, err
    return d, ctx, R.build([CASE["graph_seqs"]], K), bad, indels


@pytest.mark.gpu
def test_reference_command_lines(case):
    d, ctx, graph, bad, indels = case
    plain = [("", c["read"], "") for c in bad]
    # correct -q -t 1 -m 10M -F FASTA --print-orig -1 bad.txt:good ref.k9.ctx
    rc, out, err = run(31, "correct", "-q", "-t", 1, "-m", "10M", "-F", "FASTA", "--print-orig", "-1", "%s:%s" % (d / "bad.txt", d / "good"), ctx)
    assert rc == 0 and out == b"" and err == "", err
    got = gunzip(d / "good.fa.gz")
    assert got == want_text(graph, K, plain, "fa", True)
    assert got == "".join("> orig=%s\n%s\n" % (c["read"], c["corrected"]) for c in bad)
    # ... -F FASTQ: a read without qualities gets fq_zero for every base
    rc, out, err = run(31, "correct", "-q", "-t", 1, "-m", "10M", "-F", "FASTQ", "--print-orig", "-1", "%s:%s" % (d / "bad.txt", d / "good"), ctx)
    assert rc == 0 and err == "", err
    got = gunzip(d / "good.fq.gz")
    assert got == want_text(graph, K, plain, "fq", True)
    assert got == "".join("@ orig=%s\n%s\n+\n%s\n" % (c["read"], c["corrected"], "." * len(c["corrected"])) for c in bad)
    # the indel FASTQ with its qualities (FASTQ is the default format); the status lines of a run that is not quiet
    fq = [(c["name"], c["read"], c["qual"]) for c in indels]
    rc, out, err = run(31, "correct", "-t", 1, "--print-orig", "-1", "%s:%s" % (d / "indels.bad.fq", d / "indels.good"), ctx)
    assert rc == 0, err
    got = gunzip(d / "indels.good.fq.gz")
    assert got == want_text(graph, K, fq, "fq", True)
    assert "@ins_T>TT orig=%s\n%s\n+\nabcdefghijklmnopqrstuwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ1\n" % (indels[0]["read"], indels[0]["corrected"]) in got
    assert [ln for ln in got.split("\n")[1::4]] == [c["corrected"] for c in indels]
    assert "[CorrectReads] 4 reads" in err and "gaps: 6, filled 6" in err
    # an existing output is kept unless --force; -Z, plain output, two threads
    rc, out, err = run(31, "correct", "-1", "%s:%s" % (d / "indels.bad.fq", d / "indels.good"), ctx)
    assert rc != 0 and "Output file already exists: %s" % (d / "indels.good.fq.gz") in err and "Error creating output files" in err
    assert gunzip(d / "indels.good.fq.gz") == got
    rc, out, err = run(31, "correct", "-q", "-f", "-Z", "#", "-1", "%s:%s" % (d / "indels.bad.fq", d / "indels.good"), ctx)
    assert rc == 0 and gunzip(d / "indels.good.fq.gz") == want_text(graph, K, fq, "fq", False, "#"), err
    rc, out, err = run(31, "correct", "-q", "-F", "plain", "-1", "%s:%s" % (d / "indels.bad.fq", d / "indels.good"), ctx)
    assert rc == 0 and gunzip(d / "indels.good.txt.gz") == "".join(c["corrected"] + "\n" for c in indels), err


@pytest.mark.gpu
def test_seq2_seqi_pairs_order_and_task_options(case):
    d, ctx, graph, bad, indels = case
    fq = [(c["name"], c["read"], c["qual"]) for c in indels]
    r1 = [("p%d/1" % i, s, q) for i, (_, s, q) in enumerate(fq)]
    r2 = [("p%d/2" % i, s, q) for i, (_, s, q) in enumerate(reversed(fq))]
    (d / "r1.fq").write_text("".join("@%s\n%s\n+\n%s\n" % r for r in r1))
    (d / "r2.fq").write_text("".join("@%s\n%s\n+\n%s\n" % r for r in r2))
    rc, out, err = run(31, "correct", "-q", "-2", "%s:%s:%s" % (d / "r1.fq", d / "r2.fq", d / "pe"), ctx)
    assert rc == 0, err
    assert gunzip(d / "pe.1.fq.gz") == want_text(graph, K, r1, "fq")
    assert gunzip(d / "pe.2.fq.gz") == want_text(graph, K, r2, "fq")
    assert gunzip(d / "pe.fq.gz") == ""
    # interleaved: pairs by name, a read without a mate goes to the unpaired file
    inter = [x for pair in zip(r1[:2], r2[:2]) for x in pair] + [("lonely", fq[0][1], fq[0][2])] + [r1[2], r2[2]]
    (d / "i.fq").write_text("".join("@%s\n%s\n+\n%s\n" % r for r in inter))
    # the options in front of a --seq are that task's: two-way and d = 0 for the first, the defaults again for the second
    rc, out, err = run(31, "correct", "-q", "-F", "FASTA", "-W", "-d", "0", "-i", "%s:%s" % (d / "i.fq", d / "il"), "-w", "-d", "5", "-D", "0.1",
                       "-e", "-X", "7", "-l", "0", "-L", "500", "-M", "FR", "-1", "%s:%s" % (d / "bad.txt", d / "se"), ctx)
    assert rc == 0, err
    kw = {"two_way": True, "d": 0.0}
    assert gunzip(d / "il.1.fa.gz") == want_text(graph, K, [inter[0], inter[2], inter[5]], "fa", **kw)
    assert gunzip(d / "il.2.fa.gz") == want_text(graph, K, [inter[1], inter[3], inter[6]], "fa", **kw)
    assert gunzip(d / "il.fa.gz") == want_text(graph, K, [inter[4]], "fa", **kw)
    assert gunzip(d / "se.fa.gz") == want_text(graph, K, [("", c["read"], "") for c in bad], "fa")


@pytest.mark.gpu
def test_colour_of_a_two_colour_file(case):
    d, ctx, graph, bad, indels = case
    (d / "other.txt").write_text(CASE["graph_seqs"][0] + "\n")
    ctx2 = d / "two.k9.ctx"
    rc, _, err = run(31, "build", "-q", "-k", K, "-s", "other", "-1", d / "other.txt", "-s", "ref", "-1", d / "ref.txt", ctx2)
    assert rc == 0, err
    g2 = R.build([[CASE["graph_seqs"][0]], CASE["graph_seqs"]], K)
    plain = [("", c["read"], "") for c in bad]
    for col in (0, 1):
        rc, out, err = run(31, "correct", "-q", "-f", "-F", "FASTA", "-c", col, "-1", "%s:%s" % (d / "bad.txt", d / "col"), ctx2)
        assert rc == 0, err
        assert gunzip(d / "col.fa.gz") == want_text(g2, K, plain, "fa", colour=col)
    assert want_text(g2, K, plain, "fa", colour=0) != want_text(g2, K, plain, "fa", colour=1) == want_text(graph, K, plain, "fa")


@pytest.mark.gpu
def test_mccortex63_at_k33(built, tmp_path):
    import random
    import correct_cases as CC
    k = 33
    rng = random.Random(33)
    gen = CC.rseq(rng, 700)
    (tmp_path / "gen.txt").write_text(gen + "\n")
    rc, _, err = run(63, "build", "-q", "-k", k, "-s", "gen", "-1", tmp_path / "gen.txt", tmp_path / "g.ctx")
    assert rc == 0, err
    graph = R.build([[gen]], k)
    rd = []
    for i in range(40):
        q = rng.randrange(0, len(gen) - 160)
        s = CC.mutate(rng, gen[q:q + rng.randrange(90, 160)], nsub=i % 3, indel=(0, 1, -2, 3)[i % 4], n_at=i % 7 == 0)
        s = CC.rc(s) if i % 2 else s
        rd.append(("r%d" % i, s, "".join(chr(65 + (i + j) % 26) for j in range(len(s)))))
    (tmp_path / "r.fq").write_text("".join("@%s\n%s\n+\n%s\n" % r for r in rd))
    rc, out, err = run(63, "correct", "-q", "-1", "%s:%s" % (tmp_path / "r.fq", tmp_path / "o"), tmp_path / "g.ctx")
    assert rc == 0, err
    want = want_text(graph, k, rd, "fq")
    assert gunzip(tmp_path / "o.fq.gz") == want
    assert sum(a != b for a, b in zip(want.split("\n")[1::4], (s for _, s, _ in rd))) > 20  # (most reads were changed)
