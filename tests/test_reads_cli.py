"""`mccortex<K> reads`: the command-line contract of src/commands/ctx_reads.c, and a replay of the four command lines of
the reference's tests/reads (golden/reads.json) on the device, compared byte for byte with reads_restate.py."""
import gzip
import json
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reads_restate as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
G31, G5 = os.path.join(GOLD, "tiny_k31.ctx"), os.path.join(GOLD, "tiny_k5.ctx")
CASE = json.load(open(os.path.join(GOLD, "reads.json")))


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
    for args in (["reads", "-h"], ["reads"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d reads [options] <in.ctx>[:cols] [in2.ctx ...]" % maxk in err
        assert "Filters reads based on which have a kmer in the graph." in err
        for opt in ("-h, --help                  This help message", "-q, --quiet                 Silence status output",
                    "-f, --force                 Overwrite output files", "-m, --memory <mem>          Memory to use",
                    "-n, --nkmers <kmers>        Number of hash table entries (e.g. 1G ~ 1 billion)",
                    "-t, --threads <T>           Number of threads to use [default: 2]",
                    "-F, --format <f>            Output format may be: FASTA, FASTQ [default: FASTQ]",
                    "-v, --invert                Print reads/read pairs with no kmer in graph",
                    "-1, --seq  <in>:<O>         Writes output to <O>.fq.gz",
                    "-2, --seq2 <in1>:<in2>:<O>  Writes output to <O>.{1,2}.fq.gz",
                    "-i, --seqi <in>:<O>         Writes output to <O>.{1,2}.fq.gz", "--device <N>",
                    "Output is <O>.fq.gz for FASTQ, <O>.fa.gz for FASTA, <O>.txt.gz for plain",
                    "If either read of a\n  pair touches the graph, both are printed."):
            assert opt in err, opt
        assert "not part of this build" not in err
    rc, _, err = run(maxk)
    assert "reads       filter reads against a graph" in err
    rc, _, err = run(maxk, "view", "x.ctx")
    assert "not part of this build" in err and "reads" in err


def test_argument_errors(built, tmp_path, fa):
    o = str(tmp_path / "o")
    missing = str(tmp_path / "missing.fa")
    cases = [
        ([G31], "Please specify at least one sequence file (-1, -2 or -i)"),
        (["--seq", fa + ":" + o], "Please specify input graph file(s)"),
        (["-1", fa + ":" + o, "-F", "SAM", G31], "Invalid -F, --format {FASTA,FASTQ,PLAIN} option: SAM"),
        (["-1", fa + ":" + o, "--format", "banana", G31], "Invalid -F, --format {FASTA,FASTQ,PLAIN} option: banana"),
        (["-1", fa + ":" + o, "-F", "fa", "-F", "fq", G31], "-F, --format given twice"),
        (["-1", fa, G31], "Expected -1 <in>:<out>"),
        (["-1", fa + ":" + o + ":x", G31], "Expected -1 <in>:<out>"),
        (["--seq2", fa + ":" + o, G31], "Expected -2 <in1>:<in2>:<out>"),
        (["--seqi", fa, G31], "Expected -i <in>:<out>"),
        (["-1", missing + ":" + o, G31], "Cannot open -1 file: %s" % missing),
        (["-1", missing + "," + o, G31], "Cannot open -1 file: %s" % missing),
        (["-i", missing + ":" + o, G31], "Cannot open -i file: %s" % missing),
        (["-2", fa + ":" + missing + ":" + o, G31], "Cannot open 2 file: %s" % missing),
        (["-1", fa + ":" + o, "-f", "-f", G31], "-f, --force given twice"),
        (["-1", fa + ":" + o, "-v", "--invert", G31], "-v, --invert given twice"),
        (["-1", fa + ":" + o, "-t", "0", G31], "-t, --threads requires an int x > 0"),
        (["-1", fa + ":" + o, "-t", "2", "-t", "3", G31], "-t, --threads given twice"),
        (["-1", fa + ":" + o, "-m", "1G", "-m", "1G", G31], "-m, --memory <M> specifed more than once"),
        (["-1", fa + ":" + o, "-n", "1M", "-n", "1M", G31], "-n, --nkmers <N> specifed more than once"),
        (["-1", fa + ":" + o, "-n", "banana", G31], "Invalid hash size: banana"),
        (["-1", fa + ":" + o, "--device", "x", G31], "--device requires an int x >= 0: x"),
        (["-1", fa + ":" + o, "--nosuchoption", G31], "reads -h` for help. Bad option: --nosuchoption"),
        (["-1", fa + ":" + o, str(tmp_path / "missing.ctx")], "missing.ctx"),
        (["-1", fa + ":" + o, G31, G5], "Kmer sizes don't match [31 vs 5]"),
    ]
    for args, msg in cases:
        rc, out, err = run(31, "reads", *args)
        assert rc != 0 and msg in err and out == b"", (args, err)
        assert sorted(os.listdir(tmp_path)) == ["in.fa"], args  # nothing was created


def test_no_overwrite_without_force(built, tmp_path, fa):
    # the third output of the second task exists: refused before a device is looked for, the three files this run had
    # created by then are gone again, and the existing one is as it was
    exists = tmp_path / "out" / "b.2.fq.gz"
    exists.parent.mkdir()
    exists.write_bytes(b"keep")
    rc, out, err = run(31, "reads", "--seq", "%s:%s" % (fa, tmp_path / "out" / "deep" / "a"), "--seq2", "%s:%s:%s" % (fa, fa, tmp_path / "out" / "b"),
                       "--seqi", "%s:%s" % (fa, tmp_path / "out" / "c"), G31)
    assert rc != 0 and out == b""
    assert "Output file already exists: %s" % exists in err and "Error creating output files" in err
    assert exists.read_bytes() == b"keep"
    left = sorted(os.path.join(d, f) for d, _, fs in os.walk(tmp_path / "out") for f in fs)
    assert left == [str(exists)], left
    # a path that cannot be created
    (tmp_path / "file").write_text("x")
    rc, _, err = run(31, "reads", "--seq", "%s:%s" % (fa, tmp_path / "file" / "a"), G31)
    assert rc != 0 and "Cannot create file: %s" % (tmp_path / "file" / "a.fq.gz") in err and "Error creating output files" in err


# ---- on the device ---------------------------------------------------------------------------------------------------
def fasta(reads):
    return "".join(">%s\n%s\n" % (n, s) for n, s in reads)


def gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read().decode()


def totals(err):
    m = re.search(r"Total printed (\d+) / (\d+) \((\d+\.\d\d)%\) reads", err)
    assert m, err
    assert m.group(3) == "%.2f" % (100.0 * int(m.group(1)) / int(m.group(2)) if int(m.group(2)) else 0.0)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.gpu
def test_reference_k9(built, tmp_path):
    k = CASE["k"]
    keys = S.keys_of([CASE["genome"]], k)
    (tmp_path / "seq.fa").write_text(CASE["genome"] + "\n")
    ctx = tmp_path / "seq.k9.ctx"
    rc, _, err = run(31, "build", "-q", "-m", "1M", "-k", k, "--sample", "Seq", "--seq", tmp_path / "seq.fa", ctx)
    assert rc == 0, err
    (tmp_path / "reads.fa").write_text(fasta(CASE["reads"]))
    with gzip.open(tmp_path / "reads.1.fa.gz", "wb") as f:
        f.write(fasta(CASE["reads1"]).encode())
    with gzip.open(tmp_path / "reads.2.fa.gz", "wb") as f:
        f.write(fasta(CASE["reads2"]).encode())
    inter = [r for pair in zip(CASE["reads1"], CASE["reads2"]) for r in pair]
    with gzip.open(tmp_path / "reads.interleaved.fq.gz", "wb") as f:  # (the last record has no newline, as in the reference's test)
        f.write((fasta(inter) + fasta(CASE["singles"])).rstrip("\n").encode())
    rd = {n: [(a, b, "") for a, b in CASE[n]] for n in ("reads", "reads1", "reads2", "singles")}
    se = [[(r,) for r in rd[n]] for n in ("reads", "reads1", "reads2")]
    pe = S.pair_seq2(rd["reads1"], rd["reads2"])
    ipe = S.pair_seqi([(a, b, "") for a, b in inter] + rd["singles"])
    assert [len(u) for u in ipe] == [2] * 5 + [1, 1]
    R1, R2, RI = tmp_path / "reads.1.fa.gz", tmp_path / "reads.2.fa.gz", tmp_path / "reads.interleaved.fq.gz"
    for invert in (False, True):
        out = tmp_path / ("out%d" % invert)
        inv = ["--invert"] if invert else []
        # (command line, [(output base, paired, units)], format)
        lines = [
            (["--seq", "%s:%s/se" % (tmp_path / "reads.fa", out), "--seq", "%s:%s/se.1" % (R1, out), "--seq", "%s:%s/se.2" % (R2, out)],
             [("se", False, se[0]), ("se.1", False, se[1]), ("se.2", False, se[2])], "fq"),
            (["--seq2", "%s:%s:%s/pe" % (R1, R2, out)], [("pe", True, pe)], "fq"),
            (["--seqi", "%s:%s/ipe" % (RI, out)], [("ipe", True, ipe)], "fq"),
            (["--format", "fa", "--seq2", "%s:%s:%s/pe" % (R1, R2, out)], [("pe", True, pe)], "fa"),
        ]
        for args, tasks, fmt in lines:
            rc, so, err = run(31, "reads", *inv, *args, ctx)
            assert rc == 0 and so == b"", err
            assert ("Printing reads that do %stouch the graph" % ("not " if invert else "")) in err
            printed = total = 0
            for base, paired, units in tasks:
                exp, p, t = S.filter_units(keys, k, units, fmt, invert)
                _, p_other, _ = S.filter_units(keys, k, units, fmt, not invert)
                assert p + p_other == t
                printed += p
                total += t
                for which in ("", "1", "2") if paired else ("",):
                    path = "%s/%s%s.%s.gz" % (out, base, "." + which if which else "", fmt)
                    assert gunzip(path) == exp[which], (args, path)
                if not paired and base != "se":  # (se.1 and se.2 are the bases of the other two tasks)
                    assert not os.path.exists("%s/%s.1.%s.gz" % (out, base, fmt))
            assert totals(err) == (printed, total), (args, err)
    # the outcome the reference's test documents: pairs 1, 2 and 4; the single `hit`
    assert gunzip(tmp_path / "out0" / "pe.1.fa.gz") == fasta([CASE["reads1"][i] for i in (0, 1, 3)])
    assert gunzip(tmp_path / "out0" / "ipe.fq.gz") == "@hit\nTACCGCCAGGTCAGGGCT\n+\n..................\n"
    assert gunzip(tmp_path / "out1" / "ipe.fq.gz") == "@moo\nACA\n+\n...\n"
    # printed + inverted-printed = total, from the two runs' own lines
    rc, _, e0 = run(31, "reads", "-f", "-t", "1", "--seqi", "%s:%s/x" % (RI, tmp_path), ctx)
    rc1, _, e1 = run(31, "reads", "-f", "-v", "--seqi", "%s:%s/x" % (RI, tmp_path), ctx)
    assert rc == 0 and rc1 == 0
    assert totals(e0) == (7, 12) and totals(e1) == (5, 12)
    # without -f the files of the run before are in the way
    rc, _, err = run(31, "reads", "--seqi", "%s:%s/x" % (RI, tmp_path), ctx)
    assert rc != 0 and "Output file already exists: %s/x.fq.gz" % tmp_path in err


@pytest.mark.gpu
def test_fastq_plain_and_short_mate_file(built, tmp_path):
    """qualities kept, cut and padded; plain output; lower case kept; a --seq2 task stops at the shorter file"""
    k = CASE["k"]
    g = CASE["genome"]
    keys = S.keys_of([g], k)
    (tmp_path / "seq.fa").write_text(g + "\n")
    ctx = tmp_path / "seq.ctx"
    rc, _, err = run(31, "build", "-q", "-k", k, "--sample", "Seq", "--seq", tmp_path / "seq.fa", ctx)
    assert rc == 0, err
    r1 = [("a/1 first", g[:12].lower(), "IIIIIIIIIIII"), ("b/1", "TTTTTTTTTTTTT", "#############"), ("c/1", g[20:33], "ABCDEFGHIJKLM")]
    r2 = [("a/2", "CCCCCCCCCCCC", "JJJJJJJJJJJJ"), ("b/2", "GGGGGGGGGGGGG", "$$$$$$$$$$$$$")]
    (tmp_path / "r1.fq").write_text("".join("@%s\r\n%s\n+\n%s\n" % r for r in r1))
    (tmp_path / "r2.fq").write_text("".join("@%s\n%s\n+\n%s\n" % r for r in r2))
    rc, _, err = run(31, "reads", "--seq2", "%s:%s:%s" % (tmp_path / "r1.fq", tmp_path / "r2.fq", tmp_path / "q"), ctx)
    assert rc == 0, err
    assert "Different number of reads in pe files [%s; %s]" % (tmp_path / "r1.fq", tmp_path / "r2.fq") in err
    exp, p, t = S.filter_units(keys, k, S.pair_seq2(r1, r2), "fq")
    assert (p, t) == (2, 4) == totals(err)
    for which in ("", "1", "2"):
        assert gunzip("%s/q%s.fq.gz" % (tmp_path, "." + which if which else "")) == exp[which]
    assert exp["1"] == "@a/1 first\n%s\n+\nIIIIIIIIIIII\n" % g[:12].lower()
    rc, _, err = run(31, "reads", "-F", "plain", "--seq", "%s:%s" % (tmp_path / "r1.fq", tmp_path / "p"), ctx)
    assert rc == 0, err
    assert gunzip(tmp_path / "p.txt.gz") == g[:12].lower() + "\n" + g[20:33] + "\n" and totals(err) == (2, 3)
