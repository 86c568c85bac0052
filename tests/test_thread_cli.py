"""`mccortex<K> thread`: the command-line contract of src/commands/ctx_thread.c and read_thread_cmd.c without -p and -u,
and its command lines on the golden graph of the reference's unit test (golden/thread.json) on the device: the .ctp.gz
is gunzipped, its JSON header checked field by field against thread_restate.py and the command line, its body compared
byte for byte."""
import gzip
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import thread_restate as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
G31 = os.path.join(GOLD, "tiny_k31.ctx")
CASE = json.load(open(os.path.join(GOLD, "thread.json")))["path_tests"]
K = CASE["k"]
READS = [c["read"] for c in CASE["calls"]]
TOTAL = sum(len(s) for s in CASE["graph_seqs"])


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
    p.write_text(READS[0] + "\n")
    return str(p)


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_help_and_dispatcher(built, maxk):
    for args in (["thread", "-h"], ["thread"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d thread [options] <in.ctx>" % maxk in err
        assert "Thread reads through the graph.  Save to file <out.ctp>." in err
        for opt in ("-o, --out <out.ctp.gz>   Save output file [required]",
                    "-p, --paths <in.ctp>     Load link file (can specify multiple times)",
                    "-0, --zero-paths         Zero counts on initially loaded links.",
                    "-1, --seq <in.fa>        Thread reads from file",
                    "-2, --seq2 <in1:in2>     Thread paired end sequences",
                    "-i, --seqi <in.bam>      Thread PE reads from a single file",
                    "-w, --one-way            Use one-way gap filling (conservative) [default]",
                    "-W, --two-way            Use two-way gap filling (liberal)",
                    "-D, --gap-diff-coeff <D>   abs(gap_exp - gap_seen) <= gap_exp*D + d",
                    "-u, --use-new-paths      Use links as they are being added",
                    "-x,--print-contigs -y,--print-paths -z,--print-reads", "--device <N>"):
            assert opt in err, opt
        assert "not part of this build" not in err
    # the dispatcher knows the command; its own usage text and its list of commands stay as the transcripts of
    # tests/golden/cli_transcripts.json recorded them
    rc, _, err = run(maxk, "thread", "--nosuchoption")
    assert rc != 0 and "not part of this build" not in err and "thread/correct -h` for help. Bad option: --nosuchoption" in err


def test_argument_errors_and_refusals(built, tmp_path, txt):
    o = str(tmp_path / "out.ctp.gz")
    cases = [
        (["-1", txt, "-o", o], "Expected exactly one graph file"),
        (["-1", txt, "-o", o, G31, G31], "Expected only one graph file. What is this: '%s'" % G31),
        (["-1", txt, G31], "--out <out.ctp> is required"),
        (["-o", o, "-o", o, "-1", txt, G31], "-o, --out given twice"),
        (["-f", "-f", "-o", o, "-1", txt, G31], "-f, --force given twice"),
        (["-o", o, "-1", txt, "-W", G31], "Ignored arguments after last --seq"),
        (["-o", o, "-1", txt, "-d", "3", G31], "Ignored arguments after last --seq"),
        (["-o", o, "-1", txt, "-E", G31], "Ignored arguments after last --seq"),
        (["-o", o, "-M", "XX", "-1", txt, G31], "-M,--matepair <orient> must be one of: FF,FR,RF,RR"),
        (["-o", o, "-d", "-1", "-1", txt, G31], "-d, --gap-diff-const requires a double x >= 0: -1"),
        (["-o", o, "-D", "nan", "-1", txt, G31], "-D, --gap-diff-coeff requires a double x >= 0: nan"),
        (["-o", o, "-X", "x", "-1", txt, G31], "-X, --max-context requires an int x >= 0: x"),
        (["-o", o, "-l", "x", "-1", txt, G31], "-l, --min-frag-len requires an int x >= 0: x"),
        (["-o", o, "-L", "x", "-1", txt, G31], "-L, --max-frag-len requires an int x >= 0: x"),
        (["-o", o, "-l", "9", "-L", "3", "-1", txt, G31], "--min-ins 9 is greater than --max-ins 3"),
        (["-o", o, "-t", "0", "-1", txt, G31], "-t, --threads requires an int x > 0"),
        (["-o", o, "-1", str(tmp_path / "missing.txt"), G31], "Cannot open -1 file: %s" % (tmp_path / "missing.txt")),
        (["-o", o, "--device", "x", "-1", txt, G31], "--device requires an int x >= 0: x"),
        (["-o", o, "-1", txt, str(tmp_path / "missing.ctx")], "missing.ctx"),
        # what this build leaves out, each by the option's name and with the reason
        (["-p", "links.ctp", "-o", o, "-1", txt, G31], "-p, --paths <in.ctp>: the walker that uses links is not part of this build"),
        (["--paths", "links.ctp", "-o", o, "-1", txt, G31], "-p, --paths <in.ctp>: the walker that uses links is not part of this build"),
        (["-0", "-o", o, "-1", txt, G31], "-0, --zero-paths has no meaning without -p, --paths <in.ctp>, which is not part of this build"),
        (["-u", "-o", o, "-1", txt, G31], "-u, --use-new-paths: the walker that uses links is not part of this build"),
        (["-o", o, "-2", "%s:%s" % (txt, txt), G31], "-2, --seq2 <in1:in2>: the insert gap between mates is not built; give each mate's file as --seq"),
        (["-o", o, "-i", txt, G31], "-i, --seqi <in.bam>: the insert gap between mates is not built; give the reads as --seq"),
        (["-o", o, "-Q", "10", "-1", txt, G31], "-Q, --fq-cutoff <Q> is not part of this build's `thread`"),
        (["-o", o, "-O", "33", "-1", txt, G31], "-O, --fq-offset <N> is not part of this build's `thread`"),
        (["-o", o, "-H", "5", "-1", txt, G31], "-H, --cut-hp <bp> is not part of this build's `thread`"),
        (["-o", o, "-g", "gaps.csv", "-1", txt, G31], "-g, --gap-hist <o.csv> is not part of this build's `thread`"),
        (["-o", o, "-G", "frag.csv", "-1", txt, G31], "-G, --frag-hist <o.csv> is not part of this build's `thread`"),
        (["-o", o, "-x", "-1", txt, G31], "-x, --print-contigs is not part of this build's `thread`"),
        (["-o", o, "-y", "-1", txt, G31], "-y, --print-paths is not part of this build's `thread`"),
        (["-o", o, "-z", "-1", txt, G31], "-z, --print-reads is not part of this build's `thread`"),
    ]
    for args, msg in cases:
        rc, out, err = run(31, "thread", *args)
        assert rc != 0 and msg in err and out == b"", (args, err)
        assert sorted(os.listdir(tmp_path)) == ["in.txt"], args  # nothing was created


# ---- on the device ---------------------------------------------------------------------------------------------------
def read_ctp(path):
    """(header, comment lines, body) of a .ctp.gz"""
    with gzip.open(path, "rb") as f:
        text = f.read().decode()
    dec = json.JSONDecoder()
    hdr, end = dec.raw_decode(text)
    assert text[end:end + 2] == "\n\n"
    lines = text[end + 2:].split("\n")
    n = 0
    while n < len(lines) and (lines[n].startswith("#") or lines[n] == ""):
        n += 1
    assert all(ln.startswith("#") for ln in lines[:n] if ln) and n > 3
    return hdr, lines[:n], "\n".join(lines[n:])


def check_header(hdr, k, graph, total_sequence, store, out_path, argv, inputs):
    """the fields the reference's reader demands (gpath_reader.c:27-190) and those of gpath_save_mkhdr"""
    assert hdr["file_format"] == "ctp" and hdr["format_version"] == 4
    assert len(hdr["file_key"]) == 16 and int(hdr["file_key"], 16) >= 0
    g = hdr["graph"]
    assert g["num_colours"] == 1 and g["kmer_size"] == k and g["num_kmers_in_graph"] == len(graph)
    assert len(g["colours"]) == 1
    col = g["colours"][0]
    assert col["colour"] == 0 and col["sample"] == "ref" and col["cleaned_tips"] is False and col["cleaned_unitigs"] is False
    assert col["total_sequence"] == total_sequence
    assert len(hdr["commands"]) == 1
    cmd = hdr["commands"][0]
    assert len(cmd["key"]) == 8 and cmd["prev"] == [] and cmd["out_key"] == hdr["file_key"]
    assert cmd["cmd"][1:] == [str(a) for a in argv] and cmd["cmd"][0].startswith("mccortex")
    assert cmd["out_path"] == os.path.realpath(str(out_path)) and os.path.isdir(cmd["cwd"]) and len(cmd["date"]) == 19
    got = cmd["thread"]["inputs"]
    assert len(got) == len(inputs)
    for a, b in zip(got, inputs):
        want = {"interleaved": False, "fq_offset": 0, "fq_cutoff": 0, "hp_cutoff": 0, "matepair": "FR", "frag_len_min_bp": 0,
                "frag_len_max_bp": 1000, "one_way_gap_fill": True, "use_end_check": True, "max_context": 200, "gap_variance": 0.1,
                "gap_wiggle": 5}
        want.update(b)
        assert a == want, (a, want)
    p = hdr["paths"]
    info = store.info()
    assert {n: p[n] for n in info} == info
    assert len(p["contig_hists"]) == 1
    hist = store.contig_hist()
    assert p["contig_hists"][0] == {"lengths": [a for a, _ in hist], "counts": [b for _, b in hist]}


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    """the graph of the reference's unit test, built by this repository's own `build`"""
    d = tmp_path_factory.mktemp("thread")
    (d / "ref.txt").write_text("".join(s + "\n" for s in CASE["graph_seqs"]))
    (d / "reads.txt").write_text("".join(s + "\n" for s in READS))
    (d / "reads.fa").write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(READS)))
    with gzip.open(d / "reads.fq.gz", "wt") as f:
        f.write("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(READS)))
    ctx = d / "ref.k11.ctx"
    rc, _, err = run(31, "build", "-q", "-k", K, "-s", "ref", "-1", d / "ref.txt", ctx)
    assert rc == 0, err
    return d, ctx, R.build([CASE["graph_seqs"]], K)


@pytest.mark.gpu
def test_command_lines_on_the_golden_graph(case):
    d, ctx, graph = case
    want = T.Store(graph, K).thread(READS)
    bodies = []
    for name in ("reads.txt", "reads.fa", "reads.fq.gz"):
        out = d / (name + ".ctp.gz")
        argv = ["thread", "-q", "-t", 1, "-m", "10M", "--seq", d / name, "-o", out, ctx]
        rc, so, err = run(31, *argv)
        assert rc == 0 and so == b"" and err == "", err
        hdr, comments, body = read_ctp(out)
        argv.remove("-q")  # (the dispatcher takes it)
        check_header(hdr, K, graph, TOTAL, want, out, argv, [{"files": [str(d / name)]}])
        assert body.encode() == want.text()
        bodies.append(body)
    assert len(set(bodies)) == 1 and want.info()["num_paths"] == 15
    # an existing output is kept unless --force; the status lines of a run that is not quiet
    out = d / "reads.txt.ctp.gz"
    rc, so, err = run(31, "thread", "--seq", d / "reads.txt", "-o", out, ctx)
    assert rc != 0 and "File already exists: %s" % out in err
    assert read_ctp(out)[2] == bodies[0]
    rc, so, err = run(31, "thread", "-f", "--seq", d / "reads.txt", "-o", out, ctx)
    assert rc == 0 and "links generated: 15; kept: 15 on 10 k-mers" in err and "Creating paths file: %s" % out in err, err
    assert read_ctp(out)[2] == bodies[0]
    # two --seq files, each with the options in front of it: every count is 2; -W, -d / -D, -X, -E, -M, -l / -L in the header
    out = d / "two.ctp.gz"
    argv = ["thread", "-t", 2, "-W", "-d", 2, "-D", "0.25", "-X", 7, "-E", "-M", "FF", "-l", 5, "-L", 500, "--seq", d / "reads.fa",
            "-w", "-d", 5, "-D", "0.1", "-e", "--seq", d / "reads.txt", "-o", out, ctx]
    rc, so, err = run(31, *argv)
    assert rc == 0, err
    hdr, comments, body = read_ctp(out)
    twice = T.Store(graph, K).thread(READS, two_way=True, D=0.25, d=2.0).thread(READS)
    first = {"files": [str(d / "reads.fa")], "one_way_gap_fill": False, "gap_wiggle": 2, "gap_variance": 0.25, "max_context": 7,
             "use_end_check": False, "matepair": "FF", "frag_len_min_bp": 5, "frag_len_max_bp": 500}
    second = dict(first, files=[str(d / "reads.txt")], one_way_gap_fill=True, gap_wiggle=5, gap_variance=0.1, use_end_check=True)
    check_header(hdr, K, graph, TOTAL, twice, out, argv, [first, second])
    assert body.encode() == twice.text() and set(twice.links.values()) == {2}
    # a colour filter that yields one colour is fine; to stdout
    rc, so, err = run(31, "thread", "-q", "--seq", d / "reads.txt", "-o", "-", "%s:0" % ctx)
    assert rc == 0, err
    (d / "stdout.ctp.gz").write_bytes(so)
    assert read_ctp(d / "stdout.ctp.gz")[2] == bodies[0]


@pytest.mark.gpu
def test_a_filter_of_several_colours_dies(case):
    d, ctx, graph = case
    (d / "other.txt").write_text(CASE["graph_seqs"][0] + "\n")
    ctx2 = d / "two.k11.ctx"
    rc, _, err = run(31, "build", "-q", "-k", K, "-s", "other", "-1", d / "other.txt", "-s", "ref", "-1", d / "ref.txt", ctx2)
    assert rc == 0, err
    out = d / "no.ctp.gz"
    rc, so, err = run(31, "thread", "--seq", d / "reads.txt", "-o", out, ctx2)
    assert rc != 0 and "Please specify a single colour e.g. %s:0" % ctx2 in err and not out.exists()
    # one colour of the two: the links of the whole graph from colour 1, those of its first sequence alone from colour 0
    for col, seqs in ((1, CASE["graph_seqs"]), (0, CASE["graph_seqs"][:1])):
        rc, so, err = run(31, "thread", "-q", "-f", "--seq", d / "reads.txt", "-o", out, "%s:%d" % (ctx2, col))
        assert rc == 0, err
        assert read_ctp(out)[2].encode() == T.Store(R.build([seqs], K), K).thread(READS).text()


@pytest.mark.gpu
def test_mccortex63_at_k33(built, tmp_path):
    import random
    import correct_cases as CC
    import thread_cases as TC
    k = 33
    rng = random.Random(33)
    gen = CC.rseq(rng, 900)
    alt = gen[:300] + TC.other(gen[300]) + gen[301:450] + TC.other(gen[450]) + gen[451:700]  # (two bubbles: a join, then a fork)
    (tmp_path / "gen.txt").write_text(gen + "\n" + alt + "\n")
    rc, _, err = run(63, "build", "-q", "-k", k, "-s", "ref", "-1", tmp_path / "gen.txt", tmp_path / "g.ctx")
    assert rc == 0, err
    g = R.build([[gen, alt]], k)
    rd = []
    for i in range(40):
        q = rng.randrange(0, len(gen) - 400)
        s = CC.mutate(rng, (alt if i % 3 == 0 else gen)[q:q + rng.randrange(150, 400)], nsub=i % 3)
        rd.append(CC.rc(s) if i % 2 else s)
    (tmp_path / "r.txt").write_text("".join(s + "\n" for s in rd))
    out = tmp_path / "o.ctp.gz"
    argv = ["thread", "--seq", tmp_path / "r.txt", "-o", out, tmp_path / "g.ctx"]
    rc, so, err = run(63, *argv)
    assert rc == 0, err
    want = T.Store(g, k).thread(rd)
    hdr, comments, body = read_ctp(out)
    check_header(hdr, k, g, len(gen) + len(alt), want, out, argv, [{"files": [str(tmp_path / "r.txt")]}])
    assert body.encode() == want.text() and want.info()["num_paths"] >= 4
