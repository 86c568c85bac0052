"""`mccortex<K> breakpoints`: what is decided before a device is needed (the usage text, the option checks of
ctx_breakpoints.c:76-114 and this build's refusal of -p, each with exit status 1 and nothing written; the ABI symbol, the
wrapper and the record size), and end-to-end runs on the GPU: graphs built by the `build` command from the breakpoint1
fixture and from cases of breakpoints_cases.py, called against their reference with the header's fields and the body byte
for byte equal to the restatement's."""
import gzip
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breakpoints_cases as BC  # noqa: E402
import breakpoints_restate as B  # noqa: E402
import clean_restate as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden")
COMMENT = ("\n# This file was generated with McCortex\n#   written by Isaac Turner <turner.isaac@gmail.com>\n#   url: https://github.com/mcveanlab/mccortex\n"
           "# \n# Comment lines begin with a # and are ignored, but must come after the header\n# Format is:\n#   chr=seq:start-end:strand:offset\n"
           "#   all coordinates are 1-based\n#   <strand> is + or -. If +, start <= end. If -, start >= end.\n"
           "#   <offset> is the position in the sequence where ref starts agreeing\n\n")


def run(maxk, *args, cwd=None):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


def test_abi_symbol_wrapper_and_record_size(mcx):
    assert hasattr(mcx.lib(), "mcx_graph_breakpoints")
    assert callable(mcx.Graph.breakpoints)
    assert tuple(n for n, _ in mcx.graph.BreakpointsStats._fields_) == B.STAT_NAMES and set(mcx.graph.BreakpointsStats().as_dict()) == set(B.STAT_NAMES)
    assert mcx.graph.BREAKPOINT_REC.itemsize == 80
    assert (mcx.graph.BREAKPOINTS_NO_REF_EDGES, mcx.graph.BREAKPOINTS_REF_LOADED, mcx.graph.BREAKPOINTS_LOAD_ONLY) == (1, 2, 4)
    assert [n for n, _ in mcx.graph.BreakpointsParams._fields_] == ["min_ref", "max_ref", "flags"]


@pytest.mark.parametrize("maxk", [31, 63])
def test_usage(built, maxk):
    rc, out, err = run(maxk, "breakpoints", "-h")
    assert rc == 1 and out == b""
    assert "usage: mccortex%d breakpoints [options] <in.ctx> [in2.ctx ..]" % maxk in err
    for opt in ("-o, --out <out.txt.gz>  Save calls (gzipped output) [default: STDOUT]", "-p, --paths <in.ctp>", "-s, --seq <in>          Trusted input",
                "-r, --minref <N>        Require <N> kmers at ref breakpoint [default: 5]", "-R, --maxref <N>        Stop after <N> kmers at ref breakpoint [default: 1000]",
                "-E, --no-ref-edges      Don't load edges from the reference", "-t, --threads <T>", "-m, --memory <mem>", "-n, --nkmers <kmers>", "-f, --force",
                "-q, --quiet", "--device <N>"):
        assert opt in err, opt


ERRORS = [
    ([], "Require at least one --seq file"),
    (["in.ctx"], "Require at least one --seq file"),
    (["--seq", "ref.fa"], "Require input graph files (.ctx)"),
    (["-1", "ref.fa", "-o", "x.txt.gz"], "Require input graph files (.ctx)"),
    (["-p", "x.ctp", "-s", "ref.fa", "in.ctx"], "-p, --paths <in.ctp>: link files are not part of this build"),
    (["-r", "0", "-s", "ref.fa", "in.ctx"], "-r, --minref requires an int x > 0: 0"),
    (["-r", "x", "-s", "ref.fa", "in.ctx"], "-r, --minref requires an int x > 0: x"),
    (["-R", "-3", "-s", "ref.fa", "in.ctx"], "-R, --maxref requires an int x >= 0: -3"),
    (["-r", "9", "-R", "8", "-s", "ref.fa", "in.ctx"], "must not be above -R, --maxref <N>: 9 > 8"),
    (["-r", "1001", "-s", "ref.fa", "in.ctx"], "must not be above -R, --maxref <N>: 1001 > 1000"),
    (["-r", "3", "-r", "4", "-s", "ref.fa", "in.ctx"], "-r, --minref given twice"),
    (["-E", "-E", "-s", "ref.fa", "in.ctx"], "-E, --no-ref-edges given twice"),
    (["-o", "a.gz", "-o", "b.gz", "-s", "ref.fa", "in.ctx"], "-o, --out given twice"),
    (["--bogus", "in.ctx"], "breakpoints -h` for help. Bad option: --bogus"),
    (["-s", "ref.fa", "-o", "x.txt.gz", "missing.ctx"], "missing.ctx"),
]


@pytest.mark.parametrize("args,msg", ERRORS)
def test_option_errors(built, tmp_path, args, msg):
    rc, out, err = run(31, "breakpoints", *args, cwd=str(tmp_path))
    assert rc == 1 and out == b"" and msg in err, err[-600:]
    assert os.listdir(str(tmp_path)) == []


def test_missing_seq_file_and_existing_output(built, tmp_path):
    """the checks that read the inputs: each dies before a device is asked for"""
    ctx = os.path.join(GOLDEN, "tiny_k31.ctx")
    ref = os.path.join(GOLDEN, "breakpoint2_ref.fa")
    out = tmp_path / "have.txt.gz"
    out.write_bytes(b"")
    for args, msg in ((["-s", tmp_path / "none.fa", ctx], "Cannot read --seq file"), (["-s", ref, "-o", out, ctx], "File already exists")):
        rc, so, err = run(31, "breakpoints", "--device", "99", *args)
        assert rc == 1 and so == b"" and msg in err, err[-600:]
    assert out.read_bytes() == b""


def test_bench_tool_phases_from_profile_spans():
    """tools/bench_breakpoints.py folds the handle's profile dict {kernel: (calls, ms)} into its passes"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_breakpoints

    class Stub:
        def profile(self):
            return {"k_bp_kmers_probe": (1, 1.0), "k_bp_pack": (2, 0.5), "k_bp_count": (1, 0.25), "k_bp_occ_sort": (1, 8.0), "radix_sort_pairs": (2, 3.0), "k_bp_breaks": (1, 2.0),
                    "k_bb_forklist": (1, 0.5), "k_bp_walk_count": (2, 1.0), "k_bp_walk_write": (2, 2.0), "k_bp_merge": (2, 0.5), "k_bp_calls<false>": (1, 0.25),
                    "k_bp_calls<true>": (1, 0.25), "k_bp_size": (1, 0.125), "k_bp_offsets": (1, 0.125), "k_bp_emit": (4, 4.0), "k_cl_links": (1, 7.0)}
    ph = bench_breakpoints.phases_of(bench_breakpoints.spans(Stub()))
    assert ph == {"index": 9.75, "breaks": 2.5, "walk": 3.0, "merge": 1.0, "size": 0.25, "emit": 4.0}


def split_file(raw):
    text = raw.decode()
    at = text.index(COMMENT)
    return json.loads(text[:at]), text[at + len(COMMENT):]


def fasta(path):
    names, seqs = [], []
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].strip())
                seqs.append("")
            else:
                seqs[-1] += line.strip()
    return names, seqs


def build_graph(maxk, k, fa, ctx, sample):
    rc, _, err = run(maxk, "build", "-q", "-k", k, "--sample", sample, "--seq", fa, ctx)
    assert rc == 0, err[-800:]


def check_header(hdr, maxk, k, ncols, nkmers, samples, prm, ref_files, contigs):
    assert hdr["file_format"] == "CtxBreakpoints" and hdr["format_version"] == 3 and len(hdr["file_key"]) == 16
    gr = hdr["graph"]
    assert (gr["num_colours"], gr["kmer_size"], gr["num_kmers_in_graph"]) == (ncols, k, nkmers)
    assert [c["colour"] for c in gr["colours"]] == list(range(ncols)) and [c["sample"] for c in gr["colours"]] == samples + ["BrkpntRef"]
    assert [c.get("is_ref", False) for c in gr["colours"]] == [False] * (ncols - 1) + [True]
    assert gr["colours"][-1]["total_sequence"] == sum(c["length"] for c in contigs)
    cmd = hdr["commands"][0]
    assert cmd["breakpoints"] == {"min_ref_flank_kmers": prm[0], "max_ref_flank_kmers": prm[1], "load_ref_edges": prm[2], "ref_files": ref_files, "contigs": contigs}
    assert cmd["cmd"][:2] == ["mccortex%d" % maxk, "breakpoints"] and cmd["out_key"] == hdr["file_key"] and cmd["prev"] == []


@pytest.mark.gpu
def test_breakpoint1_fixture_through_the_command(built, tmp_path):
    k, d = 11, str(tmp_path)
    ref_fa, sample_fa = os.path.join(GOLDEN, "breakpoint1_ref.fa"), os.path.join(GOLDEN, "breakpoint1_sample.fa")
    ctx = os.path.join(d, "sample.ctx")
    build_graph(31, k, sample_fa, ctx, "sample")
    names, ref = fasta(ref_fa)
    _, sample = fasta(sample_fa)
    graph = R.build([[s.upper() for s in sample], []], k)
    out = os.path.join(d, "breakpoints.txt.gz")
    rc, so, err = run(31, "breakpoints", "-t", "1", "-m", "10M", "--minref", "5", "--seq", ref_fa, "--out", out, ctx)
    assert rc == 0 and so == b"", err[-800:]
    recs, text, stats, _, with_ref = B.call(graph, k, 2, ref, names, 5, 1000)
    hdr, body = split_file(gzip.open(out).read())
    assert body == text and stats["calls"] >= 7 and "  %d calls printed to" % stats["calls"] in err
    check_header(hdr, 31, k, 2, len(with_ref), ["sample"], (5, 1000, True), [os.path.realpath(ref_fa)],
                 [{"id": n, "length": len(s)} for n, s in zip(names, ref)])
    # the file is kept unless -f; -E; -R 0 is the default; stdout
    rc, so, err = run(31, "breakpoints", "-s", ref_fa, "-o", out, ctx)
    assert rc == 1 and "File already exists" in err
    rc, so, err = run(31, "breakpoints", "-q", "-E", "-r", "4", "-R", "0", "-1", ref_fa, ctx)
    assert rc == 0 and err == "", err[-800:]
    hdr, body = split_file(gzip.decompress(so))
    assert body == B.call(graph, k, 2, ref, names, 4, 1000, ref_edges=False)[1]
    assert hdr["commands"][0]["breakpoints"]["load_ref_edges"] is False and hdr["commands"][0]["breakpoints"]["max_ref_flank_kmers"] == 1000


@pytest.mark.gpu
def test_breakpoints_at_k97(mcx, tmp_path):
    """one run at keys of four words with two bits in the top one: three chromosomes, the sample built by mccortex127"""
    maxk, k, d = 127, 97, str(tmp_path)
    assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    case = next(c for c in BC.wide_cases() if c["name"] == "repeat_k%d" % k)
    rfa, sfa, ctx, out = (os.path.join(d, n) for n in ("ref.fa", "s.fa", "s.ctx", "o.txt.gz"))
    with open(rfa, "w") as f:
        f.write("".join(">%s\n%s\n" % (n, s) for n, s in zip(case["names"], case["ref"])))
    with open(sfa, "w") as f:
        f.write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(case["seqs"][0])))
    build_graph(maxk, k, sfa, ctx, "col0")
    rc, so, err = run(maxk, "breakpoints", "-o", out, "--seq", rfa, ctx)
    assert rc == 0 and so == b"", err[-800:]
    recs, text, stats, _, with_ref = BC.run(case)
    hdr, body = split_file(gzip.open(out).read())
    assert body == text and stats["calls"] > 0 and "  %d calls printed to" % stats["calls"] in err
    check_header(hdr, maxk, k, 2, len(with_ref), ["col0"], (5, 1000, True), [os.path.realpath(rfa)],
                 [{"id": n, "length": len(s)} for n, s in zip(case["names"], case["ref"])])


@pytest.mark.gpu
@pytest.mark.parametrize("maxk,k", [(31, 31), (63, 33)])
def test_two_seq_files_names_cleaned_and_colour_offsets(built, tmp_path, maxk, k):
    d = str(tmp_path)
    case = next(c for c in BC.cases() if c["name"] == "repeat_k%d" % k)  # three chromosomes, one sample colour
    two = next(c for c in BC.cases() if c["name"] == "twopaths_k%d" % k)  # two sample colours
    # the reference in two files; names with ',' ':' and a comment
    raw_names = ["one,a:b first chromosome", "two\tx", "three"]
    names = [B.clean_name(n) for n in raw_names]
    assert names == ["one.a;b", "two", "three"]
    fa1, fa2 = os.path.join(d, "ref1.fa"), os.path.join(d, "ref2.fa")
    with open(fa1, "w") as f:
        f.write(">%s\n%s\n>%s\n%s\n" % (raw_names[0], case["ref"][0], raw_names[1], case["ref"][1]))
    with open(fa2, "w") as f:
        f.write(">%s\n%s\n" % (raw_names[2], case["ref"][2]))
    sfa, ctx = os.path.join(d, "s.fa"), os.path.join(d, "s.ctx")
    with open(sfa, "w") as f:
        f.write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(case["seqs"][0])))
    build_graph(maxk, k, sfa, ctx, "col0")
    out = os.path.join(d, "o.txt.gz")
    for flags, edges in (([], True), (["-E"], False)):
        rc, so, err = run(maxk, "breakpoints", "-f", "-o", out, "--seq", fa1, "-s", fa2, *flags, ctx)
        assert rc == 0 and so == b"", err[-800:]
        recs, text, stats, _, with_ref = B.call(case["graph"], k, 2, case["ref"], names, 5, 1000, edges)
        hdr, body = split_file(gzip.open(out).read())
        assert body == text and stats["calls"] > 0 and "one.a;b:" in body
        check_header(hdr, maxk, k, 2, len(with_ref), ["col0"], (5, 1000, edges), [os.path.realpath(fa1), os.path.realpath(fa2)],
                     [{"id": n, "length": len(s)} for n, s in zip(names, case["ref"])])
    # two graph files at running colour offsets, the reference behind them
    files = []
    for c, seqs in enumerate(two["seqs"]):
        fa, cx = os.path.join(d, "t%d.fa" % c), os.path.join(d, "t%d.ctx" % c)
        with open(fa, "w") as f:
            f.write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
        build_graph(maxk, k, fa, cx, "col%d" % c)
        files.append(cx)
    rfa = os.path.join(d, "tref.fa")
    with open(rfa, "w") as f:
        f.write(">chr1\n%s\n" % two["ref"][0])
    rc, so, err = run(maxk, "breakpoints", "-q", "-r", "6", "-R", "900", "-s", rfa, files[0], "1:" + files[1])
    assert rc == 0 and err == "", err[-800:]
    recs, text, stats, _, with_ref = B.call(two["graph"], k, 3, two["ref"], two["names"], 6, 900)
    hdr, body = split_file(gzip.decompress(so))
    assert body == text and "cols=1\n" in body
    check_header(hdr, maxk, k, 3, len(with_ref), ["col0", "col1"], (6, 900, True), [os.path.realpath(rfa)], [{"id": "chr1", "length": len(two["ref"][0])}])
