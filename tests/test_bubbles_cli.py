"""`mccortex<K> bubbles`: what is decided before a device is needed (the usage text, the option checks of
ctx_bubbles.c:86-147 and this build's refusal of -p, each with exit status 1 and nothing written; the ABI symbol and the
wrapper), and end-to-end runs on the GPU: graphs built from the sequences of bubbles_cases.py, one file per colour,
joined on the command line with colour offsets, with the header's fields, the body byte for byte and the status counts
equal to the restatement's."""
import gzip
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bubbles_cases as BC  # noqa: E402
import bubbles_restate as B  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
COMMENT = ("\n# This file was generated with McCortex\n#   written by Isaac Turner <turner.isaac@gmail.com>\n#   url: https://github.com/mcveanlab/mccortex\n"
           "# \n# Comment lines begin with a # and are ignored, but must come after the header\n\n")


def run(maxk, *args, cwd=None):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


def test_abi_symbol_and_wrapper(mcx):
    assert hasattr(mcx.lib(), "mcx_graph_bubbles")
    assert callable(mcx.Graph.bubbles)
    assert tuple(n for n, _ in mcx.graph.BubblesStats._fields_) == B.STAT_NAMES and set(mcx.graph.BubblesStats().as_dict()) == set(B.STAT_NAMES)
    assert mcx.graph.BUBBLE_REC.itemsize == 64


@pytest.mark.parametrize("maxk", [31, 63])
def test_usage(built, maxk):
    rc, out, err = run(maxk, "bubbles", "-h")
    assert rc == 1 and out == b""
    assert "usage: mccortex%d bubbles [options] <in.ctx> [in2.ctx ...]" % maxk in err
    for opt in ("-o, --out <bub.txt.gz>", "-p, --paths <in.ctp>", "-H, --haploid <col>", "-A, --max-allele <len>  Max bubble branch length in kmers [default: 2000]",
                "-F, --max-flank <len>   Max flank length in kmers [default: 500]", "-S, --keep-serial ", "-t, --threads <T>", "--device <N>"):
        assert opt in err, opt


ERRORS = [
    ([], "Require input graph files (.ctx)"),
    (["-o", "x.bub.gz"], "Require input graph files (.ctx)"),
    (["-p", "x.ctp", "in.ctx"], "-p, --paths <in.ctp>: link files are not part of this build"),
    (["-A", "0", "in.ctx"], "-A, --max-allele requires an int x > 0: 0"),
    (["-F", "x", "in.ctx"], "-F, --max-flank requires an int x > 0: x"),
    (["-A", "3", "-A", "4", "in.ctx"], "-A, --max-allele given twice"),
    (["-S", "-S", "in.ctx"], "-S, --keep-serial given twice"),
    (["-H", "0", "-H", "1", "in.ctx"], "-H, --haploid given twice"),
    (["-o", "a.gz", "-o", "b.gz", "in.ctx"], "-o, --out given twice"),
    (["--bogus", "in.ctx"], "bubbles -h` for help. Bad option: --bogus"),
    (["-o", "x.bub.gz", "missing.ctx"], "missing.ctx"),
]


@pytest.mark.parametrize("args,msg", ERRORS)
def test_option_errors(built, tmp_path, args, msg):
    rc, out, err = run(31, "bubbles", *args, cwd=str(tmp_path))
    assert rc == 1 and out == b"" and msg in err, err[-600:]
    assert os.listdir(str(tmp_path)) == []


def test_bad_haploid_list_and_existing_output(built, tmp_path):
    """the checks that read the graph headers: each dies before a device is asked for"""
    ctx = os.path.join(ROOT, "tests", "golden", "tiny_k31.ctx")  # two colours
    out = tmp_path / "have.bub.txt.gz"
    out.write_bytes(b"")
    for args, msg in ((["-H", "2", ctx], "Invalid haploid colour list: 2"), (["-H", "0,x", ctx], "Invalid haploid colour list: 0,x"),
                      (["-H", "1-", ctx], "Invalid haploid colour list: 1-"), (["-o", out, ctx], "File already exists")):
        rc, so, err = run(31, "bubbles", "--device", "99", *args)
        assert rc == 1 and so == b"" and msg in err, err[-600:]
    assert out.read_bytes() == b""


def test_bench_tool_phases_from_profile_spans():
    """tools/bench_bubbles.py folds the handle's profile dict {kernel: (calls, ms)} into its passes"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_bubbles

    class Stub:
        def profile(self):
            return {"k_bb_forks": (1, 1.0), "k_bb_forklist": (1, 0.5), "radix_sort_pairs": (2, 3.0), "k_bb_walk_count": (2, 1.0), "k_bb_walk_write": (2, 2.0),
                    "k_bb_first": (2, 0.5), "k_bb_group<false>": (2, 0.25), "k_bb_group<true>": (2, 0.25), "k_bb_size": (2, 0.125), "k_bb_emit": (4, 4.0),
                    "k_cl_links": (1, 7.0)}
    ph = bench_bubbles.phases_of(bench_bubbles.spans(Stub()))
    assert ph == {"forks": 1.5, "walk": 3.0, "group": 1.0, "size": 0.125, "emit": 4.0}


def split_file(raw):
    text = raw.decode()
    at = text.index(COMMENT)
    return json.loads(text[:at]), text[at + len(COMMENT):]


def colour_files(case, d, maxk):
    """one graph file per colour, built by the `build` command from the case's sequences"""
    paths = []
    for c, seqs in enumerate(case["seqs"]):
        fa, ctx = os.path.join(d, "c%d.fa" % c), os.path.join(d, "c%d.ctx" % c)
        with open(fa, "w") as f:
            f.write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
        rc, _, err = run(maxk, "build", "-q", "-k", case["k"], "--sample", "col%d" % c, "--seq", fa, ctx)
        assert rc == 0, err[-800:]
        paths.append(ctx)
    return paths


def counts_in(err, stats):
    return all(s in err for s in ("Bubble Caller called %d bubbles" % stats["bubbles"], "Haploid bubbles dropped: %d" % stats["haploid_dropped"],
                                  "Serial bubbles dropped: %d" % stats["serial_dropped"]))


@pytest.mark.gpu
@pytest.mark.parametrize("maxk,k", [(31, 11), (31, 31), (63, 33)])
def test_bubbles_of_joined_colour_files(built, tmp_path, maxk, k):
    d = str(tmp_path)
    case = next(c for c in BC.cases() if c["name"] == "snp_k%d" % k)
    files = colour_files(case, d, maxk)
    args = [files[0]] + ["%d:%s" % (i, p) for i, p in enumerate(files) if i]
    out = os.path.join(d, "calls.bub.txt.gz")
    # -A, -F and a haploid colour; output to a file
    rc, so, err = run(maxk, "bubbles", "-o", out, "-H", "1", "-A", "100", "-F", "5", "-t", "2", *args)
    assert rc == 0 and so == b"", err[-800:]
    recs, text, stats, _ = B.call(case["graph"], k, case["ncols"], 100, 5, (1,))
    hdr, body = split_file(gzip.open(out).read())
    assert body == text and stats["bubbles"] > 0 and counts_in(err, stats)
    assert hdr["file_format"] == "CtxBubbles" and hdr["format_version"] == 2 and len(hdr["file_key"]) == 16
    gr = hdr["graph"]
    assert (gr["num_colours"], gr["kmer_size"], gr["num_kmers_in_graph"]) == (case["ncols"], k, len(case["graph"]))
    assert [c["colour"] for c in gr["colours"]] == list(range(case["ncols"])) and [c["sample"] for c in gr["colours"]] == ["col%d" % i for i in range(case["ncols"])]
    cmd = hdr["commands"][0]
    assert cmd["bubbles"] == {"max_flank_kmers": 5, "max_allele_kmers": 100, "haploid_colours": [1]}
    assert cmd["cmd"][:2] == ["mccortex%d" % maxk, "bubbles"] and cmd["out_key"] == hdr["file_key"] and cmd["prev"] == []
    # the file is kept unless -f; -o - is stdout; -H '*'
    rc, so, err = run(maxk, "bubbles", "-o", out, *args)
    assert rc == 1 and "File already exists" in err
    rc, so, err = run(maxk, "bubbles", "-q", "-o", "-", "-H", "*", "-A", "100", "-F", "5", *args)
    assert rc == 0 and err == "", err[-800:]
    hdr, body = split_file(gzip.decompress(so))
    assert body == B.call(case["graph"], k, case["ncols"], 100, 5, tuple(range(case["ncols"])))[1]
    assert hdr["commands"][0]["bubbles"]["haploid_colours"] == list(range(case["ncols"]))


@pytest.mark.gpu
def test_bubbles_at_k97(mcx, tmp_path):
    """one run at keys of four words with two bits in the top one: colour files built and joined by mccortex127"""
    maxk, k, d = 127, 97, str(tmp_path)
    assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    case = next(c for c in BC.wide_cases() if c["name"] == "snp_k%d" % k)
    files = colour_files(case, d, maxk)
    out = os.path.join(d, "calls.bub.txt.gz")
    rc, so, err = run(maxk, "bubbles", "-o", out, "-H", "1", "-A", "300", "-F", "5", files[0], *["%d:%s" % (i, p) for i, p in enumerate(files) if i])
    assert rc == 0 and so == b"", err[-800:]
    recs, text, stats, _ = B.call(case["graph"], k, case["ncols"], 300, 5, (1,))
    hdr, body = split_file(gzip.open(out).read())
    assert body == text and stats["bubbles"] > 0 and counts_in(err, stats)
    gr = hdr["graph"]
    assert (gr["num_colours"], gr["kmer_size"], gr["num_kmers_in_graph"]) == (case["ncols"], k, len(case["graph"]))
    assert hdr["commands"][0]["cmd"][:2] == ["mccortex%d" % maxk, "bubbles"]


@pytest.mark.gpu
def test_keep_serial_haploid_drop_and_defaults(built, tmp_path):
    k = 31
    d = str(tmp_path)
    out = os.path.join(d, "o.bub.txt.gz")
    case = next(c for c in BC.cases() if c["name"] == "serial_k%d" % k)
    sub = os.path.join(d, "serial")
    os.mkdir(sub)
    files = colour_files(case, sub, 31)
    args = [files[0], "1:" + files[1]]
    for flags, keep in (([], False), (["-S"], True), (["--keep-serial"], True)):
        rc, _, err = run(31, "bubbles", "-f", "-o", out, *flags, *args)
        assert rc == 0, err[-800:]
        recs, text, stats, _ = B.call(case["graph"], k, 2, 2000, 500, (), keep)
        hdr, body = split_file(gzip.open(out).read())
        assert body == text and counts_in(err, stats) and (stats["serial_dropped"] == 0) == keep
        assert hdr["commands"][0]["bubbles"] == {"max_flank_kmers": 500, "max_allele_kmers": 2000, "haploid_colours": []}
    case = next(c for c in BC.cases() if c["name"] == "haploid_k%d" % k)
    sub = os.path.join(d, "haploid")
    os.mkdir(sub)
    files = colour_files(case, sub, 31)
    for hap in ((), (0,)):
        rc, _, err = run(31, "bubbles", "-f", "-o", out, *(["-H", "0"] if hap else []), files[0], "1:" + files[1])
        assert rc == 0, err[-800:]
        recs, text, stats, _ = B.call(case["graph"], k, 2, 2000, 500, hap)
        assert split_file(gzip.open(out).read())[1] == text and counts_in(err, stats) and (stats["haploid_dropped"] > 0) == bool(hap)
