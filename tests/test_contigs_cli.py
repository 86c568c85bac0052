"""`mccortex<K> contigs`: what is decided before a device is needed (the usage text, the option checks of
ctx_contigs.c:99-160 and this build's refusals, each with exit status 1 and nothing written), and one end-to-end run on
the GPU: build, thread, contigs, with the FASTA and the -S table equal to the restatement's."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import contigs_restate as G  # noqa: E402
import thread_restate as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")


def run(maxk, *args, cwd=None):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


@pytest.mark.parametrize("maxk", [31, 63])
def test_usage(built, maxk):
    rc, out, err = run(maxk, "contigs", "-h")
    assert rc == 1 and out == b""
    assert "usage: mccortex%d contigs [options] <in.ctx>" % maxk in err
    for opt in ("-o, --out <out.fa>", "-p, --paths <in.ctp>", "-N, --ncontigs <N>", "-s, --seed <in.fa>", "-r, --reseed", "-R, --no-reseed",
                "-G, --genome <G>", "-C, --confid-cumul <c>", "-T, --confid-step <c>", "-S, --confid-save <o.csv>", "-M, --no-missing-check", "--device <N>"):
        assert opt in err, opt


ERRORS = [
    (["-r", "-R", "-p", "x.ctp", "in.ctx"], "Cannot specify both -r and -R"),
    (["-r", "-p", "x.ctp", "in.ctx"], "Please specify one or more of: --no-reseed | --ncontigs | --seed <in.fa>"),
    (["-C", "1.5", "-p", "x.ctp", "in.ctx"], "-C, --confid-cumul must be 0 <= x <= 1"),
    (["-T", "2", "-p", "x.ctp", "in.ctx"], "-T, --confid-step must be 0 <= x <= 1"),
    (["-p", "x.ctp"], "Require input graph files (.ctx)"),
    (["-P", "-p", "x.ctp", "in.ctx"], "-P, --use-seed-paths: seeding with the links that no contig used is not part of this build"),
    (["-p", "x.ctp", "-p", "y.ctp", "in.ctx"], "-p, --paths <in.ctp> given twice"),
    (["-p", "x.ctp", "in.ctx", "in2.ctx"], "takes one graph file"),
    (["in.ctx"], "-p, --paths <in.ctp> is required"),
    (["-N", "3", "-N", "4", "-p", "x.ctp", "in.ctx"], "-N, --ncontigs given twice"),
    (["-o", "a.fa", "-o", "b.fa", "-p", "x.ctp", "in.ctx"], "-o, --out given twice"),
    (["--bogus", "in.ctx"], "contigs -h` for help. Bad option: --bogus"),
]


@pytest.mark.parametrize("args,msg", ERRORS)
def test_option_errors(built, tmp_path, args, msg):
    rc, out, err = run(31, "contigs", *args, cwd=str(tmp_path))
    assert rc == 1 and out == b"" and msg in err, err[-600:]
    assert os.listdir(str(tmp_path)) == []


def test_refusals_that_read_the_headers(built, tmp_path):
    """a .ctp of two colours, -c beyond the colours the graph file loads into, a .ctp of another k: each dies before a device is asked for"""
    import links_cases as LC
    ctx = os.path.join(ROOT, "tests", "golden", "tiny_k31.ctx")  # two colours
    two, one, k5 = (str(tmp_path / n) for n in ("two.ctp.gz", "one.ctp.gz", "k5.ctp.gz"))
    LC.ctp_file(two, 31, b"", ncols=2)
    LC.ctp_file(one, 31, b"")
    LC.ctp_file(k5, 5, b"")
    for args, msg in ((["-p", two, ctx], "takes a link file of one colour, this one has 2"), (["-c", "2", "-p", one, ctx], "-c, --colour 2: the graph file loads into 2 colours"),
                      (["-p", k5, ctx], "Kmer sizes don't match"), (["-o", two, "-p", one, ctx], "File already exists")):
        rc, out, err = run(31, "contigs", "--device", "99", *args)
        assert rc == 1 and out == b"" and msg in err, err[-600:]


def test_bench_tool_phases_from_profile_spans():
    """tools/bench_contigs.py folds the handle's profile dict {kernel: (calls, ms)} into its phases"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_contigs

    class Stub:
        def profile(self):
            return {"k_cg_walk": (3, 1.5), "k_cg_claim<false>": (1, 0.25), "k_cg_claim<true>": (1, 0.25), "k_cg_hits": (1, 0.5), "k_cg_text": (1, 2.0),
                    "radix_sort_pairs": (4, 9.0)}
    sp = bench_contigs.spans(Stub())
    assert sp["k_cg_claim"] == 0.5 and bench_contigs.phases_of(sp) == {"walks": 1.5, "resolve": 1.0, "text": 2.0}


@pytest.mark.gpu
def test_build_thread_contigs(built, tmp_path):
    build_thread_contigs(tmp_path, 31, 31)


@pytest.mark.gpu
def test_build_thread_contigs_k97(mcx, tmp_path):
    """the same at keys of four words with two bits in the top one"""
    assert os.path.exists(os.path.join(BIN, "mccortex127"))
    build_thread_contigs(tmp_path, 127, 97)


def build_thread_contigs(tmp_path, maxk, k):
    import random
    rng = random.Random(99)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    rep = rs(k + 12)
    gen = rs(300) + rep + rs(320) + rep + rs(300)
    n = max(250, 4 * k)  # (a read that spans the repeat and a k-mer on either side of it)
    reads = [gen[a:a + n] for a in range(0, len(gen) - n, 23)] + [gen[-n:]]
    d = str(tmp_path)
    fa = os.path.join(d, "reads.fa")
    with open(fa, "w") as f:
        f.write("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    ctx, ctp, out, csv = (os.path.join(d, n) for n in ("g.ctx", "l.ctp.gz", "contigs.fa", "conf.csv"))
    rc, _, err = run(maxk, "build", "-q", "-k", k, "--sample", "s", "--seq", fa, ctx)
    assert rc == 0, err[-800:]
    rc, _, err = run(maxk, "thread", "-q", "--seq", fa, "-o", ctp, ctx)
    assert rc == 0, err[-800:]
    rc, _, err = run(maxk, "contigs", "-o", out, "-p", ctp, "-S", csv, ctx)
    assert rc == 0, err[-800:]
    graph = R.build([reads], k)
    store = T.Store(graph, k).thread(reads)
    links = [(key, o, b, n) for (key, o, b), n in store.links.items()]
    conf = G.conf_table(dict(store.contig_hist()), len(graph))
    recs, seq, st = G.assemble(graph, k, links, conf)
    assert open(csv).read() == G.conf_csv(conf)
    assert open(out).read() == G.fasta(k, recs, seq)
    assert st["wlk_steps"][G.USELINKS] > 0 and "pulled out %d contigs" % st["contigs"] in err
    # the same through pieces of a few hundred bytes, with seeds and -N
    seeds = os.path.join(d, "seeds.fa")
    picks = [gen[10:10 + k], gen[400:400 + k], gen[10:10 + k]]
    with open(seeds, "w") as f:
        f.write("".join(">s%d\n%s\n" % (i, s) for i, s in enumerate(picks)))
    env = dict(os.environ, MCX_LINKS_PIECE="300")
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk), "contigs", "-q", "-f", "-o", out, "-p", ctp, "-s", seeds, "-r", "-N", "2", "-M", ctx],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert p.returncode == 0, p.stderr.decode()[-800:]
    recs, seq, st = G.assemble(graph, k, links, conf, flags=G.RESEED | G.NO_MISSING_CHECK, ncontigs=2, seeds=picks)
    assert open(out).read() == G.fasta(k, recs, seq) and st["contigs"] == 2
