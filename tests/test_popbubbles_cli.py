"""`mccortex<K> popbubbles`: the command-line contract of src/commands/ctx_pop_bubbles.c, and replays of the reference's
tests/pop_bubbles/pop_bubbles1 and pop_bubbles2 (golden/pop_bubbles.json) on the device."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import pop_cases as P  # noqa: E402
import pop_restate as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
G31, G5 = os.path.join(GOLD, "tiny_k31.ctx"), os.path.join(GOLD, "tiny_k5.ctx")


def run(maxk, *args):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63, 95, 127):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_help_and_dispatcher(built, maxk):
    for args in (["popbubbles", "-h"], ["popbubbles"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d popbubbles [options] <in.ctx> [in2.ctx ...]" % maxk in err
        assert "Pop bubbles in the graph. All graphs are loaded and treated as one colour" in err
        for opt in ("-o, --out <out.ctx>   Output file [required]", "-m, --memory <mem>", "-n, --nkmers <kmers>", "-t, --threads <T>",
                    "-C, --max-covg <C>    Only remove branches whose mean coverage is less than <C>",
                    "-L, --max-len <L>     Only remove branches whose lengths are less than <L> kmers",
                    "-D, --max-diff <D>    Only pop bubbles whose branch lengths are within <D> kmers", "-S, --sort", "--device <N>",
                    "-f, --force", "-q, --quiet"):
            assert opt in err, opt
        assert "not part of this build" not in err
    rc, _, err = run(maxk)
    assert "popbubbles  pop bubbles in the population graph" in err
    rc, _, err = run(maxk, "view", "x.ctx")
    assert "not part of this build" in err and "popbubbles" in err


def test_argument_errors(built, tmp_path):
    exists = tmp_path / "out.ctx"
    exists.write_bytes(b"keep")
    cases = [
        ([], "Require input graph files (.ctx)"),
        (["-o", "a", "-o", "b", G31], "-o, --out given twice"),
        (["-f", "-f", G31], "-f, --force given twice"),
        (["-t", "0", G31], "-t, --threads requires an int x > 0"),
        (["-t", "2", "-t", "3", G31], "-t, --threads given twice"),
        (["-m", "1G", "-m", "1G", G31], "-m, --memory <M> specifed more than once"),
        (["-n", "banana", G31], "Invalid hash size: banana"),
        (["-C", "1", "-C", "2", G31], "-C, --max-covg given twice"),
        (["-L", "1", "--max-len", "2", G31], "-L, --max-len given twice"),
        (["-D", "0", "-D", "0", G31], "-D, --max-diff given twice"),
        (["-C", "x", G31], "-C, --max-covg requires an int x >= 0: x"),
        (["-D", "-1", G31], "-D, --max-diff requires an int x >= 0: -1"),
        (["-S", "-S", G31], "-S, --sort given twice"),
        (["--device", "x", G31], "--device requires an int x >= 0: x"),
        (["--nosuchoption", G31], "popbubbles -h` for help. Bad option: --nosuchoption"),
        ([str(tmp_path / "missing.ctx")], "missing.ctx"),
        ([G31, G5], "Kmer sizes don't match [31 vs 5]"),
    ]
    for args, msg in cases:
        rc, out, err = run(31, "popbubbles", *args)
        assert rc != 0 and msg in err and out == b"", (args, err)
    # an existing output is refused without -f, before a device is looked for, and left as it was
    rc, _, err = run(31, "popbubbles", "-o", str(exists), G31)
    assert rc != 0 and "File already exists: %s" % exists in err
    assert exists.read_bytes() == b"keep"


# ---- on the device ---------------------------------------------------------------------------------------------------
def ctx_body(buf, k, ncols):
    from oracle import ctxio
    hdr, size = ctxio.read_header(buf)
    assert hdr["kmer_size"] == k and hdr["num_cols"] == ncols
    return hdr, buf[size:]


def build_ctx(tmp, maxk, k, sample, seqs):
    fa = tmp / (sample + ".fa")
    fa.write_text("".join("%s\n" % s for s in seqs))
    out = tmp / (sample + ".ctx")
    rc, _, err = run(maxk, "build", "-q", "-k", k, "--sample", sample, "--seq", fa, out)
    assert rc == 0, err
    return out


def truth_keys(k, seqs):
    return set(R.build([[s.upper() for s in seqs]], k))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pop_bubbles1", "pop_bubbles2"])
def test_reference_replays(built, tmp_path, name):
    gold = P.golden()
    k, case = gold["kmer_size"], gold[name]
    inputs = [build_ctx(tmp_path, 31, k, inp["sample"], inp["seqs"]) for inp in case["inputs"]]
    ncols = len(inputs)
    graph = R.build([[s.upper() for s in inp["seqs"]] for inp in case["inputs"]], k)
    exp, popped, nremoved = PR.pop(graph, k)
    assert popped >= 1
    out = tmp_path / "popped.ctx"
    rc, so, err = run(31, "popbubbles", "--sort", "--out", out, *inputs)
    assert rc == 0 and so == b"", err
    hdr, body = ctx_body(out.read_bytes(), k, ncols)
    assert set(R.parse(body, k, ncols)) == truth_keys(k, case["truth"])
    assert body == R.pack(exp, k, ncols)
    for line in ("Popping bubbles...", "Popped %d bubbles" % popped,
                 "Number of kmers %d -> %d (-%d)" % (len(graph), len(exp), nremoved)):
        assert line in err, line
    assert [gi.sample_name for gi in hdr["ginfo"]] == [inp["sample"] for inp in case["inputs"]]
    assert not any(gi.cleaning.cleaned_tips or gi.cleaning.cleaned_unitigs for gi in hdr["ginfo"])  # popping sets no flag
    # to STDOUT by default, quietly, unsorted: the same records
    rc, so, err = run(31, "popbubbles", "-q", *inputs)
    assert rc == 0 and err == ""
    _, body2 = ctx_body(so, k, ncols)
    rs = 8 + 5 * ncols
    assert sorted(body2[i:i + rs] for i in range(0, len(body2), rs)) == sorted(body[i:i + rs] for i in range(0, len(body), rs))
    # an existing output is overwritten with -f; the losing branch (mean 1, k k-mers, equal lengths) passes -C 1 -L k -D 0
    rc, _, err = run(31, "popbubbles", "-q", "-f", "--sort", "-C", "1", "-L", k, "-D", "0", "-o", out, *inputs)
    assert rc == 0 and ctx_body(out.read_bytes(), k, ncols)[1] == body
    # and does not pass -L k-1: the graph comes out as it went in
    rc, _, err = run(31, "popbubbles", "-q", "-f", "--sort", "-L", k - 1, "-o", out, *inputs)
    assert rc == 0 and ctx_body(out.read_bytes(), k, ncols)[1] == R.pack(graph, k, ncols)


@pytest.mark.gpu
def test_mccortex63_at_k33(built, tmp_path):
    import random
    k = 33
    rng = random.Random(12)
    left, right = P.rseq(rng, 70), P.rseq(rng, 70)
    seqs = [left + "A" + right] * 3 + [left + "C" + right]
    raw = build_ctx(tmp_path, 63, k, "s", seqs)
    graph = R.build([seqs], k)
    exp, popped, nremoved = PR.pop(graph, k)
    assert popped >= 1 and nremoved == k
    out = tmp_path / "p.ctx"
    rc, _, err = run(63, "popbubbles", "-S", "-o", out, raw)
    assert rc == 0, err
    assert ctx_body(out.read_bytes(), k, 1)[1] == R.pack(exp, k, 1)
