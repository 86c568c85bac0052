"""`mccortex<K> join`: the command-line contract of src/commands/ctx_join.c -- usage, every argument error with rc 1 and
nothing written, an existing output left alone; all of it before a device is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
G31, G5, G63 = (os.path.join(GOLD, n) for n in ("tiny_k31.ctx", "tiny_k5.ctx", "tiny_k63.ctx"))


def run(maxk, *args, cwd=None):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63, 95, 127):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_help_and_dispatcher(built, maxk):
    for args in (["join", "-h"], ["join"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d join [options] in1.ctx [[offset:]in2.ctx[:1,2,4-5] ...]" % maxk in err
        assert "Merge cortex graphs." in err
        for opt in ("-f, --force             Overwrite output files", "-o, --out <out.ctx>     Output file [required]",
                    "-m, --memory <mem>      Memory to use", "-n, --nkmers <kmers>    Number of hash table entries",
                    "-N, --ncols <c>         How many colours to load at once [default: 1]",
                    "-i, --intersect <a.ctx> Only load the kmers that are in graph A.ctx. Can be",
                    "-S, --sort              Output sorted graph file", "--device <N>", "-q, --quiet",
                    "Files can be specified with specific colours: samples.ctx:2,3",
                    "Offset specifies where to load the first colour: 3:samples.ctx"):
            assert opt in err, opt
        assert "not part of this build" not in err
    # the dispatcher's own texts are as they were; `view` stays unknown
    rc, _, err = run(maxk)
    assert rc == 1 and "hashtest    test hash table speed" in err and " join " not in err
    rc, _, err = run(maxk, "view", "x.ctx")
    assert rc == 1 and "command 'view' is not part of this build (build, sort, index, clean, inferedges, popbubbles, subgraph, unitigs, reads and hashtest are)" in err


def test_argument_errors(built, tmp_path):
    out = tmp_path / "never.ctx"
    cases = [
        ([G31], "--out <out.ctx> required"),
        (["-o", out], "Please specify at least one input graph file"),
        (["-o", out, "-o", out, G31], "-o, --out given twice"),
        (["-o", out, "-f", "-f", G31], "-f, --force given twice"),
        (["-o", out, "-S", "--sort", G31], "-S, --sort given twice"),
        (["-o", out, "-N", "1", "-N", "2", G31], "-N, --ncols given twice"),
        (["-o", out, "-N", "0", G31], "-N, --ncols requires an int x > 0"),
        (["-o", out, "-N", "x", G31], "-N, --ncols requires an int x > 0"),
        (["-o", out, "-m", "1G", "-m", "1G", G31], "-m, --memory <M> specifed more than once"),
        (["-o", out, "-m", "banana", G31], "Invalid memory argument: banana"),
        (["-o", out, "-n", "1M", "-n", "1M", G31], "-n, --nkmers <N> specifed more than once"),
        (["-o", out, "-n", "banana", G31], "Invalid hash size: banana"),
        (["-o", out, "--device", "x", G31], "--device requires an int x >= 0: x"),
        (["-o", out, "--nosuchoption", G31], "join -h` for help. Bad option: --nosuchoption"),
        (["-o", out, tmp_path / "missing.ctx"], "missing.ctx"),
        (["-o", out, "-i", tmp_path / "missing.ctx", G31], "missing.ctx"),
        (["-o", out, G31, G5], "Kmer sizes don't match [31 vs 5]"),
        (["-o", out, "-i", G5, G31], "Kmer sizes don't match [31 vs 5]"),
        (["-o", out, G31 + ":2"], "tiny_k31.ctx:2"),  # the file has colours 0 and 1
        (["-o", "-", "-N", "1", G31], "I need 2 colours if outputting to STDOUT (--ncols)"),
        (["-o", out, "-m", "1K", G31], "Not enough memory for requested graph: require at least"),
    ]
    for args, msg in cases:
        rc, so, err = run(31, "join", *args)
        assert rc == 1 and msg in err and so == b"", (args, rc, err)
        assert not out.exists(), args
    assert os.listdir(tmp_path) == []


def test_kmer_size_of_the_binary(built, tmp_path):
    out = tmp_path / "never.ctx"
    rc, so, err = run(31, "join", "-o", out, G63)
    assert rc == 1 and so == b"" and not out.exists() and "tiny_k63.ctx" in err
    rc, so, err = run(63, "join", "-o", out, G31)
    assert rc == 1 and so == b"" and not out.exists() and "tiny_k31.ctx" in err


def test_existing_output_is_left_alone(built, tmp_path):
    exists = tmp_path / "out.ctx"
    exists.write_bytes(b"keep")
    rc, so, err = run(31, "join", "-o", exists, G31)
    assert rc == 1 and so == b"" and "File already exists: %s" % exists in err
    assert exists.read_bytes() == b"keep"
    # the checks above come first even with -f and intersection graphs
    rc, so, err = run(31, "join", "-f", "-o", exists, "-i", G31 + ":0,1", G31, G5)
    assert rc == 1 and "Kmer sizes don't match [31 vs 5]" in err
    assert "Flattening intersection graph into colour 0: %s:0,1" % G31 in err
    assert exists.read_bytes() == b"keep"


def test_ncols_warning(built, tmp_path):
    exists = tmp_path / "out.ctx"
    exists.write_bytes(b"keep")
    rc, _, err = run(31, "join", "-N", "7", "-o", exists, G31)  # (stops at the existing output, after the warning)
    assert rc == 1 and "I only need 2 colours ('--ncols 7' ignored)" in err
    assert exists.read_bytes() == b"keep"
