"""`mccortex<K> inferedges`: the command-line contract of src/commands/ctx_infer_edges.c (CPU: every
case below dies while the arguments are checked, before a device is opened)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")


def run(maxk, *args):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63, 95, 127):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_inferedges_help_and_dispatcher(built, maxk):
    rc, _, err = run(maxk, "inferedges", "-h")
    assert rc == 1 and "usage: mccortex%d inferedges [options] <pop.ctx>" % maxk in err
    for opt in ("-P, --pop", "-A, --all", "-o, --out <out.ctx>", "-m, --memory <mem>", "-n, --nkmers <N>", "-D, --device <N>"):
        assert opt in err, opt
    rc, _, err = run(maxk)
    assert rc == 1 and "inferedges" in err
    assert "not part of this build" not in run(maxk, "inferedges", "-h")[2]


def test_inferedges_argument_errors(built, tmp_path):
    g = os.path.join(GOLD, "tiny_k31.ctx")
    cases = [
        (["--all", "--pop", g], "Please specify only one of --all --pop"),
        (["-P", "-A", g], "Please specify only one of --all --pop"),
        ([], "Expected exactly one graph file"),
        ([g, g], "Expected only one graph file. What is this: '%s'" % g),
        ([g + ":0"], "Cannot use ':' in input graph for `mccortex31 inferedges`"),
        ([str(tmp_path / "missing.ctx")], "Cannot open file: %s" % (tmp_path / "missing.ctx")),
        (["--bogus", g], "Bad option: --bogus"),
        (["-t", "0", g], "-t, --threads requires an int x > 0"),
        (["-D", "x", g], "-D, --device requires an int x >= 0: x"),
    ]
    for args, msg in cases:
        rc, out, err = run(31, "inferedges", *args)
        assert rc == 1, (args, err)
        assert msg in err, (args, err)
        assert "No MI355X" not in err, (args, err)  # (what opening a device prints on a machine without one)
        assert out == b""


def test_inferedges_output_exists_without_force(built, tmp_path):
    """an existing -o file is refused (futil_fopen_create) before anything is loaded"""
    out = tmp_path / "o.ctx"
    out.write_bytes(b"x")
    rc, _, err = run(31, "inferedges", "-o", str(out), os.path.join(GOLD, "tiny_k31.ctx"))
    assert rc == 1 and "File already exists: %s" % out in err
    assert out.read_bytes() == b"x"
