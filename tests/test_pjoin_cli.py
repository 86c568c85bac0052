"""`mccortex<K> pjoin`: the command-line contract of src/commands/ctx_pjoin.c, everything that is decided before a device
is opened: the usage text, no inputs, no -o, options given twice, -c below what the inputs need, a bad colour filter, a
missing file, a file of format version 3, files of two k-mer sizes, sample names that clash, an existing output left alone."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import links_cases as LC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
BODY = b"ACGTA 1\nF 1 3 A seq=ACGTAA juncpos=0\n"


def run(maxk, *args, cwd=None):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300, cwd=cwd)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63, 95, 127):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


@pytest.fixture()
def files(tmp_path):
    a, b = str(tmp_path / "a.ctp.gz"), str(tmp_path / "b.ctp.gz")
    LC.ctp_file(a, 5, BODY, totals=(1, 1, 1))
    LC.ctp_file(b, 5, BODY, totals=(1, 1, 1))
    return a, b


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_usage(built, maxk):
    rc, out, err = run(maxk, "pjoin", "-h")
    assert rc == 1 and out == b""
    assert "is not part of this build" not in err
    assert "usage: mccortex%d pjoin [options] <in1.ctp.gz> [[offset:]in2.ctp[:0,2-4] ...]" % maxk in err
    assert "Merge cortex link files." in err
    for opt in ("-o, --out <out.ctp.gz> Output file [required]", "-m, --memory <mem>", "-n, --nkmers <nkmers>", "-t, --threads <T>", "-g, --graph <in.ctx>",
                "-c, --outcols <C>      How many 'colours' should the output file have", "-r, --noredundant      Accepted; changes nothing", "--device <N>",
                "Files can be specified with specific colours: samples.ctp:2,3", "Offset specifies where to load the first colour: 3:samples.ctp"):
        assert opt in err, opt


def test_argument_errors(built, files, tmp_path):
    a, b = files
    out = tmp_path / "out.ctp.gz"
    for args, msg in (
            (["-o", out], "Please specify at least one input file"),
            ([a, b], "--out <out.ctp.gz> required"),
            (["-o", out, "-o", out, a], "-o, --out given twice"),
            (["-f", "-f", "-o", out, a], "-f, --force given twice"),
            (["-r", "-r", "-o", out, a], "-r, --noredundant given twice"),
            (["-c", "2", "-c", "2", "-o", out, a], "-c, --outcols given twice"),
            (["-c", "0", "-o", out, a], "-c, --outcols requires an int x > 0"),
            (["-t", "0", "-o", out, a], "-t, --threads requires an int x > 0"),
            (["-m", "1G", "-m", "1G", "-o", out, a], "-m, --memory <M> specifed more than once"),
            (["-n", "x", "-o", out, a], "Invalid hash size: x"),
            (["-c", "1", "-o", out, a, b], "You specified --outcols 1 but inputs need at 2 colours")):
        rc, so, err = run(31, "pjoin", *args)
        assert rc == 1 and so == b"" and msg in err, (args, err)
        assert "usage: mccortex31 pjoin" in err
        assert not out.exists()


def test_refused_inputs(built, files, tmp_path):
    a, b = files
    out = tmp_path / "out.ctp.gz"
    rc, _, err = run(31, "pjoin", "-o", out, a, b + ":1")  # the file has one colour
    assert rc == 1 and "Invalid filter path: %s:1" % b in err
    rc, _, err = run(31, "pjoin", "-o", out, a, "0,1:" + b)  # two into colours for one
    assert rc == 1 and "Invalid filter path" in err
    rc, _, err = run(31, "pjoin", "-o", out, a, tmp_path / "nothing.ctp.gz")
    assert rc == 1 and "Cannot open file: %s" % (tmp_path / "nothing.ctp.gz") in err
    v3 = str(tmp_path / "v3.ctp.gz")
    LC.ctp_file(v3, 5, BODY, version=3)
    rc, _, err = run(31, "pjoin", "-o", out, a, v3)
    assert rc == 1 and "Only link files of format version 4 are read, this one has version 3" in err
    k7 = str(tmp_path / "k7.ctp.gz")
    LC.ctp_file(k7, 7, b"ACGTACG 1\nF 1 3 A\n", totals=(1, 1, 1))
    rc, _, err = run(31, "pjoin", "-o", out, a, k7)
    assert rc == 1 and "Kmer-size doesn't match between files [5 vs 7]: %s" % k7 in err
    two = str(tmp_path / "two.ctp.gz")  # colour 1 is another sample than colour 0 of a
    LC.ctp_file(two, 5, b"ACGTA 1\nF 1 3,1 A\n", ncols=2, totals=(1, 1, 1))
    rc, _, err = run(31, "pjoin", "-o", out, a, "0:" + two + ":1")
    assert rc == 1 and "Graph/path sample names do not match [1->0]" in err
    assert not out.exists()


def test_existing_output_is_left_alone(built, files, tmp_path):
    a, b = files
    out = tmp_path / "out.ctp.gz"
    out.write_bytes(b"mine")
    rc, _, err = run(31, "pjoin", "-o", out, a, b)
    assert rc == 1 and "File already exists: %s" % out in err
    assert out.read_bytes() == b"mine"


def test_bench_tool_files_are_what_pjoin_and_links_take():
    """tools/bench_pjoin.py: its synthetic bodies parse under the restatements of both commands, and files share links"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_pjoin
    import links_restate as LR
    import pjoin_restate as PR
    files = bench_pjoin.make_files(3, 4000, 12, 0.5)
    r = PR.Pjoin(31, 3)
    kept = 0
    for c, (plain, tagged) in enumerate(files):
        ps = r.add(plain, 1, [(0, c)])
        assert ps["links_kept"] == ps["link_lines"] > 20 and ps["kmers_n_mismatch"] == 0
        kept += ps["links_kept"]
        assert LR.links(tagged, 31)[2]["links_in"] == ps["link_lines"]
    assert 0 < r.info()["num_paths"] < kept  # some links are in two files
