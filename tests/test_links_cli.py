"""`mccortex<K> links`: the command-line contract of src/commands/ctx_links.c, everything that is decided before a
device is needed: the usage text, each argument error of ctx_links.c:156-195 with exit status 1 and nothing written,
options given twice, -P refused, -T refused with too small a matrix, an existing output left alone, a header of two
colours and one of format version 3 refused."""
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
def ctp(tmp_path):
    p = str(tmp_path / "in.ctp.gz")
    LC.ctp_file(p, 5, BODY, totals=(1, 1, 1))
    return p


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_usage(built, maxk):
    for args in (["links", "-h"], ["links"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d links [options] <in.ctp.gz>" % maxk in err
        assert "Clean, minimise and list cortex links. Works on a stream of input only," in err
        for opt in ("-o,--out <out.ctp.gz>   Save output link file [default: STDOUT]", "-L,--limit <N>          Only use links from first N kmers",
                    "-l,--list <out.txt>     List as CSV links", "-P,--plot <out.dot>     Plot last from limit",
                    "-c,--clean <N>          Remove junction choices with coverage < N", "-T,--threshold <t.txt>  Calculate the cleaning threshold, write to file",
                    "-H,--covg-hist <f.csv>  Write link coverage matrix to a csv file", "-D,--max-dist <max>     Set max dist when using --covg-hist ...",
                    "-C,--max-covg <max>     Set max covg when using --covg-hist ...", "--device <N>"):
            assert opt in err, opt
    assert ("Wrong number of arguments" in err)


ERRORS = [
    (["-D", "4", "-l", "l.csv"], "--max-dist without --covg-hist"),
    (["-C", "40", "-l", "l.csv"], "--max-covg without --covg-hist"),
    (["-l", "l.csv"], "Wrong number of arguments"),
    (["-l", "l.csv", "IN", "IN"], "Wrong number of arguments"),
    (["-c", "3", "IN"], "Need to give --out <out.ctp.gz> with --clean"),
    (["-L", "3", "IN"], "Please specify one of --plot, --list or --clean"),
    (["-o", "-", "-T", "t.txt", "IN"], "Outputing both cleaning threshold (-T) and links (-o) to STDOUT!"),
    (["-o", "-", "-H", "h.csv", "IN"], "Outputing both cleaning threshold (-T) and links (-o) to STDOUT!"),
    (["-c", "x", "-o", "o.ctp.gz", "IN"], "-c, --clean requires an int x >= 0: x"),
    (["-L", "-1", "-l", "l.csv", "IN"], "-L, --limit requires an int x >= 0: -1"),
    (["-H", "h.csv", "-D", "two", "IN"], "-D, --max-dist requires an int x >= 0: two"),
    (["--device", "x", "-l", "l.csv", "IN"], "--device requires an int x >= 0: x"),
    (["-o", "a", "-o", "b", "IN"], "-o, --out given twice"), (["-f", "-f", "-l", "l.csv", "IN"], "-f, --force given twice"),
    (["-l", "a", "--list", "b", "IN"], "-l, --list given twice"), (["-c", "2", "-c", "3", "-o", "o", "IN"], "-c, --clean given twice"),
    (["-L", "2", "-L", "3", "-l", "l", "IN"], "-L, --limit given twice"), (["-T", "a", "-T", "b", "IN"], "-T, --threshold given twice"),
    (["-H", "a", "-H", "b", "IN"], "-H, --covg-hist given twice"), (["-H", "a", "-C", "20", "-C", "30", "IN"], "-C, --max-covg given twice"),
    (["-H", "a", "-D", "7", "--max-dist", "8", "IN"], "-D, --max-dist given twice"),
    (["-P", "p.dot", "IN"], "-P, --plot <out.dot> is not part of this build's `links`"),
    (["-T", "t.txt", "-H", "h.csv", "-D", "5", "IN"], "-D, --max-dist <max> must be at least 6"),
    (["-T", "t.txt", "-H", "h.csv", "-C", "9", "IN"], "-C, --max-covg <max> must be at least 10"),
    (["--nonsense", "IN"], "`mccortex31 links -h` for help. Bad option: --nonsense"),
]


@pytest.mark.parametrize("i", range(len(ERRORS)))
def test_argument_errors(built, ctp, tmp_path, i):
    args, msg = ERRORS[i]
    before = sorted(os.listdir(tmp_path))
    rc, out, err = run(31, "links", *[ctp if a == "IN" else a for a in args], cwd=str(tmp_path))
    assert rc == 1 and out == b"" and msg in err, err
    assert sorted(os.listdir(tmp_path)) == before  # nothing written


def test_existing_outputs_are_kept(built, ctp, tmp_path):
    for opt in ("-l", "-o", "-T", "-H"):
        keep = tmp_path / ("keep" + opt)
        keep.write_text("mine")
        extra = ["-o", str(tmp_path / "other.ctp.gz")] if opt != "-o" else []
        rc, out, err = run(31, "links", opt, str(keep), *extra, ctp)
        assert rc == 1 and "File already exists: %s" % keep in err and "Use -f,--force to overwrite files" in err
        assert keep.read_text() == "mine" and not (tmp_path / "other.ctp.gz").exists()


def test_headers_refused_before_a_device(built, tmp_path):
    two, v3, notctp, k7 = (str(tmp_path / n) for n in ("two.ctp.gz", "v3.ctp.gz", "not.ctp.gz", "k7.ctp.gz"))
    LC.ctp_file(two, 5, BODY, ncols=2)
    LC.ctp_file(v3, 5, BODY, version=3)
    LC.ctp_file(k7, 7, BODY)
    with open(notctp, "wb") as f:
        f.write(b"ACGTA 1\n")
    env_free = dict(os.environ, HIP_VISIBLE_DEVICES="")
    for path, msg, maxk in ((two, "Can only clean a single colour at a time. Sorry.", 31), (v3, "Only link files of format version 4 are read, this one has version 3", 31),
                            (notctp, "Expected JSON header", 31), (k7, "kmer size 7 is not an odd number within 33..63", 63),
                            (str(tmp_path / "none.ctp.gz"), "Cannot open file", 31)):
        p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk), "links", "-l", str(tmp_path / "l.csv"), "-o", str(tmp_path / "o.ctp.gz"), path],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env_free)
        assert p.returncode == 1 and msg in p.stderr.decode(), p.stderr.decode()
        assert not (tmp_path / "l.csv").exists() and not (tmp_path / "o.ctp.gz").exists()
