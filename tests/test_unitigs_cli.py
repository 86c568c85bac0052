"""`mccortex<K> unitigs`: the command-line contract of src/commands/ctx_unitigs.c.  Every case below ends while the
arguments and inputs are checked, before a device is opened."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
G31, G5 = os.path.join(GOLD, "tiny_k31.ctx"), os.path.join(GOLD, "tiny_k5.ctx")


def run(maxk, *args):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


@pytest.fixture(scope="module")
def built(mcx):
    for maxk in (31, 63, 95, 127):
        assert os.path.exists(os.path.join(BIN, "mccortex%d" % maxk))
    return True


@pytest.mark.parametrize("maxk", [31, 63, 95, 127])
def test_unitigs_help_and_dispatcher(built, maxk):
    for args in (["unitigs", "-h"], ["unitigs"]):
        rc, out, err = run(maxk, *args)
        assert rc == 1 and out == b""
        assert "usage: mccortex%d unitigs [options] <in.ctx> [<in2.ctx> ...]" % maxk in err
        assert "Print unitigs with k-1 bases of overlap." in err
        for opt in ("-o, --out <out.txt>   Save output graph file [default: STDOUT]", "-m, --memory <mem>", "-n, --nkmers <kmers>",
                    "-t, --threads <T>", "-F, --fasta           Print in FASTA format (default)",
                    "-g, --gfa             Print in Graphical Fragment Assembly (GFA) format",
                    "-d, --dot             Print in graphviz (DOT) format", "-P, --points          Used with --dot, print contigs as points",
                    "-D, --device <N>", "-f, --force", "-q, --quiet",
                    "e.g. mccortex%d unitigs --dot in.ctx | dot -Tpdf > in.pdf" % maxk):
            assert opt in err, opt
        assert "not part of this build" not in err
    rc, _, err = run(maxk)
    assert "unitigs     pull out unitigs in FASTA, DOT or GFA format" in err


def test_unitigs_argument_errors(built, tmp_path):
    exists = tmp_path / "out.fa"
    exists.write_bytes(b"keep")
    cases = [
        (["-P", G31], "--point is only for use with --dot"),            # -P with FASTA: the first of the two messages
        (["-g", "-P", G31], "--points only valid with --graphviz / --dot"),  # -P with GFA: the second
        (["-g", "-d", G31], "-d, --dot given twice"),                   # a second format option after a non-FASTA one
        (["-d", "-F", G31], "-F, --fasta given twice"),
        (["-g", "-g", G31], "-g, --gfa given twice"),
        (["-d", "-P", "-P", G31], "-P, --points given twice"),
        (["-f", "-f", G31], "-f, --force given twice"),
        (["-o", "a", "-o", "b", G31], "-o, --out given twice"),
        (["-t", "0", G31], "-t, --threads requires an int x > 0"),
        (["-t", "2", "-t", "3", G31], "-t, --threads given twice"),
        (["-m", "1G", "-m", "1G", G31], "-m, --memory <M> specifed more than once"),
        (["-n", "banana", G31], "Invalid hash size: banana"),
        (["-D", "x", G31], "-D, --device requires an int x >= 0: x"),
        (["--nosuchoption", G31], "unitigs -h` for help. Bad option: --nosuchoption"),
        ([str(tmp_path / "missing.ctx")], "missing.ctx"),
        ([G31, G5], "Kmer sizes don't match [31 vs 5]"),
        (["-F", "-F", G31, G5], "Kmer sizes don't match"),             # FASTA twice is let through (cmd_check(!syntax))
        (["-F", "-d", "-P", G31, G5], "Kmer sizes don't match"),
    ]
    for args, msg in cases:
        rc, out, err = run(31, "unitigs", *args)
        assert rc != 0 and msg in err and out == b"", (args, err)
    # an existing output is refused without -f, before a device is looked for, and left as it was
    rc, _, err = run(31, "unitigs", "-o", str(exists), G31)
    assert rc != 0 and "File already exists: %s" % exists in err
    assert exists.read_bytes() == b"keep"
    # the status line names the format and the destination (STDOUT by default)
    rc, _, err = run(31, "unitigs", "-g", "-o", str(exists), G31)
    assert rc != 0 and "Output in GFA format to %s" % exists in err
