"""`mccortex<K> clean`: the command-line contract of src/commands/ctx_clean.c (CPU: every case below ends while
the arguments are checked, before a device is opened) and the host's threshold picker against the restatement."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402

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
def test_clean_help_and_dispatcher(built, maxk):
    rc, _, err = run(maxk, "clean", "-h")
    assert rc == 1 and "usage: mccortex%d clean [options] <in.ctx> [in2.ctx ...]" % maxk in err
    for opt in ("-T[L], --tips[=L]", "-U[X], --unitigs[=X]", "-B, --fallback <T>", "-c, --covg-before <out.csv>",
                "-C, --covg-after <out.csv>", "-l, --len-before <out.csv>", "-L, --len-after <out.csv>", "-S, --sort",
                "-N, --ncols <N>"):
        assert opt in err, opt
    assert "not part of this build" not in err


def test_clean_argument_errors(built, tmp_path):
    g31, g5 = os.path.join(GOLD, "tiny_k31.ctx"), os.path.join(GOLD, "tiny_k5.ctx")
    exists = tmp_path / "out.ctx"
    exists.write_bytes(b"")
    cases = [
        ([], "Please give input graph files"),
        (["-T", g31], "Please specify --out <out.ctx> for cleaned graph"),
        (["--unitigs=2", g31], "Please specify --out <out.ctx> for cleaned graph"),
        (["-o", str(exists), g31], "Output file already exists: %s" % exists),
        (["-o", str(tmp_path / "new.ctx"), g31, g5], "Kmer sizes don't match [31 vs 5]"),
    ]
    for args, msg in cases:
        rc, _, err = run(31, "clean", *args)
        assert rc != 0 and msg in err, (args, err)
    # warnings come before the inputs are opened: a mixed-k pair ends the run right after them
    rc, _, err = run(31, "clean", "--fallback", "3", "-c", "-", g31, g5)
    assert rc != 0 and "-B, --fallback <T> without --unitigs" in err
    rc, _, err = run(31, "clean", "-C", str(tmp_path / "a.csv"), g31, g5)
    assert rc != 0 and "without any cleaning (set -U, --unitigs or -t, --tips)" in err
    # -f lets an existing output through to the next check
    rc, _, err = run(31, "clean", "-f", "-o", str(exists), g31, g5)
    assert rc != 0 and "Kmer sizes don't match" in err


def _host_pick():
    L = ctypes.CDLL(os.path.join(BIN, "libmcxhost.so"))
    L.cleaning_pick_kmer_threshold.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 4
    return lambda h: L.cleaning_pick_kmer_threshold(np.ascontiguousarray(h, dtype=np.uint64).ctypes.data, len(h),
                                                    None, None, None, None)


def test_threshold_picker_matches_restatement(built):
    pick = _host_pick()
    rng = np.random.default_rng(3)
    hists = []
    for depth in (5, 10, 20, 30, 60):  # errors at coverage 1-3 on top of a Poisson peak
        h = np.zeros(1000, dtype=np.uint64)
        h[1:] = np.bincount(np.minimum(rng.poisson(depth, 200000), 999), minlength=1000)[1:]
        h[1] += 400000
        h[2] += 60000
        h[3] += 8000
        hists.append(h)
    empty = np.zeros(1000, dtype=np.uint64)
    no_ones = hists[2].copy()
    no_ones[1] = 0
    low_kept = np.zeros(1000, dtype=np.uint64)  # nearly all coverage sits below any cutoff
    low_kept[1:4] = (10**6, 10**5, 10**4)
    low_kept[500] = 1
    picks = []
    for h in hists + [empty, no_ones, low_kept]:
        want = R.pick_threshold([int(x) for x in h])
        assert pick(h) == want
        picks.append(want)
    assert all(p > 1 for p in picks[:5])
    assert picks[5] == -1 and picks[7] == -1  # (kmer_covg[1] == 0 is compared above, whatever it gives)
