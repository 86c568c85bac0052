"""Inputs for the `pjoin` tests, built on links_cases.py: its bodies with count columns of several colours, pairs of files
that share some of their links, and the small hand-written bodies that pin saturation and dropped lines."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import links_cases as LC  # noqa: E402


def recount(text, ncols, seed, zero=0.2, tags=True):
    """the body with every count column replaced by `ncols` counts: 0 with probability `zero`, all of a line with half of it (so some lines
    are dropped), otherwise 1..300 (so some saturate alone); tags=False also drops seq= and juncpos="""
    rng = random.Random(seed)
    out = []
    for ln in text.decode().split("\n")[:-1]:
        if ln[:1] in ("F", "R"):
            cols = ln.split(" ")
            none = rng.random() < zero / 2  # a line of zeros: it is dropped
            cols[2] = ",".join(str(0 if none or rng.random() < zero else rng.choice((1, 2, 3, 100, 254, 255, 256, 300))) for _ in range(ncols))
            ln = " ".join(cols if tags else cols[:4])
        out.append(ln)
    return ("\n".join(out) + "\n").encode()


def generated(k, nkmers, ncols, seed):
    """links_cases.generated with `ncols` counts a line"""
    return recount(LC.generated(k, nkmers, seed=seed), ncols, seed + 1000)


def second_word(k=33):
    """two k-mers that differ in their last base only (the second key word at k = 33), each with the same links"""
    stem = "ACGTTGCAGGCATCAGCATCGACTACGACTTCAGGCATC"[:k - 1]
    return ("%sA 2\nF 2 3 AC\nR 1 1 T\n%sC 2\nF 2 5 AC\nR 1 7 T\n" % (stem, stem)).encode()


def shared(text, seed):
    """two bodies out of one: every block goes to the first, the second or both (there with other counts), the blocks of
    the second in another order"""
    rng = random.Random(seed)
    a, b = [], []
    for blk in LC.blocks_of(text):
        r = rng.random()
        if r < 0.7:
            a.append(blk)
        if r > 0.3:
            b.append(recount(blk, 1, rng.randint(0, 1 << 30), zero=0.0))
    rng.shuffle(b)
    return b"".join(a), b"".join(b)


# ---- hand-written bodies (k = 5): the expected texts stand in golden/pjoin.json ----
SATURATION = {
    "200+100": ([b"ACGTA 1\nF 2 200 AC\n", b"ACGTA 1\nF 2 100 AC\n"], "0:"),
    "300": ([b"ACGTA 1\nF 2 300 AC\n"], "0:"),
    "255+0": ([b"ACGTA 1\nF 2 255,0 AC\n", b"ACGTA 1\nF 2 0,7 AC\n"], "cols"),
}
# the second k-mer has one link, whose picked colour counts 0: the line and the k-mer go
DROPPED = b"ACGTA 2\nF 1 4,0 C\nR 2 0,9 GT\nCCGTA 1\nF 3 0,2 ACG\n"
PREFIX = b"ACGTA 3\nF 3 1 ACG\nF 2 1 AC\nF 4 1 ACGT\n"
BOTH_WAYS = b"ACGTA 2\nR 2 6 AC\nF 2 5 AC\n"
TWO_BLOCKS = b"ACGTA 1\nF 1 2 A\nGGGTA 1\nF 1 1 T\nACGTA 2\nF 1 3 A\nR 1 1 C\n"
ALL_DROPPED = b"ACGTA 2\nF 1 0 C\nR 2 0 GT\n# nothing is left\nCCGTA 1\nF 3 0 ACG\n"

REFUSALS = [  # (body, src_ncols, refusal, the line it is on)
    (b"ACGTA 1\nF 1 3,4 C\nF 1 5 G\n", 2, "count_columns", 2),
    (b"ACGTA 1\nF 1 3,4 C\nF 1 5,6,7 G\n", 2, "count_columns", 2),
    (b"# first\nF 1 3 C\nACGTA 1\n", 1, "link_before_kmer", 1),
    (b"ACGTA 1\nX 1 3 C\n", 1, "bad_orient", 1),
    (b"ACGTA 1\nF x 3 C\n", 1, "bad_number", 1),
    (b"ACGTA 1\nF 1 3, C\n", 1, "bad_number", 1),
    (b"ACGTA 1\nF 1 3\n", 1, "bad_number", 1),
    (b"ACGTA 1\nF 1 3 N\n", 1, "bad_junction", 1),
    (b"ACGTA 1\nF 0 3 C\n", 1, "njuncs_range", 1),
    (b"ACGTA 1\nF 40000 3 C\n", 1, "njuncs_range", 1),
    (b"ACGTA 1\nF 2 3 C\n", 1, "njuncs_length", 1),
    (b"ACGTAC 1\nF 1 3 C\n", 1, "bad_kmer_line", 0),
    (b"ACGTA x\nF 1 3 C\n", 1, "bad_kmer_line", 0),
    (b"ACGTA 1\nF 1 3 C\nF 2 3 C\nX 1 3 C\n", 1, "njuncs_length", 2),  # the first bad line wins
]


def line_offset(body, line):
    return sum(len(x) + 1 for x in body.split(b"\n")[:line])
