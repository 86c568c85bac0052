"""The cases of the `breakpoints` tests, built on the CPU and shared by test_breakpoints_restate.py (which asserts that they
reach every rule named there), test_gpu_breakpoints.py (which runs them on the device) and test_breakpoints_cli.py.  Small
graphs at k = 11, 31 and 33 (keys of one and two words): a reference of one to three chromosomes and one or two sample
colours; the reference colour is the last one and is empty before the call.  min_ref is 5 unless a case says otherwise.
tests/golden/breakpoints.json pins these by name.  wide_cases() is the same structures at k = 63, 65, 95, 97 and 127 (keys
of two, three and four words, the top word full or holding two bits; up to 675 k-mers), which no golden pins: there the
device is compared with the restatement alone.

Structures (upper-case names are random stretches without a repeated k-mer, a b c d are single bases that differ; M is
min_ref):
  equal      ref L R, sample L R: no break.
  refbubble  ref L a R L b R (the reference holds its own SNP bubble), sample the same: no call.
  snp        ref L a R, sample L b R: a call from either side; flank3pidx = k.  `snp_maxref` is the same with max_ref 8:
             every walk stops on the length of its run.
  insertion  ref L R, sample L X R.    deletion   ref L X R, sample L R (flank3pidx = k - 1, the path line is empty).
  microhom   ref L R[:2] Y R, sample L R: the deleted stretch starts with the two bases that follow it, so flank3pidx < k - 1.
  twosnps    ref L a R c T, sample L b R d T: the walks that start at one SNP stop where their run ends at the other.
  junction   ref A and B, sample A[:h] B[h:]: the flanks lie on two chromosomes.
  ends       ref L and R, sample L R: the fork node is the last k-mer of a chromosome and has one successor.
  inversion  ref L M R, sample L rc(M) R: runs on the - strand in an allele walk.
  repeat     ref A P B, C P D and E F with P of M + 3 k-mers, sample A' P B' (a SNP early in A, one late in B) and
             E X P B: runs on two chromosomes picked up at one node, one of which ends; two runs at one qoffset (the
             sort's tie-break).  `repeat_exact`: P of exactly M k-mers; the run that ends is not kept, on a flank and on
             an allele.
  exact      ref L a R without its edges, sample L[-(k-1+M):] b R[:k-1+M]: runs of exactly M k-mers still active when the
             walks end are kept.  With the reference's edges (`exact_edges`) the walks go on along the reference.
  lost       ref L R, sample Z R[3:k+5] X: a 5' walk whose only run ends with 3 k-mers gives no flank.
  tail       ref L R, sample L X with X long: an allele that never meets the reference again.
  twosucc    ref L a R, samples L b R | L c R: a fork node with two non-reference successors.
  merged     ref L a R, samples L b R | L b R: one call with cols=0,1.
  twopaths   ref L a R, samples L b R | L b R[:9] d R[10:]: the flank is merged, the alleles differ: two calls of a break.
  nocol      ref L a R e T, samples L b R[:k+2] | L b R f T2: the allele of colour 0 goes on along the reference and stops
             where the population forks and the colour has neither branch.
  lacks      ref L a R, samples L b R | L a R: colour 1 holds the fork node and not the successor.
  loop       ref L R, sample L U U U ..: the allele goes round a cycle off the reference and stops at its third entry.
  cycleref   ref L R and Z c Z2 without its edges, sample L U U U .. and L2 into the middle of the cycle, c the M cycle
             k-mers in front of the k-mer that L enters the cycle by: the allele goes round a cycle with two ways in; at
             every second step end it holds a run of exactly M k-mers, which is dropped in the next step, so the runs a
             walk would hand out fall and rise along it; the repeat rule ends the walk where it holds one.
  refn       ref z N l with l in lower case and z a stretch the sample lacks, sample l with a SNP: offsets run on across
             the N; the reference adds k-mers."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import breakpoints_restate as B  # noqa: E402
from bubbles_cases import pieces, bases  # noqa: E402

KS = (11, 31, 33)
WIDE_KS = (63, 65, 95, 97, 127)  # a full and a 2-bit top word at keys of two, three and four words
M = 5


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def equal(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    return [L + Rr], [[L + Rr]]


def refbubble(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    a, b = bases(rng, 2)
    s = L + a + Rr + L + b + Rr
    return [s], [[s]]


def snp(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    a, b = bases(rng, 2)
    return [L + a + Rr], [[L + b + Rr]]


def insertion(rng, k):
    L, X, Rr = pieces(rng, k, (k + 8, 4, k + 10))
    return [L + Rr], [[L + X + Rr]]


def deletion(rng, k):
    L, X, Rr = pieces(rng, k, (k + 8, 4, k + 10))
    return [L + X + Rr], [[L + Rr]]


def microhom(rng, k):
    L, Y, Rr = pieces(rng, k, (k + 8, 3, k + 10))
    return [L + Rr[:2] + Y + Rr], [[L + Rr]]


def twosnps(rng, k):
    L, Rr, T = pieces(rng, k, (k + 8, k + 10, k + 8))
    a, b = bases(rng, 2)
    c, d = bases(rng, 2)
    return [L + a + Rr + c + T], [[L + b + Rr + d + T]]


def junction(rng, k):
    A, Bb = pieces(rng, k, (2 * k + 10, 2 * k + 10))
    h = k + 5
    return [A, Bb], [[A[:h] + Bb[h:]]]


def ends(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    return [L, Rr], [[L + Rr]]


def inversion(rng, k):
    L, Mm, Rr = pieces(rng, k, (k + 8, 2 * k + 6, k + 10))
    return [L + Mm + Rr], [[L + rc(Mm) + Rr]]


def other(ch):
    return "ACGT"[("ACGT".index(ch) + 1) % 4]


def repeat(rng, k, plen=M + 3):
    A, P, Bb, Cc, D, E, F, X = pieces(rng, k, (2 * k + 8, k - 1 + plen, 2 * k + 8, k + 4, k + 4, k + 8, k + 4, 4))
    Cc, D = Cc[:-1] + other(A[-1]), other(Bb[0]) + D[1:]  # the two copies of P agree in exactly its k-mers
    a = next(c for c in "ACGT" if c != A[3])
    b = next(c for c in "ACGT" if c != Bb[-4])
    return [A + P + Bb, Cc + P + D, E + F], [[A[:3] + a + A[4:] + P + Bb[:-4] + b + Bb[-3:], E + X + P + Bb]]


def repeat_exact(rng, k):
    return repeat(rng, k, M)


def exact(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    a, b = bases(rng, 2)
    return [L + a + Rr], [[L[-(k - 1 + M):] + b + Rr[:k - 1 + M]]]


def lost(rng, k):
    L, Rr, Z, X = pieces(rng, k, (k + 8, k + 10, k + 2, k + 2))
    return [L + Rr], [[Z + Rr[3:k + 5] + X]]


def tail(rng, k):
    L, Rr, X = pieces(rng, k, (k + 8, k + 10, 2 * k))
    return [L + Rr], [[L + X]]


def twosucc(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    a, b, c = bases(rng, 3)
    return [L + a + Rr], [[L + b + Rr], [L + c + Rr]]


def merged(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    a, b = bases(rng, 2)
    return [L + a + Rr], [[L + b + Rr], [L + b + Rr]]


def twopaths(rng, k):
    L, Rr = pieces(rng, k, (k + 8, 2 * k + 10))
    a, b = bases(rng, 2)
    d = next(c for c in "ACGT" if c != Rr[9])
    return [L + a + Rr], [[L + b + Rr], [L + b + Rr[:9] + d + Rr[10:]]]


def nocol(rng, k):
    L, Rr, T, T2 = pieces(rng, k, (k + 8, k + 10, k + 4, k + 4))
    a, b = bases(rng, 2)
    e, f = bases(rng, 2)
    return [L + a + Rr + e + T], [[L + b + Rr[:k + 2]], [L + b + Rr + f + T2]]


def lacks(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    a, b = bases(rng, 2)
    return [L + a + Rr], [[L + b + Rr], [L + a + Rr]]


def loop(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    U = rnd(rng, 7)
    return [L + Rr], [[L + U * ((k + 20) // 7 + 2)]]


def cycleref(rng, k):
    L, Rr, L2, Z, Z2 = pieces(rng, k, (k + 8, k + 10, k + 4, k + 2, k + 2))
    U = rnd(rng, 12)
    turns = U * ((3 * k) // 12 + 4)
    copy = turns[7:11 + k]  # the M cycle k-mers that end in front of the cycle's first k-mer
    return [L + Rr, Z + copy + Z2], [[L + turns, L2 + turns[6:6 + k + 6]]]


def refn(rng, k):
    Z, L = pieces(rng, k, (k + 6, 2 * k + 12))
    a = next(c for c in "ACGT" if c != L[k + 6])
    return [Z + "N" + L.lower() + "NN" + Z[:k - 1]], [[L[:k + 6] + a + L[k + 7:]]]


# name, maker, (min_ref, max_ref, ref_edges), what the case must reach: stats or events that are not 0
SPECS = (
    ("equal", equal, (M, 1000, True), ("ref_keys",)),
    ("refbubble", refbubble, (M, 1000, True), ("key_occurs_twice",)),
    ("snp", snp, (M, 1000, True), ("calls", "flank3pidx_from_k1")),
    ("twosnps", twosnps, (M, 1000, True), ("calls", "stop_runs", "runs_ended")),
    ("snp_maxref", snp, (M, 8, True), ("stop_maxref", "calls")),
    ("insertion", insertion, (M, 1000, True), ("calls",)),
    ("deletion", deletion, (M, 1000, True), ("calls", "flank3pidx_from_k1")),
    ("microhom", microhom, (M, 1000, True), ("calls", "flank3pidx_below_k1")),
    ("junction", junction, (M, 1000, True), ("calls",)),
    ("ends", ends, (M, 1000, True), ("calls", "fork_has_one_successor")),
    ("inversion", inversion, (M, 1000, True), ("calls", "allele_run_minus")),
    ("repeat", repeat, (M, 1000, True), ("calls", "one_of_two_runs_ends", "sort_tie_on_chrom", "runs_two_chroms_one_qoffset", "runs_ended")),
    ("repeat_exact", repeat_exact, (M, 1000, True), ("calls", "one_of_two_runs_ends", "exact_run_dropped_5p", "exact_run_dropped_3p")),
    ("exact", exact, (M, 1000, False), ("calls", "exact_run_kept_5p", "exact_run_kept_3p", "stop_nocovg")),
    ("exact_edges", exact, (M, 1000, True), ("calls",)),
    ("lost", lost, (M, 1000, True), ("stop_flank", "flanks_norun")),
    ("tail", tail, (M, 1000, True), ("alleles_norun",)),
    ("twosucc", twosucc, (M, 1000, True), ("two_nonref_successors", "calls")),
    ("merged", merged, (M, 1000, True), ("colours_merged",)),
    ("twopaths", twopaths, (M, 1000, True), ("two_calls_one_break",)),
    ("nocol", nocol, (M, 1000, True), ("stop_nocolcovg", "calls")),
    ("lacks", lacks, (M, 1000, True), ("colour_lacks_successor", "calls")),
    ("loop", loop, (M, 1000, True), ("stop_repeat",)),
    ("cycleref", cycleref, (M, 1000, False), ("kept_runs_fell", "stop_repeat", "calls", "exact_run_kept_3p")),
    ("refn", refn, (M, 1000, True), ("ref_added", "calls")),
)
NO_CALL = ("equal", "refbubble", "lost", "tail", "loop")  # cases whose text is empty
NO_BREAK = ("equal", "refbubble")


def run(case, **kw):
    p = dict(case["params"])
    p.update(kw)
    return B.call(case["graph"], case["k"], case["ncols"], case["ref"], case["names"], p["min_ref"], p["max_ref"], p["ref_edges"])


@functools.lru_cache(maxsize=None)
def cases(ks=KS):
    out = []
    made = {}
    for k in ks:
        for name, make, (mn, mx, edges), need in SPECS:
            for salt in range(200):
                key = (make.__name__, k, salt)
                if key not in made:
                    ref, cols = make(random.Random(9000 + 100 * k + salt), k)
                    made[key] = (R.build(cols + [[]], k), len(cols) + 1, ref, cols)
                graph, ncols, ref, cols = made[key]
                case = {"name": "%s_k%d" % (name, k), "k": k, "ncols": ncols, "graph": graph, "ref": ref, "seqs": cols,
                        "names": ["chr%d" % (i + 1) for i in range(len(ref))],
                        "params": {"min_ref": mn, "max_ref": mx, "ref_edges": edges}}
                _, _, stats, events, _ = run(case)
                if all(stats.get(n, 0) or events.get(n, 0) for n in need):
                    out.append(case)
                    break
            else:
                raise AssertionError("no graph for %s at k=%d" % (name, k))
    return tuple(out)


def wide_cases():
    """the same structures at WIDE_KS; no golden pins these, the restatement is the oracle"""
    return cases(WIDE_KS)
