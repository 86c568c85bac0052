"""Hand-made graphs for `popbubbles`, shared by the restatement's test and the device test.  Each case is
(name, k, graph, (max_covg, max_klen, max_kdiff), expected removed keys, expected num_popped); the expectations are
worked out by hand from the reference's rules and the project's visiting order (pop_restate.py), not computed."""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pop_bubbles.json")


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def keys_of(seq, k):
    return {R.canon(R.kmer_int(seq[i:i + k]), k) for i in range(len(seq) - k + 1)}


def branch_keys(left, allele, right, k):
    """the k-mers that hold some base of `allele` in left + allele + right"""
    return keys_of(left[-(k - 1):] + allele + right[:k - 1], k)


def branch_E(left, allele, right, k):
    s = left[-(k - 1):] + allele + right[:k - 1]
    return min(R.canon(R.kmer_int(s[:k]), k), R.canon(R.kmer_int(s[-k:]), k))


def golden():
    return json.load(open(GOLDEN))


def snp(seed, k, alleles="ACG"):
    """left flank, right flank and the alleles in ascending order of their branches' E"""
    rng = random.Random(seed)
    left, right = rseq(rng, 2 * k), rseq(rng, 2 * k)
    return left, right, sorted(alleles, key=lambda a: branch_E(left, a, right, k))


def pops_of_two(e_winner, e_loser):
    """two branches with different means: the winner's turn removes the loser as the alternative and marks it visited
    (1 pop).  If the loser comes first it removes itself as s1, is not marked, and the winner pops it again (2 pops)."""
    return 1 if e_winner < e_loser else 2


def drop_edge(graph, key, bit):
    cv, ed = graph[key]
    graph[key] = (cv, [e & ~(1 << bit) for e in ed])


def cases():
    out = []
    k = 11
    # -- three branches between the same two forks (the drawing in pop_bubbles.c), coverage 3, 2, 1 ------------------
    # Every unitig that takes its turn meets both others.  Lowest E has the highest coverage: it goes first, both others
    # lose as alternatives and are marked visited, so they never take their turn: 2 pops.
    left, right, (a, b, c) = snp(1, k)
    seqs = [left + a + right] * 3 + [left + b + right] * 2 + [left + c + right]
    gone = branch_keys(left, b, right, k) | branch_keys(left, c, right, k)
    out.append(("three_branches_top_first", k, R.build([seqs], k), (-1, -1, -1), gone, 2))
    # Lowest E has the lowest coverage: it loses twice as s1 (not marked visited, but it has had its turn); the middle one
    # then takes its turn (pops the lowest again, loses to the highest), then the highest pops both again: 6 pops.
    seqs = [left + a + right] + [left + b + right] * 2 + [left + c + right] * 3
    gone = branch_keys(left, a, right, k) | branch_keys(left, b, right, k)
    out.append(("three_branches_bottom_first", k, R.build([seqs], k), (-1, -1, -1), gone, 6))
    # -- equal coverage: the alternative of the branch with the lower E goes ----------------------------------------------
    left, right, (a, b) = snp(2, k, "CT")
    seqs = [left + a + right] * 2 + [left + b + right] * 2
    out.append(("tie", k, R.build([seqs], k), (-1, -1, -1), branch_keys(left, b, right, k), 1))
    # two colours, one allele in each: the means are taken over the summed coverage, the edges over the union
    g2 = R.build([[left + a + right] * 2, [left + b + right] * 2], k)
    out.append(("tie_two_colours", k, g2, (-1, -1, -1), branch_keys(left, b, right, k), 1))
    # -- -C, -L, -D: the loser has mean 2 and k k-mers against mean 5 -------------------------------------------------------
    left, right, (a, b) = snp(3, k, "AG")
    g = R.build([[left + a + right] * 5 + [left + b + right] * 2], k)
    lose = branch_keys(left, b, right, k)
    for name, args, pops in (("defaults", (-1, -1, -1), True), ("zeros_ignore_C_and_L", (0, 0, -1), True), ("C_keeps", (1, -1, -1), False),
                             ("C_allows", (2, 0, -1), True), ("L_keeps", (-1, k - 1, -1), False), ("L_allows", (0, k, -1), True),
                             ("D_zero_allows_equal_lengths", (-1, -1, 0), True)):
        out.append(("snp_" + name, k, g, args, lose if pops else set(), 1 if pops else 0))
    # an insertion of 2 bases: branches of k - 1 (without) and k + 1 (with) k-mers
    rng = random.Random(4)
    left, right = rseq(rng, 2 * k), rseq(rng, 2 * k)
    ins = next(x for x in ("AC", "CA", "GT", "TG", "AG", "GA") if x[0] != right[0] and x[-1] != left[-1] and x[0] != left[-1])
    g = R.build([[left + right] * 4 + [left + ins + right]], k)
    lose = branch_keys(left, ins, right, k)
    assert len(lose) == k + 1
    out.append(("indel_D_keeps", k, g, (-1, -1, 1), set(), 0))
    out.append(("indel_D_zero_keeps", k, g, (0, 0, 0), set(), 0))
    out.append(("indel_D_allows", k, g, (-1, -1, 2), lose, pops_of_two(branch_E(left, "", right, k), branch_E(left, ins, right, k))))
    out.append(("indel_L_keeps", k, g, (-1, k, -1), set(), 0))
    # -- a chain of ties: A || B, B || C, but A and C share no fork.  B sits between two left forks (x1, x2) and two
    # right forks (y1, y2); A hangs on x1 and y1 only, C on x2 and y2 only.  All three have mean 2.  In E order A < B < C:
    # A's turn removes B (the alternative) and marks it visited; B never takes its turn, so C stays; C's turn removes B
    # again: {B} removed, 2 pops.  (A pairwise rule "lower (mean, E) loses" would remove C as well.)
    rng = random.Random(5)
    f1, f2, g1, g2 = (rseq(rng, 2 * k) for _ in range(4))
    mid_l, mid_r = rseq(rng, k - 1), rseq(rng, k - 1)
    p, q, r, s = "A", "C", "G", "T"
    A, B, C = sorted("ACG", key=lambda x: branch_E(mid_l, x, mid_r, k))  # the shared branch is the middle one in E
    seqs = [f1 + p + mid_l + A + mid_r + r + g1] * 2 + [f1 + p + mid_l + B + mid_r + r + g1, f2 + q + mid_l + B + mid_r + s + g2] + \
           [f2 + q + mid_l + C + mid_r + s + g2] * 2
    out.append(("tie_chain", k, R.build([seqs], k), (-1, -1, -1), branch_keys(mid_l, B, mid_r, k), 2))
    # -- a hairpin: stem + loop + reversed stem.  The loop leaves the stem's last k-mer x and returns into x reversed, so
    # the loop read backwards is a sibling of itself at both ends: it is its own alternative, ties with itself and goes.
    rng = random.Random(6)
    stem, loop = rseq(rng, 2 * k), "A" + rseq(rng, k + 2) + "C"  # (first base != complement of the last)
    out.append(("hairpin_loop", k, R.build([[stem + loop + rc(stem)] * 2], k), (-1, -1, -1), branch_keys(stem, loop, rc(stem), k), 1))
    # -- a branch of length 1: one more base in a run of k - 2 equal bases.  k = 5: ..CGAAAT.. against ..CGAAAAT..; the
    # short path crosses the single k-mer GAAAT, the long one GAAAA and AAAAT
    k5 = 5
    fl, fr = "TCTGC", "TGCCAGT"
    g = R.build([[fl + "GAAAT" + fr] * 3 + [fl + "GAAAAT" + fr]], k5)
    e_short = R.canon(R.kmer_int("GAAAT"), k5)
    e_long = min(R.canon(R.kmer_int("GAAAA"), k5), R.canon(R.kmer_int("AAAAT"), k5))
    out.append(("branch_of_length_1_wins", k5, g, (-1, -1, -1), keys_of("GAAAAT", k5), pops_of_two(e_short, e_long)))
    g = R.build([[fl + "GAAAT" + fr] + [fl + "GAAAAT" + fr] * 3], k5)
    out.append(("branch_of_length_1_goes", k5, g, (-1, -1, -1), keys_of("GAAAT", k5), pops_of_two(e_long, e_short)))
    # -- one-sided edges: three branches, coverage 3, 2, 1 in E order, and the left fork has lost its edge to the first
    # (highest) branch, which still has its edge back.  That branch sees both others (it walks out over its own edge and
    # back over the fork's two remaining edges: nothing to clear there), pops both and marks them visited: 2 pops.  The
    # others would not have seen it from their side.
    k = 11
    left, right, (a, b, c) = snp(7, k)
    g = R.build([[left + a + right] * 3 + [left + b + right] * 2 + [left + c + right]], k)
    fork = left[-k:]
    fk = R.canon(R.kmer_int(fork), k)
    fo = 0 if fk == R.kmer_int(fork) else 1
    drop_edge(g, fk, "ACGT".index(a) + 4 * fo)
    out.append(("one_sided_edge", k, g, (-1, -1, -1), branch_keys(left, b, right, k) | branch_keys(left, c, right, k), 2))
    return out


def fragment_case():
    """one-sided edges that make an alternative a fragment of a unitig: two branches, and the left fork has lost its edge
    to the first one, so the fork and the second branch form one unitig.  From the first branch's left end the alternative
    is the part of that unitig after the fork.  (The seed makes the fork's end the first branch's left end: the one with the
    lower key.)"""
    k = 11
    for seed in range(8, 100):
        left, right, (a, b) = snp(seed, k, "AT")
        s = left[-(k - 1):] + a + right[:k - 1]
        if R.canon(R.kmer_int(s[:k]), k) < R.canon(R.kmer_int(s[-k:]), k):
            break
    g = R.build([[left + a + right] * 3 + [left + b + right]], k)
    fork = left[-k:]
    fk = R.canon(R.kmer_int(fork), k)
    fo = 0 if fk == R.kmer_int(fork) else 1
    drop_edge(g, fk, "ACGT".index(a) + 4 * fo)
    return k, g, branch_keys(left, b, right, k)
