"""The cases of the `bubbles` tests, built on the CPU and shared by test_bubbles_restate.py (which asserts that they reach
every rule named there), test_gpu_bubbles.py (which runs them on the device) and test_bubbles_cli.py.  Small graphs at
k = 11, 31 and 33 (keys of one and two words) from a few sequences each, 2 to 4 colours; max_allele and max_flank lie
between 3 and 100.  tests/golden/bubbles.json pins these by name.  wide_cases() is the same structures at k = 63, 65, 95, 97
and 127 (keys of two, three and four words, the top word full or holding two bits) with the limits of 100 grown to 3 k,
which no golden pins: there the device is compared with the restatement alone.

Structures (upper-case names are random stretches without a repeated k-mer, a b c d are single bases that differ):
  snp      L a R | L b R | L a R, and in colour 0 also Z R[4:]: a SNP between colours called from both sides with branches
           of k k-mers; colours 0 and 2 walk the same path (duplicates); the unitig of branch a is a candidate whose paths
           all start alike; Z splits R, so its second unitig is a candidate whose previous steps are all alike; L is longer
           than max_flank.  `snp_limit` is the same graph with max_allele 3: every path stops at the limit.
  indel    L X R | L R.
  empty    P INS P[-(k-1):] Q | P Q: the k-mer behind the fork starts the 3' flank, so one branch has no k-mer.
  three    L a R | L b R | L c R | L a R: a call with three branches.
  multi    L a R | L b R | Z (L a R)[i:] with i inside branch a: that branch is made of two unitigs, and walked
           backwards it passes a fork of which one branch only is in the colour.
  haploid  colour 0 holds L a R, L b R and Z L[3:], colour 1 holds L a R: with colour 0 haploid the second allele goes and
           the bubble is dropped; walked from R the paths of colour 0 stop at the fork that Z makes (both branches in it).
  serial   L a M c R | L b M d R: from L the candidate R is dropped because both paths pass M; kept with keep_serial.
  nocol    L a R[:k+3] | L b R x T1, R[-k:] y T2, Z R[4:k+6]: the path of colour 0 goes on through k-mers that the
           colour lacks and stops where the population forks and the colour has neither branch.
  loop     L U U U .. | L V with U a few bases long: the path of colour 0 goes round the loop and stops at its third entry.
  cross    P1 C a R | P2 C b R with C one k-mer: the fork node has two ways in, so the 5' flank is that k-mer alone."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import bubbles_restate as B  # noqa: E402

KS = (11, 31, 33)
WIDE_KS = (63, 65, 95, 97, 127)  # a full and a 2-bit top word at keys of two, three and four words


def pieces(rng, k, lens):
    """random stretches of the given lengths whose concatenation repeats no k-mer (nor a reverse complement)"""
    while True:
        p = ["".join(rng.choice("ACGT") for _ in range(n)) for n in lens]
        s = "".join(p)
        keys = [R.canon(R.kmer_int(s[i:i + k]), k) for i in range(len(s) - k + 1)]
        if len(set(keys)) == len(keys):
            return p


def bases(rng, n, avoid=""):
    """n bases that differ from each other and from those of `avoid`"""
    return rng.sample([c for c in "ACGT" if c not in avoid], n)


def snp(rng, k):
    L, Rr, Z = pieces(rng, k, (k + 8, k + 10, k + 2))
    a, b = bases(rng, 2)
    return [[L + a + Rr, Z + Rr[4:]], [L + b + Rr], [L + a + Rr]]


def indel(rng, k):
    L, Rr = pieces(rng, k, (k + 8, k + 10))
    X = "".join(rng.choice("ACGT") for _ in range(3))
    return [[L + X + Rr], [L + Rr]]


def empty(rng, k):
    P, INS, Q = pieces(rng, k, (k + 6, 4, k + 6))
    return [[P + INS + P[-(k - 1):] + Q], [P + Q]]


def three(rng, k):
    L, Rr = pieces(rng, k, (k + 3, k + 4))
    a, b, c = bases(rng, 3)
    return [[L + a + Rr], [L + b + Rr], [L + c + Rr], [L + a + Rr]]


def multi(rng, k):
    L, Rr, Z = pieces(rng, k, (k + 3, k + 4, k + 2))
    a, b = bases(rng, 2)
    s0 = L + a + Rr
    return [[s0], [L + b + Rr], [Z + s0[len(L) - k + 1 + 3:]]]


def haploid(rng, k):
    L, Rr, Z = pieces(rng, k, (k + 8, k + 4, k + 2))
    a, b = bases(rng, 2)
    return [[L + a + Rr, L + b + Rr, Z + L[3:]], [L + a + Rr]]


def serial(rng, k):
    L, M, Rr = pieces(rng, k, (k + 3, k + 4, k + 4))
    a, b = bases(rng, 2)
    c, d = bases(rng, 2)
    return [[L + a + M + c + Rr], [L + b + M + d + Rr]]


def nocol(rng, k):
    L, Rr, Z, T1, T2 = pieces(rng, k, (k + 3, k + 10, k + 2, k + 2, k + 2))
    a, b = bases(rng, 2)
    x, y = bases(rng, 2)
    return [[L + a + Rr[:k + 3]], [L + b + Rr + x + T1, Rr[-k:] + y + T2, Z + Rr[4:k + 6]]]


def loop(rng, k):
    L, V = pieces(rng, k, (k + 3, k + 3))
    U = "".join(rng.choice("ACGT") for _ in range(7))
    return [[L + U * ((k + 20) // 7 + 2)], [L + V]]


def cross(rng, k):
    P1, P2, Cc, Rr = pieces(rng, k, (k + 2, k + 2, k, k + 4))
    a, b = bases(rng, 2)
    return [[P1 + Cc + a + Rr], [P2 + Cc + b + Rr]]


# name, maker, (max_allele, max_flank, haploid, keep_serial), what the case must reach: stats or events that are not 0
SPECS = (
    ("snp", snp, (100, 5, (), False), ("bubbles", "branch_k_kmers", "dupes_removed", "3p_first_equal", "3p_prev_equal", "flank_cut", "stop_nocovg")),
    ("snp_limit", snp, (3, 5, (), False), ("stop_limit",)),
    ("indel", indel, (100, 100, (), False), ("bubbles",)),
    ("empty", empty, (100, 100, (), False), ("branch_empty", "dupes_removed")),
    ("three", three, (100, 100, (), False), ("call_three_branches",)),
    ("multi", multi, (100, 100, (), False), ("branch_multi_unitig", "popfrk_colfwd")),
    ("haploid", haploid, (100, 100, (0,), False), ("haploid_dropped", "stop_nolinks")),
    ("haploid_off", haploid, (100, 100, (), False), ("bubbles", "stop_nolinks")),
    ("serial", serial, (100, 100, (), False), ("serial_dropped", "bubbles")),
    ("serial_kept", serial, (100, 100, (), True), ("branch_multi_unitig",)),
    ("nocol", nocol, (100, 100, (), False), ("stop_nocolcovg", "popfwd")),
    ("loop", loop, (100, 100, (), False), ("stop_repeat",)),
    ("cross", cross, (100, 7, (1,), False), ("flank_one",)),
)


def run(case):
    p = case["params"]
    return B.call(case["graph"], case["k"], case["ncols"], p["max_allele"], p["max_flank"], p["haploid"], p["keep_serial"])


def limit(n, k):
    """a limit of SPECS at k: those of 100 grow with a wide k (an allele of `serial` alone is some 2 k k-mers long) and
    are 100 at every k of KS; those of 3, 5 and 7 stay"""
    return max(100, 3 * k) if n == 100 else n


@functools.lru_cache(maxsize=None)
def cases(ks=KS):
    out = []
    graphs = {}
    for k in ks:
        for name, make, (ma, mf, hap, serial_kept), need in SPECS:
            ma, mf = limit(ma, k), limit(mf, k)
            for salt in range(200):
                key = (make.__name__, k, salt)
                if key not in graphs:
                    seqs = make(random.Random(7000 + 100 * k + salt), k)
                    graphs[key] = (R.build(seqs, k), len(seqs), seqs)
                graph, ncols, seqs = graphs[key]
                case = {"name": "%s_k%d" % (name, k), "k": k, "ncols": ncols, "graph": graph, "seqs": seqs,
                        "params": {"max_allele": ma, "max_flank": mf, "haploid": tuple(hap), "keep_serial": serial_kept}}
                _, _, stats, events = run(case)
                if all(stats.get(n, 0) or events.get(n, 0) for n in need):
                    out.append(case)
                    break
            else:
                raise AssertionError("no graph for %s at k=%d" % (name, k))
    return tuple(out)


def wide_cases():
    """the same structures at WIDE_KS; no golden pins these, the restatement is the oracle"""
    return cases(WIDE_KS)
