"""The restatement of `unitigs` (unitigs_restate.py) against expectations worked out by hand, and its properties on
random graphs.  k-mers below are written as strings; a key is the lower of a k-mer and its reverse complement."""
import os
import random
from collections import Counter
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import unitigs_restate as U  # noqa: E402


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def build(seqs, k):
    return R.build([seqs], k)


def test_single_kmer_is_forward():
    # TTT's key is AAA: printed forwards as AAA whatever strand was read
    g = build(["TTT"], 3)
    assert U.fasta(g, 3) == b">unitig0 prev= next=\nAAA\n"
    assert U.gfa(g, 3) == b"H\tVN:Z:1.0\nS\tnode0\tAAA\n"
    assert U.dot(g, 3) == (b"digraph G {\n  edge [dir=both arrowhead=none arrowtail=none color=\"blue\"]\n"
                            b"  node [shape=none, fontname=courier, fontsize=9]\n  node0 [label=AAA]\n\n}\n")
    assert b"node [shape=point, label=none, fontname=courier, fontsize=9]" in U.dot(g, 3, points=True)


def test_chain_with_higher_key_first_is_reversed():
    # TGAAC holds TGA (key TCA), GAA (key GAA), AAC (key AAC): as read, the chain starts at the higher end key TCA.
    # Normalised it starts at AAC read backwards (GTT) and ends at TCA forwards: GTT TTC TCA
    g = build(["TGAAC"], 3)
    us = R.unitigs(g, 3)
    assert len(us) == 1 and len(us[0]) == 3
    assert U.fasta(g, 3) == b">unitig0 prev= next=\nGTTCA\n"
    assert U.gfa(g, 3) == b"H\tVN:Z:1.0\nS\tnode0\tGTTCA\n"


def test_fork_letters_and_link_orientations():
    # k = 5: the stem CCACA forks to CACAA -> ACAAG and to CACAT -> ACATG
    #   keys: CCACA, CACAA, ACAAG, ATGTG (CACAT reversed), ACATG
    #   unitigs: [CACAA ACAAG], [CACAT ACATG], [CCACA]; lower end keys ACAAG and ACATG, so both arms are reversed:
    #   CTTGT TTGTG = CTTGTG and CATGT ATGTG = CATGTG; first keys ACAAG < ACATG < CCACA give the numbers
    g = build(["CCACAAG", "CCACATG"], 5)
    assert U.fasta(g, 5).decode() == (">unitig0 prev= next=G\nCTTGTG\n"
                                      ">unitig1 prev= next=G\nCATGTG\n"
                                      ">unitig2 prev= next=AT\nCCACA\n")
    # each arm leaves its right end (+) into the stem read backwards (-).  The arms' end keys CACAA and ATGTG are
    # below the stem's CCACA, so the arms print the lines and the stem prints none
    assert U.gfa(g, 5).decode() == ("H\tVN:Z:1.0\nS\tnode0\tCTTGTG\nS\tnode1\tCATGTG\nS\tnode2\tCCACA\n"
                                    "L\tnode0\t+\tnode2\t-\t4M\nL\tnode1\t+\tnode2\t-\t4M\n")
    assert U.dot(g, 5).decode().endswith("  node2 [label=CCACA]\n\n  node0:e -> node2:e\n  node1:e -> node2:e\n}\n")


def test_closed_cycle_entered_away_from_its_lowest_key():
    # k = 3, the cycle CAG -> AGC -> GCA -> CAG entered at GCA: keys CAG, AGC, GCA; the lowest is AGC, forwards
    g = build(["GCAGCA"], 3)
    us = R.unitigs(g, 3)
    assert len(us) == 1 and len(us[0]) == 3 and U.is_cycle(g, us[0], 3)
    assert U.fasta(g, 3) == b">unitig0 prev=C next=C\nAGCAG\n"  # CAG comes before AGC, and AGC after CAG
    # the edge from the last k-mer back to the first: only the left end's line passes the rule (AGC < CAG)
    assert U.gfa(g, 3) == b"H\tVN:Z:1.0\nS\tnode0\tAGCAG\nL\tnode0\t-\tnode0\t-\t2M\n"


def test_cycle_whose_lowest_key_is_reached_in_reverse():
    # k = 3, the cycle TGA -> GAT -> ATG -> TGA: keys TCA (TGA reversed), ATC (GAT reversed), ATG (forwards).  The lowest
    # key is ATC, met as GAT: the cycle is read the other way round: ATC -> TCA -> CAT
    g = build(["TGATGA"], 3)
    us = R.unitigs(g, 3)
    assert len(us) == 1 and U.is_cycle(g, us[0], 3)
    assert U.fasta(g, 3) == b">unitig0 prev=C next=C\nATCAT\n"
    assert [kk for kk, _ in U.unitigs(g, 3)[0]] == [R.kmer_int("ATC"), R.kmer_int("TCA"), R.kmer_int("ATG")]


def test_hairpin():
    # k = 3: CCGCGT holds CCG, CGC, GCG, CGT; GCG is CGC's reverse complement: the walk meets the key CGC twice in a
    # row (B -> B') and the unitig ends there on both sides
    g = build(["CCGCGT"], 3)
    fa = U.fasta(g, 3).decode()
    seqs = sorted(fa.split("\n")[1::2])
    assert seqs == ["ACG", "CCG", "CGC"]
    spelled = [U.spell(u, 3) for u in U.unitigs(g, 3)]
    assert sorted(spelled) == seqs
    # CGC links to itself: + to - (the hairpin), printed once, from the right end
    assert "L\tnode2\t+\tnode2\t-\t2M\n" in U.gfa(g, 3).decode()
    assert U.gfa(g, 3).decode().count("node2\t+\tnode2") == 1


def test_homopolymer_self_loop_gives_one_link():
    g = build(["AAAAA"], 3)
    assert U.fasta(g, 3) == b">unitig0 prev=A next=A\nAAA\n"
    assert U.gfa(g, 3) == b"H\tVN:Z:1.0\nS\tnode0\tAAA\nL\tnode0\t+\tnode0\t+\t2M\n"
    assert U.dot(g, 3).decode().count("->") == 1


def random_graph(rng, k):
    n = 40 if k <= 7 else 400
    seqs = [rseq(rng, rng.randrange(k, k + n)) for _ in range(6)]
    seqs += [seqs[0][:k + 5] + rseq(rng, k), "A" * (k + 2)]
    cyc = rseq(rng, 2 * k)
    seqs.append(cyc + cyc[:k])
    return build(seqs, k)


@pytest.mark.parametrize("k", [3, 5, 7, 31, 63, 95, 127])
def test_properties_on_random_graphs(k):
    for seed in range(8 if k <= 7 else 2):
        g = random_graph(random.Random(100 * k + seed), k)
        us = U.unitigs(g, k)
        # every key is spelled exactly once
        keys = [kk for u in us for kk, _ in u]
        assert sorted(keys) == sorted(g)
        # numbering: ascending first keys
        assert [u[0][0] for u in us] == sorted(u[0][0] for u in us)
        for u in us:
            # consecutive k-mers are joined by an edge in both
            for (a, oa), (b, ob) in zip(u, u[1:]):
                sa = a if oa == 0 else R.revcomp(a, k)
                sb = b if ob == 0 else R.revcomp(b, k)
                assert sa & ((1 << (2 * (k - 1))) - 1) == sb >> 2
                assert (U.nibble(g, a, oa) >> (sb & 3)) & 1
                assert (U.nibble(g, b, 1 - ob) >> (3 - (sa >> (2 * (k - 1))))) & 1
            # no unitig could be extended at either end
            for key, o in (u[-1], (u[0][0], 1 - u[0][1])):
                nib = U.nibble(g, key, o)
                if bin(nib).count("1") != 1:
                    continue
                nk, no = R.step(key, o, nib.bit_length() - 1, k)
                back = bin(U.nibble(g, nk, 1 - no)).count("1")
                inside = {kk for kk, _ in u}
                assert nk not in g or back != 1 or nk == key or (nk in inside and U.is_cycle(g, u, k))
            # normal form
            if len(u) == 1:
                assert u[0][1] == 0
            elif U.is_cycle(g, u, k):
                assert u[0] == (min(kk for kk, _ in u), 0)
            else:
                assert u[0][0] < u[-1][0]
        # every link appears exactly once: an edge between two ends is seen from both of them (i a j b and j !b i !a),
        # except a hairpin edge, which is its own mirror image; the rule keeps one of each pair
        def canon(e):
            i, a, j, b = e
            return min(e, (j, 1 - b, i, 1 - a))
        seen = Counter(canon(e) for e in U.links(g, us, k, rule=False))
        kept = Counter(canon(e) for e in U.links(g, us, k))
        for e, cnt in seen.items():
            mirror = e == (e[2], 1 - e[3], e[0], 1 - e[1])
            assert kept[e] == (cnt if mirror else cnt // 2) and (mirror or cnt % 2 == 0), e
        assert set(kept) == set(seen)
        gfa = U.gfa(g, k).decode().split("\n")
        assert len([x for x in gfa if x.startswith("L")]) == sum(kept.values())
        # the three formats agree on the sequences
        fa = U.fasta(g, k).decode().split("\n")[1::2][:len(us)]
        S = [x.split("\t")[2] for x in gfa if x.startswith("S")]
        D = [x.split("label=")[1][:-1] for x in U.dot(g, k).decode().split("\n") if "label=" in x and x.startswith("  node") and "[label" in x]
        assert fa == S == D == [U.spell(u, k) for u in us]
        assert all(len(s) == k - 1 + len(u) for s, u in zip(S, us))
