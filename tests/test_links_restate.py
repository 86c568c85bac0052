"""links_restate.py on the CPU, pinned by cases worked by hand through src/paths/link_tree.c: the maximal-link quirk,
duplicates summed beyond a byte, F and R groups on one k-mer, a histogram in which both clips bite, -L, every refusal of
the line parser, and the inputs of the reference's tests/clean_links pipeline (golden/clean_links.json) through
thread_restate.py: cleaning at 5 removes every erroneous link and keeps the true ones.  golden/links.json is what the
restatement gives today."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import links_cases as LC  # noqa: E402
import links_restate as LR  # noqa: E402
import thread_restate as T  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "links.json")))
QUIRK = b"ACGTA 2\nF 1 10 A seq=ACGTAA juncpos=0\nF 2 2 AC seq=ACGTAAGC juncpos=0,2\n"


def totals(st):
    return st["num_trees_with_links"], st["num_links"], st["num_link_bytes"]


def test_quirk_without_clean():
    ctp, lst, st, _ = LR.links(QUIRK, 5)
    assert lst == b"6,12\n8,2\n"  # A counts its own 10 and the 2 of AC
    assert ctp == b"ACGTA 1\nF 2 2 AC seq=ACGTAAGC juncpos=0,2\n"  # A is the prefix of a longer link: not written
    assert totals(st) == (1, 1, 1)


def test_quirk_with_clean():
    """AC (2 < 5) goes; A (12) stays in the tree and in the list, yet it is still 'the prefix of a longer link': the
    child below A is kept (only its counts are cleared), so nothing is written and nothing is counted"""
    ctp, lst, st, _ = LR.links(QUIRK, 5, clean=5)
    assert lst == b"6,12\n" and ctp == b"" and totals(st) == (0, 0, 0)


def test_duplicates_sum_beyond_a_byte():
    text = b"ACGTA 3\nF 1 200 G seq=ACGTATG juncpos=1\nF 1 200 G seq=ACGTATG juncpos=1\nF 1 7 T seq=ACGTATT juncpos=1\n"
    ctp, lst, st, _ = LR.links(text, 5)
    assert ctp == b"ACGTA 2\nF 1 400 G seq=ACGTATG juncpos=1\nF 1 7 T seq=ACGTATT juncpos=1\n" and lst == b"7,400\n7,7\n"
    assert totals(st) == (1, 2, 2) and st["links_in"] == 3 and st["tree_links"] == 2


def test_both_orientations():
    text = b"ACGTA 3\nR 1 4 C seq=TACGTC juncpos=0\nF 2 3 AC seq=ACGTAAGC juncpos=0,2\nR 2 5 CG seq=TACGTCTTG juncpos=0,3\n"
    ctp, lst, st, _ = LR.links(text, 5)
    assert ctp == b"ACGTA 2\nF 2 3 AC seq=ACGTAAGC juncpos=0,2\nR 2 5 CG seq=TACGTCTTG juncpos=0,3\n"  # F first, R C is a prefix
    assert lst == b"6,3\n8,3\n6,9\n9,5\n" and totals(st) == (1, 2, 2)
    ctp, lst, st, _ = LR.links(text, 5, clean=4)  # the F tree goes, the k-mer stays for its R link
    assert ctp == b"ACGTA 1\nR 2 5 CG seq=TACGTCTTG juncpos=0,3\n" and lst == b"6,9\n9,5\n" and totals(st) == (1, 1, 1)


def test_histogram_clips():
    text = b"ACGTA 3\nF 3 2 ACG seq=ACGTAACTTG juncpos=0,1,4\nF 2 9 AT seq=ACGTAAT juncpos=0,1\nF 1 1 C seq=ACGTAC juncpos=0\n"
    _, lst, _, hists = LR.links(text, 5, hist=(3, 4))
    # A: dist 0, 11 -> bin 3; C: dist 0, 1; AC: dist 1, 2; AT: dist 1, 9 -> bin 3; ACG: dist 4 is beyond the matrix
    assert hists == [[0, 1, 0, 1], [0, 0, 1, 1], [0, 0, 0, 0]]
    assert lst == b"6,11\n7,2\n10,2\n7,9\n6,1\n"
    assert LR.hist_csv(hists, 3, 4) == "  ,covg.01,covg.02,covg.03\ndist.01,0,1,1\ndist.02,0,0,0\n"
    # the histogram is taken before cleaning
    assert LR.links(text, 5, hist=(3, 4), clean=100)[3] == hists


def test_limit():
    text = QUIRK + b"# c\n\nCCCCC 1\nF 1 1 A seq=CCCCCA juncpos=0\nGGGGG 1\nthis line is never read\n"
    assert LR.links(text, 5, limit=1)[:2] == LR.links(QUIRK, 5)[:2]
    ctp, _, st, _ = LR.links(text, 5, limit=2)
    assert ctp.endswith(b"CCCCC 1\nF 1 1 A seq=CCCCCA juncpos=0\n") and st["kmers_read"] == 2
    with pytest.raises(LR.BadLine):
        LR.links(text, 5)


GOOD = "F 2 3 AC seq=ACGTAGAGC juncpos=1,3"
BAD = [("bad_kmer_line", "ACGT 1"), ("bad_kmer_line", "ACGTA x"), ("bad_orient", "X 2 3 AC seq=ACGTAGAGC juncpos=1,3"),
       ("bad_orient", "FR 2 3 AC seq=ACGTAGAGC juncpos=1,3"), ("bad_number", "F x 3 AC seq=ACGTAGAGC juncpos=1,3"),
       ("bad_number", "F 2 y AC seq=ACGTAGAGC juncpos=1,3"), ("multi_colour", "F 2 3,4 AC seq=ACGTAGAGC juncpos=1,3"),
       ("bad_junction", "F 2 3 AN seq=ACGTAGAGC juncpos=1,3"), ("njuncs_range", "F 0 3  seq=ACGTA juncpos=0"),
       ("njuncs_range", "F 32768 3 AC seq=ACGTAGAGC juncpos=1,3"), ("njuncs_length", "F 3 3 AC seq=ACGTAGAGC juncpos=1,3"),
       ("no_seq", "F 2 3 AC juncpos=1,3"), ("no_juncpos", "F 2 3 AC seq=ACGTAGAGC"), ("juncpos_count", "F 2 3 AC seq=ACGTAGAGC juncpos=1"),
       ("juncpos_count", "F 2 3 AC seq=ACGTAGAGC juncpos=1,x"), ("seq_length", "F 2 3 AC seq=ACGTAGAGCA juncpos=1,3"),
       ("seq_base", "F 2 3 AC seq=ACGTAGTGC juncpos=1,3")]


@pytest.mark.parametrize("code,line", BAD)
def test_parser_refusals(code, line):
    text = "ACGTA 1\n%s\n%s\n" % (GOOD, line)
    with pytest.raises(LR.BadLine) as ei:
        LR.links(text.encode(), 5)
    assert (ei.value.code, ei.value.offset) == (code, text.index("\n" + line + "\n") + 1)
    assert LR.links(("ACGTA 1\n%s\n" % GOOD).encode(), 5)[0] == ("ACGTA 1\n%s\n" % GOOD).encode()


def test_link_before_kmer():
    with pytest.raises(LR.BadLine) as ei:
        LR.links(("# c\n%s\nACGTA 1\n" % GOOD).encode(), 5)
    assert (ei.value.code, ei.value.offset) == ("link_before_kmer", 4)


def test_clean_links_pipeline():
    """build -> thread -> links --clean 5 on the reference's own test: 20 copies of two true sequences that share their
    middle, 2 copies of the two recombinants; every link of a recombinant goes, the true ones stay"""
    C = json.load(open(os.path.join(HERE, "golden", "clean_links.json")))
    k = C["k"]
    reads = C["ref"] * C["ref_copies"] + C["err"] * C["err_copies"]
    graph = R.build([reads], k)
    store = T.Store(graph, k).thread(reads)
    raw = store.text(seq=True)
    ctp0, _, st0, _ = LR.links(raw, k)
    ctp, lst, st, _ = LR.links(raw, k, clean=C["clean"])
    counts0 = sorted(int(ln.split()[2]) for ln in ctp0.decode().splitlines() if ln[0] in "FR" and ln[1] == " ")
    counts = sorted(int(ln.split()[2]) for ln in ctp.decode().splitlines() if ln[0] in "FR" and ln[1] == " ")
    assert set(counts0) == {C["err_copies"], C["ref_copies"]} and set(counts) == {C["ref_copies"]}
    assert len(counts) == counts0.count(C["ref_copies"]) > 0 and st["num_links"] == len(counts) < st0["num_links"]
    # a true link carries the junction base of a true sequence: its seq= is a substring of one (or of its reverse complement)
    for ln in ctp.decode().splitlines():
        if ln[:2] in ("F ", "R "):
            seq = ln.split(" seq=")[1].split(" ")[0]
            assert any(seq in s or LC.revcomp(seq) in s for s in C["ref"]), ln
    assert all(int(r.split(",")[1]) >= C["clean"] for r in lst.decode().split())


def test_golden_is_current():
    for name, c in GOLDEN["hand"].items():
        hist = tuple(c["hist"]) if "hist" in c else None
        ctp, lst, st, hists = LR.links(c["text"].encode(), c["k"], clean=c.get("clean"), hist=hist, limit=c.get("limit", 0))
        assert (ctp.decode(), lst.decode(), st, hists) == (c["ctp"], c["list"], c["stats"], c["hists"]), name
    assert GOLDEN["hand"]["quirk"]["ctp"] == "ACGTA 1\nF 2 2 AC seq=ACGTAAGC juncpos=0,2\n" and GOLDEN["hand"]["quirk_clean5"]["ctp"] == ""
    import hashlib
    for g in GOLDEN["generated"]:
        if g["option"] in ("plain", "clean9_hist"):
            text = LC.generated(g["k"], g["nkmers"], g["seed"])
            opt = {"plain": {}, "clean9_hist": {"clean": 9, "hist": (6, 100)}}[g["option"]]
            ctp, lst, st, _ = LR.links(text, g["k"], **opt)
            assert (hashlib.sha256(text).hexdigest(), hashlib.sha256(ctp).hexdigest(), hashlib.sha256(lst).hexdigest(), st) == \
                (g["input_sha256"], g["ctp_sha256"], g["list_sha256"], g["stats"])
    assert os.path.getsize(os.path.join(HERE, "golden", "links.json")) < 16384


@pytest.mark.parametrize("k", LC.SHARED_KS)
def test_shared_high_words(k):
    """the file of k-mers that agree in their high key words is what it says: every k-mer is canonical as the groups hold
    it, a group that differs in the last word agrees in every other, a group of word j agrees above it, differs in it and
    sorts the other way round below it; the file holds the last group's k-mers turned round, and the usual noise"""
    text, groups = LC.shared_high_words(k)
    W = (2 * k + 63) // 64
    assert text == LC.shared_high_words(k)[0] and W == {63: 2, 95: 3, 127: 4}[k]
    assert sorted(j for j, _, _ in groups) == list(range(1, W - 1)) + [W - 1] * 4
    lines = text.decode().split("\n")
    heads = [ln.split(" ")[0] for ln in lines if ln[:1] in ("A", "C", "G", "T")]
    assert len(heads) == len(set(heads)) == sum(len(kmers) for _, kmers, _ in groups)
    assert heads != sorted(heads) and any(ln == "" for ln in lines[:-1]) and any(ln.startswith("#") for ln in lines)
    for j, kmers, turned in groups:
        assert len(kmers) >= 4 and len(set(kmers)) == len(kmers)
        words = [LC.key_words(s) for s in kmers]
        for s in kmers:
            assert len(s) == k and R.canon(R.kmer_int(s), k) == R.kmer_int(s)
            assert (LC.revcomp(s) if turned else s) in heads and (s if turned else LC.revcomp(s)) not in heads
        assert len({tuple(w[:j]) for w in words}) == 1 and len({w[j] for w in words}) == len(kmers)
        if j == W - 1:
            assert len({s[:32 * (W - 1)] for s in kmers}) == 1
        else:
            by_j = sorted(words, key=lambda w: w[j])
            assert by_j == sorted(words) and by_j == sorted(words, key=lambda w: w[j + 1:], reverse=True)
    assert sum(turned for _, _, turned in groups) == 1
    # the words are those of the packed records
    s = groups[0][1][0]
    assert R.pack({R.kmer_int(s): ((1,), [0])}, k, 1)[:8 * W] == b"".join(w.to_bytes(8, "little") for w in LC.key_words(s))
    # what a graph keeps of it: the turned k-mers under their canonical keys, their links the other way round
    links = LC.stored(text, k)
    assert {key for key, _, _, _ in links} == {R.kmer_int(s) for _, kmers, _ in groups for s in kmers}
    turned = next(kmers for _, kmers, t in groups if t)
    blk = next(b.decode() for b in LC.blocks_of(text) if LC.revcomp(turned[0]) + " " in b.decode())
    ln = next(x for x in blk.split("\n") if x[:2] in ("F ", "R "))
    assert (R.kmer_int(turned[0]), "RF".index(ln[0]), tuple("ACGT".index(c) for c in ln.split(" ")[3])) in {l[:3] for l in links}
    assert all(1 <= n <= 255 for _, _, _, n in links) and any(n == 255 for _, _, _, n in links)
    ctp, lst, st, _ = LR.links(text, k)
    assert st["kmers_read"] == len(heads) and st["links_in"] > st["num_links"] > 0


def test_generators_cover_the_ground():
    text = LC.generated(31, 200, seed=31)
    lines = text.decode().split("\n")
    assert any(ln == "" for ln in lines[:-1]) and any(ln.startswith("#") for ln in lines)
    blocks = LC.blocks_of(text)
    assert len(blocks) == 200 and not any(ln.startswith("F ") for ln in blocks[1].decode().split("\n"))
    ctp, lst, st, _ = LR.links(text, 31)
    assert st["links_in"] > st["num_links"] > 0 and st["tree_links"] > st["links_in"]
    assert max(int(ln.split()[2]) for ln in ctp.decode().splitlines() if ln[:2] in ("F ", "R ")) > 300  # duplicates added up
    assert subprocess.run([sys.executable, "-c", "import links_restate"], cwd=HERE).returncode == 0
