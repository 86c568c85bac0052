"""pjoin_restate.py pinned by hand-written vectors (golden/pjoin.json): the reference's tests/pjoin/pjoin0 shape (k = 9, two
two-read genomes, their link files merged into two colours and, with `0:` offsets, into one), the pjoin1 shape (A, A, B, A,
B into five colours), saturation, a dropped line and the k-mer that goes with it, a prefix kept beside its extension, F and
R kept apart, one k-mer in two blocks, the merged header with a histogram sum, and a sample-name clash."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import links_cases as LC  # noqa: E402
import pjoin_cases as PC  # noqa: E402
import pjoin_restate as PR  # noqa: E402
import thread_restate as T  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "pjoin.json")))


def merged(k, ncols, adds):
    r = PR.Pjoin(k, ncols)
    for a in adds:
        r.add(*a)
    return r


def test_pjoin0_and_pjoin1_shapes():
    G = GOLDEN["pjoin0"]
    k = G["k"]
    bodies = [T.Store(R.build([g], k), k).thread(g).text(seq=True) for g in G["genomes"]]
    assert [b.decode() for b in bodies] == G["bodies"]
    A, B = bodies
    two = merged(k, 2, [(A, 1, [(0, 0)]), (B, 1, [(0, 1)])])
    assert two.text().decode() == G["two_colours"] and two.info() == {"num_kmers_with_paths": 4, "num_paths": 8, "path_bytes": 8}
    assert PR.default_filters([1, 1]) == [[(0, 0)], [(0, 1)]]
    one = merged(k, 1, [(A, 1, [(0, 0)]), (B, 1, [(0, 0)])])
    assert one.text().decode() == G["one_colour"]
    assert G["one_colour"].startswith("CTAGGCGAC 2\nF 1 1 A\nF 1 1 C\nGGCGACACA 2\nR 1 1 C\nR 1 1 G\n")
    five = merged(k, 5, [(f, 1, flt) for f, flt in zip((A, A, B, A, B), PR.default_filters([1] * 5))])
    assert five.text().decode() == GOLDEN["pjoin1"]["five_colours"]
    for line in five.text().decode().split("\n"):
        if line[:1] in ("F", "R"):
            c = line.split(" ")[2].split(",")
            assert c[0] == c[1] == c[3] and c[2] == c[4] and {c[0], c[2]} == {"0", "1"}


@pytest.mark.parametrize("name", sorted(GOLDEN["small"]))
def test_small_cases(name):
    G = GOLDEN["small"][name]
    r = merged(G["k"], G["ncols"], [(a["text"].encode(), a["src_ncols"], [tuple(f) for f in a["filter"]]) for a in G["adds"]])
    i = r.info()
    assert r.text().decode() == G["body"] and [i["num_kmers_with_paths"], i["num_paths"], i["path_bytes"]] == G["totals"]


def test_the_vectors_say_what_they_should():
    S = GOLDEN["small"]
    assert S["sat_200_100"]["body"] == S["sat_300"]["body"] == "ACGTA 1\nF 2 255 AC\n" and S["sat_255_0"]["body"] == "ACGTA 1\nF 2 255,7 AC\n"
    assert "CCGTA" in S["dropped"]["adds"][0]["text"] and S["dropped"]["body"] == "ACGTA 1\nF 1 4 C\n"
    assert S["prefix"]["body"].split("\n")[1:4] == ["F 2 1 AC", "F 3 1 ACG", "F 4 1 ACGT"]
    assert S["both_ways"]["body"] == "ACGTA 2\nF 2 5 AC\nR 2 6 AC\n"
    assert S["two_blocks"]["body"] == "ACGTA 2\nF 1 5 A\nR 1 1 C\nGGGTA 1\nF 1 1 T\n"


def test_line_counts_order_of_addition_and_refusals():
    r = PR.Pjoin(5, 1)
    assert r.add(PC.ALL_DROPPED, 1, [(0, 0)]) == {"kmer_lines": 2, "link_lines": 3, "links_kept": 0, "kmers_n_mismatch": 0}
    assert r.text() == b"" and r.info() == {"num_kmers_with_paths": 0, "num_paths": 0, "path_bytes": 0}
    assert r.add(b"ACGTA 3\nF 1 1 A\nCCGTA 0\nF 1 1 A\n")["kmers_n_mismatch"] == 2
    texts = [b"ACGTA 1\nF 1 200 A\n", b"ACGTA 1\nF 1 100 A\n", b"ACGTA 1\nF 1 1 A\n"]
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        assert merged(5, 1, [(texts[i], 1, [(0, 0)]) for i in order]).text() == b"ACGTA 1\nF 1 255 A\n"
    for body, src_ncols, code, line in PC.REFUSALS:
        r = PR.Pjoin(5, 2)
        with pytest.raises(PR.BadLine) as e:
            r.add(body, src_ncols, [(c, c) for c in range(src_ncols)])
        assert (e.value.code, e.value.offset) == (code, PC.line_offset(body, line)) and r.store == {}
    with pytest.raises(ValueError):
        PR.Pjoin(5, 1).add(b"ACGTA 1\nF 1 1 A\n", 1, [(0, 1)])


def test_merged_header():
    def hdr(ncols, names, hists, commands):
        h = json.loads(LC.header(9, ncols=ncols, commands=commands))
        for c in range(ncols):
            h["graph"]["colours"][c]["sample"] = names[c]
        h["paths"]["contig_hists"] = [{"lengths": [x for x, _ in hh], "counts": [y for _, y in hh]} for hh in hists]
        return h
    ca, cb, cc = {"key": "aaaa", "cmd": ["thread"], "prev": []}, {"key": "bbbb", "cmd": ["build"], "prev": []}, {"key": "cccc", "cmd": ["links"], "prev": ["aaaa"]}
    a = hdr(1, ["Gnome0"], [[(0, 9), (20, 2), (31, 4)]], [cc, ca, cb])
    b = hdr(2, ["Gnome0", "Gnome \"1\" {"], [[(20, 0), (31, 1), (40, 5)], []], [ca])
    info = {"num_kmers_with_paths": 4, "num_paths": 8, "path_bytes": 8}
    # a.ctp into 0; b.ctp:0 into 0 as well, b.ctp:1 into 2; colour 1 is filled by nobody
    h = PR.merged_header(9, 3, [(a, [(0, 0)]), (b, [(0, 0), (1, 2)])], info)
    assert [c["sample"] for c in h["graph"]["colours"]] == ["Gnome0", "undefined", "Gnome \"1\" {"]
    assert all(c["total_sequence"] == 0 and c["cleaned_tips"] is False and c["cleaned_unitigs"] is False for c in h["graph"]["colours"])
    assert h["graph"]["num_kmers_in_graph"] == 4 and h["graph"]["num_colours"] == 3 and h["format_version"] == 4 and h["file_format"] == "ctp"
    assert h["commands"][0]["prev"] == ["cccc", "aaaa"] and h["commands"][1:] == [cc, ca, cb]  # each key once, input order
    assert h["paths"]["contig_hists"] == [{"lengths": [20, 31, 40], "counts": [2, 5, 5]}, {"lengths": [], "counts": []}, {"lengths": [], "counts": []}]
    assert {n: h["paths"][n] for n in info} == info
    with pytest.raises(PR.SampleClash):
        PR.merged_header(9, 1, [(a, [(0, 0)]), (b, [(1, 0)])], info)
    empty = hdr(1, ["undefined"], [[]], [])
    h = PR.merged_header(9, 1, [(empty, [(0, 0)]), (a, [(0, 0)])], info)
    assert h["commands"][0]["prev"] == ["cccc"] and h["graph"]["colours"][0]["sample"] == "Gnome0"
