"""`links` on the MI355X (mccortex_amd.Links, csrc/mcx_links.h; the `links` command) against the CPU restatement in
links_restate.py: the .ctp body and the list text byte for byte, the statistics and the histogram by exact equality.
Generated files of links_cases.py (k = 5, 31, 33, 63, 65, 95, 97, 127) and its files of k-mers that agree in their high
key words (k = 63, 95, 127) under every option; links around the 32-junction word seams; one hot
k-mer as a comb and as a bush of 4096 links (their expected texts are kept as digests in golden/links.json, written from
the restatement, which takes its time over 8 million tree steps); the file in pieces, with "grid" = 1 and an
"out_chunk" of 64 bytes; every refusal; the device's own links; the command."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import links_cases as LC  # noqa: E402
import links_restate as LR  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "links.json")))
OPTIONS = {"plain": {}, "clean2": {"clean": 2}, "clean1000": {"clean": 1000}, "hist": {"hist": (6, 100)}, "hist3x4": {"hist": (3, 4)},
           "clean9_hist": {"clean": 9, "hist": (6, 100)}}


def want_stats(st):
    return {"kmers_read": st["kmers_read"], "kmers_with_links": st["num_trees_with_links"], "links": st["num_links"],
            "link_bytes": st["num_link_bytes"], "tree_links": st["tree_links"], "links_in": st["links_in"]}


def differ(got, want, what):
    if got != want:
        a, b = got.splitlines(), want.splitlines()
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError((what, i, a[i:i + 2], b[i:i + 2], len(a), len(b)))


def run(k, pieces, knobs=(), max_kmers=0, **opt):
    """the pieces through one handle -> (ctp, list, stats, hist or None)"""
    L = mcx.Links(k)
    for key, v in knobs:
        L.configure(key, v)
    ctp, lst, left = [], [], max_kmers
    for p in pieces:
        if max_kmers and left == 0:
            break
        before = L.stats()["kmers_read"]
        a, b = L.add(p, max_kmers=left, **opt)
        left -= L.stats()["kmers_read"] - before if max_kmers else 0
        ctp.append(a)
        lst.append(b)
    st = L.stats()
    hist = L.hist().tolist() if opt.get("hist") and L.hist_shape else None
    chunks = L.chunks
    L.close()
    return b"".join(ctp), b"".join(lst), st, hist, chunks


def check(k, text, what, pieces=None, knobs=(), max_kmers=0, **opt):
    ctp, lst, st, hists = LR.links(text, k, limit=max_kmers, **opt)
    got = run(k, pieces if pieces is not None else [text], knobs, max_kmers, **opt)
    differ(got[0], ctp, what + ": .ctp")
    differ(got[1], lst, what + ": list")
    assert got[2] == want_stats(st), what
    if opt.get("hist"):
        assert got[3] == hists, what
    return got


FILES = {k: LC.generated(k, n, seed=k) for k, n in ((5, 300), (31, 200), (33, 200), (63, 200), (65, 200), (95, 200), (97, 200), (127, 200))}


@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("k", sorted(FILES))
def test_generated(k, name):
    got = check(k, FILES[k], "k=%d %s" % (k, name), **OPTIONS[name])
    if name == "clean1000":
        # (no link is left; a shared stem of many links can still count 1000 and keep its list row)
        assert got[0] == b"" and got[2]["links"] == 0 and got[2]["kmers_with_links"] == 0 and got[1].count(b"\n") < got[2]["tree_links"] // 10
    if name == "plain":
        assert got[2]["links"] > 0 and b"\nR " in got[0] and got[2]["links"] < got[2]["links_in"]


@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("k", LC.SHARED_KS)
def test_keys_that_agree_in_their_high_words(k, name):
    """k-mers in groups that differ in their last bases only, or first in a middle key word, some written as the reverse
    complement: the blocks come out per k-mer line as written, in the order of the file"""
    text, groups = LC.shared_high_words(k)
    got = check(k, text, "shared k=%d %s" % (k, name), **OPTIONS[name])
    if name == "plain":
        heads = [ln.split(b" ")[0] for ln in text.split(b"\n") if ln[:1] in (b"A", b"C", b"G", b"T")]
        assert [ln.split(b" ")[0] for ln in got[0].split(b"\n") if ln[:1] in (b"A", b"C", b"G", b"T")] == heads
        assert got[2]["kmers_read"] == len(heads) == sum(len(kmers) for _, kmers, _ in groups)


def test_word_seams():
    text = LC.seams()
    for name in ("plain", "clean9_hist", "hist3x4"):
        check(31, text, "seams " + name, **OPTIONS[name])
    ctp = check(31, text, "seams clean 5", clean=5)[0]
    assert b"F 1000 " in ctp and ctp.count(b"\nF 65 ") == 2 and ctp.count(b"\nR 33 ") >= 2


def digest(b):
    return hashlib.sha256(b).hexdigest()


@pytest.mark.parametrize("name", ["comb", "bush"])
def test_one_hot_kmer(name):
    """4096 links on one k-mer, each the prefix of the next (comb) or all 4^6 strings (bush), cleaned mid-depth"""
    G = GOLDEN["hot"][name]
    text = LC.comb(G["n"]) if name == "comb" else LC.bush(G["depth"])
    assert digest(text) == G["input_sha256"]
    for case in G["cases"]:
        opt = {"clean": case["clean"]} if case["clean"] is not None else {}
        ctp, lst, st, hist, _ = run(5, [text], hist=(6, 100), **opt)
        print(name, case["clean"], st, len(ctp), len(lst))
        assert st == case["stats"], (name, case["clean"])
        assert (digest(ctp), len(ctp)) == (case["ctp_sha256"], case["ctp_bytes"])
        assert (digest(lst), len(lst)) == (case["list_sha256"], case["list_bytes"])
        assert [[d, c, n] for d, row in enumerate(hist) for c, n in enumerate(row) if n] == case["hists_nonzero"]
        assert lst.count(b"\n") < st["tree_links"] if case["clean"] else lst.count(b"\n") == st["tree_links"]


def test_pieces():
    k, text = 5, FILES[5]
    opt = {"clean": 2, "hist": (6, 100)}
    whole = check(k, text, "one call", **opt)
    blocks = LC.blocks_of(text)
    assert b"".join(blocks) == text and len(blocks) == 300
    per_kmer = check(k, text, "a k-mer per call", pieces=blocks, **opt)
    cuts = [0, 1, 1, 7, 120, 121, 299, 300]  # (an empty piece among them)
    uneven = check(k, text, "uneven pieces", pieces=[b"".join(blocks[a:b]) for a, b in zip(cuts, cuts[1:])], **opt)
    grid1 = check(k, text, "grid 1", knobs=[("grid", 1)], **opt)
    small = check(k, text, "out_chunk 64", knobs=[("out_chunk", 64)], **opt)
    assert max(small[4][0]) == 64 and max(small[4][1]) == 64 and len(small[4][0]) == (len(whole[0]) + 63) // 64
    for other in (per_kmer, uneven, grid1, small):
        assert other[:4] == whole[:4]
    # max_kmers inside a piece: 130 k-mers out of pieces of 100
    lim = check(k, text, "max_kmers", pieces=[b"".join(blocks[a:a + 100]) for a in (0, 100, 200)], max_kmers=130, **opt)
    assert lim[2]["kmers_read"] == 130
    assert check(k, text, "max_kmers, one call", max_kmers=130, **opt)[:4] == lim[:4]


GOOD = "F 2 3 AC seq=ACGTAGAGC juncpos=1,3"  # k = 5
BAD = [
    ("bad_kmer_line", "ACGT 1"), ("bad_kmer_line", "ACGTA"), ("bad_kmer_line", "ACGTA x"), ("bad_kmer_line", "ACGNA 1"), ("bad_kmer_line", "ACGTAC 1"),
    ("bad_orient", "X 2 3 AC seq=ACGTAGAGC juncpos=1,3"), ("bad_orient", "FR 2 3 AC seq=ACGTAGAGC juncpos=1,3"), ("bad_orient", "f 1 1 A"),
    ("bad_number", "F x 3 AC seq=ACGTAGAGC juncpos=1,3"), ("bad_number", "F 2 y AC seq=ACGTAGAGC juncpos=1,3"), ("bad_number", "F 2"), ("bad_number", "F 2 3"),
    ("multi_colour", "F 2 3,4 AC seq=ACGTAGAGC juncpos=1,3"),
    ("bad_junction", "F 2 3 AN seq=ACGTAGAGC juncpos=1,3"),
    ("njuncs_range", "F 0 3  seq=ACGTA juncpos=0"), ("njuncs_range", "F 32768 3 AC seq=ACGTAGAGC juncpos=1,3"),
    ("njuncs_length", "F 3 3 AC seq=ACGTAGAGC juncpos=1,3"),
    ("no_seq", "F 2 3 AC juncpos=1,3"), ("no_seq", "F 2 3 AC"), ("no_juncpos", "F 2 3 AC seq=ACGTAGAGC"),
    ("juncpos_count", "F 2 3 AC seq=ACGTAGAGC juncpos=1"), ("juncpos_count", "F 2 3 AC seq=ACGTAGAGC juncpos=1,3,4"),
    ("juncpos_count", "F 2 3 AC seq=ACGTAGAGC juncpos=1,x"), ("juncpos_count", "F 2 3 AC seq=ACGTAGAGC juncpos=1,"),
    ("seq_length", "F 2 3 AC seq=ACGTAGAGCA juncpos=1,3"), ("seq_length", "F 2 3 AC seq=ACGTAGAG juncpos=1,3"),
    ("seq_base", "F 2 3 AC seq=ACGTAGTGC juncpos=1,3"), ("seq_base", "F 2 3 AC seq=ACGTAGAGC juncpos=5,3"),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_refusals(i):
    code, line = BAD[i]
    text = "# c\nACGTA 1\n%s\n\n%s\nCCCCC 1\n%s\n" % (GOOD, line, GOOD)
    off = text.index("\n" + line + "\n") + 1
    with pytest.raises(LR.BadLine) as want:
        LR.links(text.encode(), 5)
    assert (want.value.code, want.value.offset) == (code, off)
    L = mcx.Links(5)
    with pytest.raises(mcx.McxError) as ei:
        L.add(text.encode())
    assert ei.value.code == mcx.graph.MCX_ERR_INVAL
    assert L.error() == (code, off)
    assert L.stats()["kmers_read"] == 0  # nothing of a refused piece counts
    L.close()


def test_refusal_order_and_limit():
    L = mcx.Links(5)
    with pytest.raises(mcx.McxError):
        L.add(("%s\nACGTA 1\n%s\n" % (GOOD, GOOD)).encode())
    assert L.error() == ("link_before_kmer", 0)
    with pytest.raises(LR.BadLine) as want:
        LR.links(("%s\nACGTA 1\n%s\n" % (GOOD, GOOD)).encode(), 5)
    assert (want.value.code, want.value.offset) == ("link_before_kmer", 0)
    # two bad lines in one piece: the first in file order is reported, whatever the launch shape
    text = "ACGTA 2\n%s\nF 2 3 AN seq=ACGTAGAGC juncpos=1,3\n" % GOOD + "".join("CC%sC 1\n%s\n" % (a + b, GOOD) for a in "ACGT" for b in "ACGT") * 40 + "F 9\n"
    for grid in (0, 1):
        L.configure("grid", grid)
        with pytest.raises(mcx.McxError):
            L.add(text.encode())
        assert L.error() == ("bad_junction", text.index("F 2 3 AN"))
    L.close()


def test_limit_hides_later_lines():
    L = mcx.Links(5)
    text = ("ACGTA 1\n%s\nCCCCC 1\nF 9\n" % GOOD).encode()
    ctp, lst = L.add(text, max_kmers=1)
    assert ctp == ("ACGTA 1\n%s\n" % GOOD).encode() and lst == b"7,3\n9,3\n"
    assert LR.links(text, 5, limit=1)[:2] == (ctp, lst)
    with pytest.raises(mcx.McxError):
        L.add(text)
    assert L.error() == ("bad_number", text.index(b"F 9"))
    with pytest.raises(mcx.McxError) as ei:
        L.add(text[:-1])
    assert ei.value.code == mcx.graph.MCX_ERR_ARG
    L.close()


def test_from_the_devices_own_links():
    """a small graph threaded on the device; its links_text(seq=True) through Links, against the restatement fed the
    text of thread_restate.py"""
    import clean_restate as R
    import thread_cases as TC
    import thread_restate as T
    k = 31
    graph, reads, _ = TC.case(k)
    g = mcx.Graph(k, 1, 1 << 16)
    g.add_records(R.pack(graph, k, 1), 1, [(0, 0)])
    g.sync()
    seqs = [s.encode() for s in reads]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    g.thread(np.frombuffer(b"".join(seqs), dtype=np.uint8), offs)
    raw = g.links_text(seq=True)
    g.close()
    want_raw = T.Store(graph, k).thread(reads).text(seq=True)
    assert raw == want_raw and raw.count(b"\n") > 100
    for name in ("plain", "clean2", "clean9_hist"):
        ctp, lst, st, hists = LR.links(want_raw, k, **OPTIONS[name])
        got = run(k, [raw], **OPTIONS[name])
        differ(got[0], ctp, name)
        differ(got[1], lst, name)
        assert got[2] == want_stats(st) and (got[3] == hists or "hist" not in OPTIONS[name])
    assert LR.links(want_raw, k)[2]["num_links"] < LR.links(want_raw, k)[2]["links_in"]  # (prefixes of longer links are not kept)


BIN = os.path.join(os.path.dirname(HERE), "mccortex_amd", "bin")


def cli(*args, env=None):
    p = subprocess.run([os.path.join(BIN, "mccortex31")] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


def test_the_command(tmp_path):
    """the reference's tests/clean_links pipeline: build, thread -o raw.ctp.gz, links -H -T, links -c 2 -l -o"""
    import clean_restate as R
    import thread_restate as T
    C = json.load(open(os.path.join(HERE, "golden", "clean_links.json")))
    k = C["k"]
    reads = C["ref"] * C["ref_copies"] + C["err"] * C["err_copies"]
    d = tmp_path
    (d / "reads.txt").write_text("".join(s + "\n" for s in reads))
    ctx, raw, clean = d / "g.ctx", d / "raw.ctp.gz", d / "clean.ctp.gz"
    rc, _, err = cli("build", "-q", "-k", k, "-s", "s", "-1", d / "reads.txt", ctx)
    assert rc == 0, err
    rc, _, err = cli("thread", "-q", "--seq", d / "reads.txt", "-o", raw, ctx)
    assert rc == 0, err
    hdr0, body0 = LC.split_ctp(gzip.open(raw).read())
    want_raw = T.Store(R.build([reads], k), k).thread(reads).text(seq=True)
    assert body0.endswith(want_raw)

    rc, out, err = cli("links", "-H", d / "h.csv", "-T", d / "t.txt", raw)
    assert rc == 0 and out == b"", err
    _, _, st0, hists = LR.links(want_raw, k, hist=(6, 100))
    assert (d / "h.csv").read_text() == LR.hist_csv(hists, 6, 100)
    assert (d / "t.txt").read_text() == LR.threshold_text(hists, 100, R.pick_threshold)
    for line in ("Number of kmers with links %d -> %d" % (hdr0["paths"]["num_kmers_with_paths"], st0["num_trees_with_links"]),
                 "Number of links %d -> %d" % (hdr0["paths"]["num_paths"], st0["num_links"]),
                 "Number of bytes %d -> %d" % (hdr0["paths"]["path_bytes"], st0["num_link_bytes"])):
        assert line in err, err
    assert sorted(os.listdir(d)) == ["g.ctx", "h.csv", "raw.ctp.gz", "reads.txt", "t.txt"]  # (nothing saved without -o, no temporary left)

    argv = ["links", "-c", 2, "-l", d / "l.csv", "-o", clean, raw]
    rc, out, err = cli(*argv)
    assert rc == 0 and out == b"", err
    ctp, lst, st, _ = LR.links(want_raw, k, clean=2)
    assert (d / "l.csv").read_bytes() == b"SeqLen,Covg\n" + lst
    hdr, body = LC.split_ctp(gzip.open(clean).read())
    lines = body.decode().split("\n")
    assert lines[0] == "" and lines[1] == "" and lines[2].startswith("# ")
    assert "\n".join(ln for ln in lines if ln and ln[0] != "#").encode() + b"\n" == ctp and body.endswith(ctp)
    assert 0 < st["num_links"] <= st0["num_links"]
    # the header: the input's, but for the key, the totals and one new first command
    new, old = hdr["commands"][0], hdr0["commands"][0]
    assert hdr["commands"][1:] == hdr0["commands"] and new["prev"] == [old["key"]] and new["key"] != old["key"] and len(new["key"]) == 8
    assert new["cmd"] == ["mccortex31"] + [str(a) for a in argv] and new["out_path"] == str(clean) and new["out_key"] == hdr["file_key"]
    assert set(new) == set(old) - {"thread"} and hdr["file_key"] != hdr0["file_key"] and len(hdr["file_key"]) == 16
    assert hdr["paths"] == dict(hdr0["paths"], num_kmers_with_paths=st["num_trees_with_links"], num_paths=st["num_links"], path_bytes=st["num_link_bytes"])
    assert {key: v for key, v in hdr.items() if key not in ("file_key", "commands", "paths")} == \
        {key: v for key, v in hdr0.items() if key not in ("file_key", "commands", "paths")}
    assert "Cleaning coverage below 2" in err and "Saving output to: %s" % clean in err
    # again on its own output: the same body; in pieces of a few hundred bytes and with -L
    rc, _, err = cli("links", "-q", "-c", 2, "-o", d / "again.ctp.gz", clean, env={"MCX_LINKS_PIECE": "300"})
    assert rc == 0, err
    hdr2, body2 = LC.split_ctp(gzip.open(d / "again.ctp.gz").read())
    assert body2 == body and len(hdr2["commands"]) == 3 and hdr2["commands"][0]["prev"] == [new["key"]] and hdr2["paths"] == hdr["paths"]
    rc, _, err = cli("links", "-q", "-L", 3, "-l", d / "l3.csv", raw, env={"MCX_LINKS_PIECE": "64"})
    assert rc == 0, err
    assert (d / "l3.csv").read_bytes() == b"SeqLen,Covg\n" + LR.links(want_raw, k, limit=3)[1]
    # the cut-off of the reference's pipeline: the links of the recombinant reads go
    rc, _, err = cli("links", "-q", "--clean", C["clean"], "--out", d / "clean5.ctp.gz", raw)
    assert rc == 0, err
    ctp5, _, st5, _ = LR.links(want_raw, k, clean=C["clean"])
    hdr5, body5 = LC.split_ctp(gzip.open(d / "clean5.ctp.gz").read())
    assert body5.endswith(ctp5) and 0 < hdr5["paths"]["num_paths"] == st5["num_links"] < st0["num_links"]
    # a bad line is named with its place
    LC.ctp_file(str(d / "bad.ctp.gz"), k, want_raw + b"F 1 1 N seq=A juncpos=0\n")
    rc, _, err = cli("links", "-l", d / "bad.csv", d / "bad.ctp.gz")
    assert rc == 1 and "Non-ACGT base in junction choices" in err and "F 1 1 N seq=A juncpos=0" in err
