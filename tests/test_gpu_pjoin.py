"""`pjoin` on the MI355X (mccortex_amd.Pjoin, csrc/mcx_pjoin.h; the `pjoin` command) against the CPU restatement in
pjoin_restate.py: the merged body byte for byte, the totals and the line counts by exact equality.  Generated files of
pjoin_cases.py at one, two and three key words and 1, 2, 3 and 9 colours; the arrangements of the files; links around the
32-junction word seams; saturation and dropped lines; one hot k-mer and one hot link; the knobs that must not change an
answer, compaction and the store's ceiling among them; every refusal; round trips with `thread` and the link loader of
`contigs`; the command."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import links_cases as LC  # noqa: E402
import pjoin_cases as PC  # noqa: E402
import pjoin_restate as PR  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "pjoin.json")))
PIECE_NAMES = ("kmer_lines", "link_lines", "links_kept", "kmers_n_mismatch")


def differ(got, want, what):
    if got != want:
        a, b = got.splitlines(), want.splitlines()
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError((what, i, a[i:i + 2], b[i:i + 2], len(a), len(b)))


def run(k, ncols, adds, knobs=()):
    """adds: [(text, src_ncols, filter)] through one handle -> (body, stats, piece stats, chunks)"""
    P = mcx.Pjoin(k, ncols)
    for key, v in knobs:
        P.configure(key, v)
    ps = [P.add(*a) for a in adds]
    body = P.finish()
    st, chunks = P.stats(), P.chunks
    P.close()
    return body, st, ps, chunks


def want(k, ncols, adds):
    R = PR.Pjoin(k, ncols)
    ps = [R.add(*a) for a in adds]
    return R.text(), R.info(), ps, R.totals


def check(k, ncols, adds, what, knobs=()):
    body, info, ps, totals = want(k, ncols, adds)
    got = run(k, ncols, adds, knobs)
    differ(got[0], body, what)
    assert got[2] == ps, what
    st = got[1]
    assert {n: st[n] for n in PIECE_NAMES} == totals, what
    assert (st["kmers"], st["links"], st["path_bytes"]) == (info["num_kmers_with_paths"], info["num_paths"], info["path_bytes"]), what
    return got


def identity(n, at=0):
    return [(c, at + c) for c in range(n)]


@pytest.mark.parametrize("ncols", [1, 2, 3, 9])
@pytest.mark.parametrize("k", [5, 9, 31, 33, 95])
def test_key_widths_and_colours(k, ncols):
    """two generated files of `ncols` colours each at default offsets, then the first again into the colours of the second"""
    a, b = PC.generated(k, 200, ncols, seed=k), PC.generated(k, 150, ncols, seed=k + 7)
    if k == 33:
        a += PC.recount(PC.second_word(k), ncols, 3, zero=0.0)
    adds = [(a, ncols, identity(ncols)), (b, ncols, identity(ncols, ncols)), (a, ncols, identity(ncols, ncols))]
    body, st, ps, _ = check(k, 2 * ncols, adds, "k=%d ncols=%d" % (k, ncols))
    assert st["links"] > 400 and st["links_kept"] > st["links"] and ps[0]["links_kept"] < ps[0]["link_lines"] and b"\nR " in body
    if k == 33:
        stem = PC.second_word(k)[:32]
        assert body.count(stem) == 2


def test_second_word_kmers():
    body = check(33, 1, [(PC.second_word(), 1, [(0, 0)])], "second word")[0]
    lines = body.decode().split("\n")
    assert lines[0][:32] == lines[3][:32] and lines[0][32] == "A" and lines[3][32] == "C" and lines[1] == "F 2 3 AC" and lines[4] == "F 2 5 AC"


ARR = PC.generated(9, 120, 2, seed=41), PC.generated(9, 100, 2, seed=42)


@pytest.mark.parametrize("name", ["default", "all_into_0", "swap", "thrice"])
def test_arrangements(name):
    a, b = ARR
    if name == "default":  # a.ctp b.ctp
        ncols, adds = 4, [(a, 2, identity(2)), (b, 2, identity(2, 2))]
    elif name == "all_into_0":  # 0:a.ctp 0:b.ctp with every colour into 0
        ncols, adds = 1, [(a, 2, [(0, 0), (1, 0)]), (b, 2, [(0, 0), (1, 0)])]
    elif name == "swap":  # a.ctp 1:b.ctp:1,0
        ncols, adds = 3, [(a, 2, identity(2)), (b, 2, [(1, 1), (0, 2)])]
    else:  # 0:a.ctp 0:a.ctp 0:a.ctp
        ncols, adds = 2, [(a, 2, identity(2))] * 3
    body, st, _, _ = check(9, ncols, adds, name)
    assert st["links"] > 100
    if name == "thrice":
        one = want(9, 2, adds[:1])[0].decode().split("\n")
        for x, y in zip(one, body.decode().split("\n")):
            if x[:1] in ("F", "R"):
                assert [min(255, 3 * int(c)) for c in x.split(" ")[2].split(",")] == [int(c) for c in y.split(" ")[2].split(",")]


def test_word_seams():
    a, b = PC.shared(LC.seams(), seed=9)
    body, st, _, _ = check(31, 2, [(a, 1, [(0, 0)]), (b, 1, [(0, 1)])], "seams, two colours")
    assert b"F 1000 " in body and body.count(b"\nF 65 ") >= 4 and body.count(b"\nR 33 ") >= 2
    one = check(31, 1, [(a, 1, [(0, 0)]), (b, 1, [(0, 0)])], "seams, one colour")[0]
    assert one.count(b"\n") == body.count(b"\n")
    both = sum(1 for ln in body.decode().split("\n") if ln[:1] in ("F", "R") and "0" not in ln.split(" ")[2].split(","))
    assert 0 < both < st["links"]  # some links are in both files, some in one


@pytest.mark.parametrize("name", sorted(GOLDEN["small"]))
def test_small_cases(name):
    """the hand-written vectors of test_pjoin_restate.py on the device"""
    G = GOLDEN["small"][name]
    adds = [(a["text"].encode(), a["src_ncols"], [tuple(f) for f in a["filter"]]) for a in G["adds"]]
    body, st, ps, _ = run(G["k"], G["ncols"], adds)
    assert body.decode() == G["body"]
    assert [st["kmers"], st["links"], st["path_bytes"]] == G["totals"]
    check(G["k"], G["ncols"], adds, name)


def test_every_line_dropped():
    body, st, ps, chunks = check(5, 1, [(PC.ALL_DROPPED, 1, [(0, 0)])], "all dropped")
    assert body == b"" and chunks == [] and (st["kmers"], st["links"], st["path_bytes"], st["links_kept"]) == (0, 0, 0, 0)
    assert ps[0] == {"kmer_lines": 2, "link_lines": 3, "links_kept": 0, "kmers_n_mismatch": 0}


def test_hot_shapes():
    """one k-mer with 4096 distinct links merged with itself into two colours; one link 5000 times in one file"""
    bush = LC.bush(6)
    body, st, _, _ = check(5, 2, [(bush, 1, [(0, 0)]), (bush, 1, [(0, 1)])], "bush")
    assert st["links"] == 4096 and st["kmers"] == 1 and body.startswith(b"CCGTA 4096\nR 6 ")
    hot = ("ACGTA 5000\n" + "F 3 1 ACG\n" * 2500 + "R 3 1 ACG\n" + "F 3 2 ACG\n" * 2499).encode()
    body, st, _, _ = check(5, 1, [(hot, 1, [(0, 0)])], "hot link")
    assert body == b"ACGTA 2\nF 3 255 ACG\nR 3 1 ACG\n"
    few = ("ACGTA 100\n" + "F 3 2 ACG\n" * 100).encode()
    assert check(5, 1, [(few, 1, [(0, 0)])], "200")[0] == b"ACGTA 1\nF 3 200 ACG\n"


def pjoin1():
    """the reference's tests/pjoin/pjoin1: files A, A, B, A, B at default offsets, five colours"""
    a, b = (want(9, 1, [(PC.generated(9, 150, 1, seed=s), 1, [(0, 0)])])[0] for s in (51, 52))  # (every link once: compacting one file gains nothing)
    return [(f, 1, [(0, c)]) for c, f in enumerate((a, a, b, a, b))]


def test_invariance():
    k, ncols = 9, 4
    a, b = ARR
    adds = [(a, 2, identity(2)), (b, 2, identity(2, 2)), (a, 2, [(0, 3), (1, 0)])]
    whole = check(k, ncols, adds, "one piece a file")
    assert len(whole[3]) == 1
    grid1 = check(k, ncols, adds, "grid 1", knobs=[("grid", 1)])
    small = check(k, ncols, adds, "out_chunk 64", knobs=[("out_chunk", 64)])
    assert max(small[3]) == 64 and len(small[3]) == (len(whole[0]) + 63) // 64
    comp = check(k, ncols, adds, "compact 1", knobs=[("compact", 1)])
    assert comp[1]["compactions"] == 3 and whole[1]["compactions"] == 0 and comp[1]["store_bytes"] < whole[1]["store_bytes"]
    blocks = [(blk, n, f) for text, n, f in adds for blk in LC.blocks_of(text)]
    assert len(blocks) == 120 + 100 + 120
    per_block = check(k, ncols, blocks, "a block a piece")
    per_block_c = check(k, ncols, blocks[:60], "a block a piece, compact 1", knobs=[("compact", 1)])
    assert 50 < per_block_c[1]["compactions"] <= 60  # (a piece of which nothing is kept leaves nothing to compact)
    for other in (grid1, small, comp, per_block):
        assert other[0] == whole[0] and {n: other[1][n] for n in ("kmers", "links", "path_bytes") + PIECE_NAMES} == \
            {n: whole[1][n] for n in ("kmers", "links", "path_bytes") + PIECE_NAMES}


def test_store_ceiling():
    """A, A, B, A, B: with "max_bytes" at 0.7 of what the five files take uncompacted the merge passes only because the
    full store was compacted; with half of that the second file cannot enter: a compacted A and A's lines are more"""
    adds = pjoin1()
    free = check(9, 5, adds, "no ceiling")
    peak = free[1]["peak_store_bytes"]
    assert free[1]["compactions"] == 0 and peak == free[1]["store_bytes"]
    for line in free[0].decode().split("\n"):
        if line[:1] in ("F", "R"):
            c = line.split(" ")[2].split(",")
            assert c[0] == c[1] == c[3] and c[2] == c[4] and (c[0] != "0" or c[2] != "0")
    tight = check(9, 5, adds, "ceiling", knobs=[("max_bytes", peak * 7 // 10)])
    assert tight[0] == free[0] and tight[1]["compactions"] >= 1 and tight[1]["peak_store_bytes"] <= peak * 7 // 10
    P = mcx.Pjoin(9, 5)
    P.configure("max_bytes", peak * 7 // 20)
    P.add(*adds[0])
    with pytest.raises(mcx.McxError) as ei:
        P.add(*adds[1])
    assert ei.value.code == -3  # MCX_ERR_NOMEM
    assert P.stats()["compactions"] == 1  # a full store compacts once before it gives up
    # what was accepted is still there, and still right
    differ(P.finish(), want(9, 5, adds[:1])[0], "after MCX_ERR_NOMEM")
    P.close()


@pytest.mark.parametrize("i", range(len(PC.REFUSALS)))
def test_refusals(i):
    body, src_ncols, code, line = PC.REFUSALS[i]
    off = PC.line_offset(body, line)
    flt = identity(src_ncols)
    good = b"GGGTA 1\nF 2 3,9 CA\n" if src_ncols == 2 else b"GGGTA 1\nF 2 3 CA\n"
    R = PR.Pjoin(5, 2)
    with pytest.raises(PR.BadLine) as w:
        R.add(body, src_ncols, flt)
    assert (w.value.code, w.value.offset) == (code, off) and R.store == {}
    P = mcx.Pjoin(5, 2)
    P.add(good, src_ncols, flt)
    with pytest.raises(mcx.McxError) as ei:
        P.add(body, src_ncols, flt)
    assert ei.value.code == mcx.graph.MCX_ERR_INVAL
    assert P.error() == (code, off)
    P.add(good, src_ncols, flt)
    st = P.stats()
    assert (st["kmer_lines"], st["link_lines"], st["links_kept"]) == (2, 2, 2)  # nothing of a refused piece counts or is stored
    differ(P.finish(), want(5, 2, [(good, src_ncols, flt)] * 2)[0], code)
    P.close()


def test_first_bad_line_wins_and_filter_range():
    text = b"ACGTA 2\nF 2 3 AC\nF 2 3 AN\n" + b"".join(b"CC%sC 1\nF 1 1 A\n" % (a + b).encode() for a in "ACGT" for b in "ACGT") * 40 + b"F 9\n"
    P = mcx.Pjoin(5, 1)
    for grid in (0, 1):
        P.configure("grid", grid)
        with pytest.raises(mcx.McxError):
            P.add(text)
        assert P.error() == ("bad_junction", text.index(b"F 2 3 AN"))
    for flt, n in (([(1, 0)], 1), ([(0, 1)], 1), ([(0, 0), (2, 0)], 2)):
        with pytest.raises(mcx.McxError) as ei:
            P.add(b"ACGTA 1\nF 1 1 A\n" if n == 1 else b"ACGTA 1\nF 1 1,1 A\n", n, flt)
        assert ei.value.code == mcx.graph.MCX_ERR_ARG
    with pytest.raises(mcx.McxError) as ei:
        P.add(b"ACGTA 1\nF 1 1 A")
    assert ei.value.code == mcx.graph.MCX_ERR_ARG
    assert P.finish() == b""
    P.close()


def thread_texts(k, graph, read_sets):
    """links_text(seq=False) of a fresh handle per read set"""
    import clean_restate as R
    out = []
    for reads in read_sets:
        g = mcx.Graph(k, 1, 1 << 16)
        g.add_records(R.pack(graph, k, 1), 1, [(0, 0)])
        g.sync()
        seqs = [s.encode() for s in reads]
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        g.thread(np.frombuffer(b"".join(seqs), dtype=np.uint8), offs)
        out.append(g.links_text(seq=False))
        g.close()
    return out


def test_round_trips_with_thread():
    """links threaded from two read files into two handles and joined into one colour are the links of both files threaded
    into one handle (no count reaches 255); the link loader of `contigs` takes the output and gives it back unchanged"""
    import clean_restate as R
    import thread_cases as TC
    k = 31
    graph, reads, _ = TC.case(k)
    half = len(reads) // 2
    a, b, both = thread_texts(k, graph, [reads[:half], reads[half:], reads])
    assert a.count(b"\n") > 20 and b.count(b"\n") > 20 and a != b
    counts = [int(ln.split(b" ")[2]) for ln in both.split(b"\n") if ln[:1] in (b"F", b"R")]
    assert max(counts) < 255 and max(counts) > 1
    body = check(k, 1, [(a, 1, [(0, 0)]), (b, 1, [(0, 0)])], "thread a + thread b")[0]
    differ(body, both, "pjoin of two threads against one thread of both")
    g = mcx.Graph(k, 1, 1 << 16)
    g.add_records(R.pack(graph, k, 1), 1, [(0, 0)])
    g.sync()
    g.links_load_text(body)
    assert g.links_text(seq=False) == body
    g.close()


BIN = os.path.join(os.path.dirname(HERE), "mccortex_amd", "bin")
VOLATILE = ("key", "cwd", "out_path", "out_key", "date", "mccortex", "zlib", "user", "host", "os", "osrelease", "osversion", "hardware")


def cli(*args, env=None):
    p = subprocess.run([os.path.join(BIN, "mccortex31")] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


def read_ctp(path):
    hdr, body = LC.split_ctp(gzip.open(path).read())
    lines = body.decode().split("\n")
    assert lines[0] == "" and lines[1] == "" and lines[2].startswith("# ")  # header, an empty line, the comment block
    return hdr, "".join(ln + "\n" for ln in lines if ln and ln[0] != "#").encode(), body


def same_header(got, want, argv):
    """the header as parsed JSON: everything but the file key and what the command wrote about its run"""
    assert len(got["file_key"]) == 16 and set(got) == set(want)
    first = got["commands"][0]
    # (the dispatcher takes -q away before the command sees its arguments)
    assert first["cmd"] == ["mccortex31"] + [str(a) for a in argv if a != "-q"] and first["out_key"] == got["file_key"] and len(first["key"]) == 8
    assert first["prev"] == want["commands"][0]["prev"] and set(first) == set(VOLATILE) | {"cmd", "prev"}
    assert got["commands"][1:] == want["commands"][1:]
    for name in ("file_format", "format_version", "graph", "paths"):
        assert got[name] == want[name], name


def test_the_command_on_files_with_given_headers(tmp_path):
    """two gzipped inputs under headers of links_cases.header: default offsets, `0:` offsets in pieces of a few hundred
    bytes, a swap of colours; the death on totals that do not match and the warning on a wrong <n>"""
    d, k = tmp_path, 9
    a, b = PC.generated(k, 60, 1, seed=71), PC.generated(k, 50, 2, seed=72)
    ra, rb = PR.Pjoin(k, 1), PR.Pjoin(k, 2)
    ta, tb = ra.add(a), rb.add(b, 2)
    ka = dict(totals=(ta["kmer_lines"], ta["link_lines"], 0))
    kb = dict(totals=(tb["kmer_lines"], tb["link_lines"], 0), ncols=2, commands=[{"key": "11112222", "cmd": ["x"], "prev": []}, {"key": "aabbccdd", "cmd": ["y"], "prev": []}])
    LC.ctp_file(str(d / "a.ctp.gz"), k, a, **ka)
    LC.ctp_file(str(d / "b.ctp.gz"), k, b, **kb)
    ha, hb = json.loads(LC.header(k, **ka)), json.loads(LC.header(k, **kb))
    hb["paths"]["contig_hists"].append({"lengths": [31, 40], "counts": [1, 2]})  # (links_cases.header gives one histogram whatever ncols is)
    with gzip.open(str(d / "b.ctp.gz"), "wb") as f:
        f.write(json.dumps(hb, indent=2).encode() + b"\n\n# a comment block\n\n" + b)

    argv = ["pjoin", "-r", "-n", "1M", "-o", d / "ab.ctp.gz", d / "a.ctp.gz", d / "b.ctp.gz"]
    rc, out, err = cli(*argv)
    assert rc == 0 and out == b"", err
    adds = [(a, 1, [(0, 0)]), (b, 2, [(0, 1), (1, 2)])]
    body, info = want(k, 3, adds)[:2]
    hdr, got, raw = read_ctp(d / "ab.ctp.gz")
    differ(got, body, "a b")
    assert raw.endswith(body)
    same_header(hdr, PR.merged_header(k, 3, [(ha, adds[0][2]), (hb, adds[1][2])], info), argv)
    assert [c["sample"] for c in hdr["graph"]["colours"]] == ['s0 {"}', 's0 {"}', 's1 {"}'] and hdr["commands"][0]["prev"] == ["aabbccdd", "11112222"]
    assert [c["key"] for c in hdr["commands"][1:]] == ["aabbccdd", "11112222"]
    assert hdr["paths"]["contig_hists"] == [{"lengths": [31], "counts": [4]}, {"lengths": [31], "counts": [4]}, {"lengths": [31, 40], "counts": [1, 2]}]
    for line in ("-r, --noredundant changes nothing", "-n, --nkmers is not used", "Paths written to: %s" % (d / "ab.ctp.gz"),
                 "  %d paths, " % info["num_paths"], " path-bytes, %d kmers" % info["num_kmers_with_paths"]):
        assert line.replace(",", "") in err.replace(",", ""), (line, err)

    # both files into colour 0 (b's colour 0 alone), -c 2 leaves colour 1 to nobody; pieces of a few hundred bytes
    argv = ["pjoin", "-q", "-c", "2", "-o", d / "one.ctp.gz", "0:" + str(d / "a.ctp.gz"), "0:" + str(d / "b.ctp.gz") + ":0"]
    rc, out, err = cli(*argv, env={"MCX_LINKS_PIECE": "300"})
    assert rc == 0 and out == b"" and err == "", err
    adds = [(a, 1, [(0, 0)]), (b, 2, [(0, 0)])]
    hdr, got, _ = read_ctp(d / "one.ctp.gz")
    differ(got, want(k, 2, adds)[0], "0:a 0:b:0")
    rc, _, err = cli(*argv)
    assert rc == 1 and "File already exists" in err
    assert hdr["graph"]["colours"][1]["sample"] == "undefined" and hdr["paths"]["contig_hists"][1] == {"lengths": [], "counts": []}
    assert hdr["paths"]["contig_hists"][0] == {"lengths": [31], "counts": [8]}
    rc, _, err = cli("pjoin", "-o", d / "clash.ctp.gz", "0:" + str(d / "a.ctp.gz"), "0:" + str(d / "b.ctp.gz") + ":1")
    assert rc == 1 and "Graph/path sample names do not match [1->0]" in err

    # a swap: b's colours 1, 0 into 1, 2 beside a in 0 (one into colour would take both, as in the reference: `1:b.ctp:1,0`
    # loads both into colour 1, and their two sample names clash)
    argv = ["pjoin", "-q", "-m", "1G", "-o", d / "swap.ctp.gz", d / "a.ctp.gz", "1,2:" + str(d / "b.ctp.gz") + ":1,0"]
    rc, out, err = cli(*argv)
    assert rc == 0, err
    adds = [(a, 1, [(0, 0)]), (b, 2, [(1, 1), (0, 2)])]
    hdr, got, _ = read_ctp(d / "swap.ctp.gz")
    differ(got, want(k, 3, adds)[0], "a 1,2:b:1,0")
    assert [c["sample"] for c in hdr["graph"]["colours"]] == ['s0 {"}', 's1 {"}', 's0 {"}']
    rc, _, err = cli("pjoin", "-o", d / "clash2.ctp.gz", d / "a.ctp.gz", "1:" + str(d / "b.ctp.gz") + ":1,0")
    assert rc == 1 and "Graph/path sample names do not match [1->1]" in err

    # the totals of the header against what is seen; a k-mer line whose <n> is off
    LC.ctp_file(str(d / "off.ctp.gz"), k, a, totals=(ta["kmer_lines"] + 1, ta["link_lines"], 0))
    rc, _, err = cli("pjoin", "-o", d / "no.ctp.gz", d / "off.ctp.gz")
    assert rc == 1 and "[LoadPathError] header number of kmers don't match seen (exp %d vs %d)" % (ta["kmer_lines"] + 1, ta["kmer_lines"]) in err
    LC.ctp_file(str(d / "off2.ctp.gz"), k, a, totals=(ta["kmer_lines"], ta["link_lines"] - 1, 0))
    rc, _, err = cli("pjoin", "-f", "-o", d / "no.ctp.gz", d / "off2.ctp.gz")
    assert rc == 1 and "[LoadPathError] header number of links don't match seen (exp %d vs %d)" % (ta["link_lines"] - 1, ta["link_lines"]) in err
    LC.ctp_file(str(d / "n.ctp.gz"), k, b"ACGTACGTA 5\nF 1 2 A\nCCGTACGTA 1\nF 1 2 A\n", totals=(2, 2, 2))
    rc, _, err = cli("pjoin", "-o", d / "n_out.ctp.gz", d / "n.ctp.gz")
    assert rc == 0 and err.count("Number of links mismatches") == 1, err
    assert read_ctp(d / "n_out.ctp.gz")[1] == b"ACGTACGTA 1\nF 1 2 A\nCCGTACGTA 1\nF 1 2 A\n"
    LC.ctp_file(str(d / "bad.ctp.gz"), k, a + b"F 1 1,2 A\n", **ka)
    rc, _, err = cli("pjoin", "-o", d / "bad_out.ctp.gz", d / "bad.ctp.gz")
    assert rc == 1 and "[LoadPathError] Bad line (refusal 14)" in err and "F 1 1,2 A" in err and not (d / "bad_out.ctp.gz").exists()


def test_the_command_from_thread_to_contigs(tmp_path):
    """build, thread two read files apart, pjoin them into one colour, contigs with the merged file: the links are those
    of both read files threaded at once, the contigs those the restatement of `contigs` gives for them"""
    import random
    import clean_restate as R
    import contigs_restate as G
    import thread_restate as T
    k, d = 31, tmp_path
    rng = random.Random(4131)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    reps = [rs(k + 20) for _ in range(3)]  # three repeats, each twice: the links lead through them
    gen = "".join(rs(300) + reps[i] for i in (0, 1, 0, 2, 1, 2)) + rs(300)
    reads = [gen[s:s + n] for s, n in ((rng.randrange(0, len(gen) - 400), rng.randrange(80, 400)) for _ in range(120))]
    halves = reads[:60], reads[60:]
    for name, rr in (("a", halves[0]), ("b", halves[1]), ("all", reads)):
        (d / (name + ".txt")).write_text("".join(s + "\n" for s in rr))
    rc, _, err = cli("build", "-q", "-k", k, "-s", "s", "-1", d / "all.txt", d / "g.ctx")
    assert rc == 0, err
    for name in ("a", "b"):
        rc, _, err = cli("thread", "-q", "--seq", d / (name + ".txt"), "-o", d / (name + ".ctp.gz"), d / "g.ctx")
        assert rc == 0, err
    argv = ["pjoin", "-q", "-g", d / "g.ctx", "-o", d / "u.ctp.gz", "0:" + str(d / "a.ctp.gz"), "0:" + str(d / "b.ctp.gz")]
    rc, _, err = cli(*argv)
    assert rc == 0, err
    graph = R.build([reads], k)
    store = T.Store(graph, k).thread(reads)
    hdr, got, _ = read_ctp(d / "u.ctp.gz")
    differ(got, store.text(seq=False), "pjoin of two threads")
    assert 1 < max(store.links.values()) < 255 and len(store.links) >= 8
    ha, hb = (LC.split_ctp(gzip.open(d / (n + ".ctp.gz")).read())[0] for n in ("a", "b"))
    same_header(hdr, PR.merged_header(k, 1, [(ha, [(0, 0)]), (hb, [(0, 0)])], store.info()), argv)
    assert hdr["paths"]["contig_hists"] == [{"lengths": [x for x, _ in store.contig_hist()], "counts": [y for _, y in store.contig_hist()]}]
    rc, _, err = cli("contigs", "-q", "-o", d / "u.fa", "-p", d / "u.ctp.gz", d / "g.ctx")
    assert rc == 0, err
    links = [(key, o, b, n) for (key, o, b), n in store.links.items()]
    conf = G.conf_table(dict(store.contig_hist()), len(graph))
    _, seq, st = G.assemble(graph, k, links, conf, 0, 0, 0)
    fa = [ln for ln in (d / "u.fa").read_text().split("\n") if ln and ln[0] != ">"]
    assert fa == seq.decode().split("\n")[:-1] and len(fa) == st["contigs"] > 0
    # a graph of another k-mer size is refused before a device is opened
    rc, _, err = cli("build", "-q", "-k", 9, "-s", "s", "-1", d / "all.txt", d / "g9.ctx")
    assert rc == 0, err
    rc, _, err = cli("pjoin", "-g", d / "g9.ctx", "-o", d / "v.ctp.gz", d / "a.ctp.gz")
    assert rc == 1 and "Kmer-size doesn't match between files [9 vs 31]" in err
