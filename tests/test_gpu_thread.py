"""`thread` on the MI355X (Graph.thread, Graph.links_*, csrc/mcx_thread.h) against the CPU restatement in
thread_restate.py: the text, the totals, the contig histogram and every count of mcx_thread_stats, by exact equality.
The golden graph of the reference's unit test (k = 11) and the random case of thread_cases.py (k = 11, 31, 33, 63, 65, 95,
97, 127: keys of one to four words), one-way and two-way, in tables of two sizes, with "grid" = 1 and with "reads_chunk" = 256,
which cuts the 600-base reads into pieces with an error over a seam; the reads in one call and in three, the reads
aimed at a structure in one call, in three and one read per call; links_reset; a count that stays at 255; links cut to
three junctions; the refusals."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import thread_cases as TC  # noqa: E402
import thread_restate as T  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thread.json")))["path_tests"]


def load(graph, k, ncols=1, cap=1 << 16):
    g = mcx.Graph(k, ncols, cap)
    g.add_records(R.pack(graph, k, ncols), ncols, [(c, c) for c in range(ncols)])
    g.sync()
    assert g.nkmers == len(graph)
    return g


def arrays(reads):
    seqs = [s.encode() for s in reads]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) or b"\n", dtype=np.uint8), offs


def thread(g, reads, stats=None, **kw):
    bases, offs = arrays(reads)
    return g.thread(bases, offs, stats=stats, **kw)


def same(g, want, what, stats=None):
    """the links the handle keeps are those of the restatement `want`"""
    if stats is not None:
        print("thread %s: %s" % (what, stats.as_dict()))
        assert stats.as_dict() == want.stats, what
    assert g.links_info() == want.info(), what
    assert g.links_contig_hist() == want.contig_hist(), what
    for seq in (True, False):
        got, text = g.links_text(seq=seq), want.text(seq=seq)
        if got != text:
            a, b = got.splitlines(), text.splitlines()
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            raise AssertionError((what, seq, i, a[i:i + 2], b[i:i + 2], len(a), len(b)))
    return g.links_text()


def test_golden_graph():
    k = GOLDEN["k"]
    graph = R.build([GOLDEN["graph_seqs"]], k)
    g = load(graph, k)
    want = T.Store(graph, k)
    assert g.links_info() == want.info() and g.links_text() == b"" and g.links_contig_hist() == []
    st = mcx.graph.ThreadStats()
    for c in GOLDEN["calls"]:
        thread(g, [c["read"]], stats=st)
        want.thread([c["read"]])
        info = g.links_info()
        assert (info["num_paths"], info["num_kmers_with_paths"]) == (c["links_total"], c["kmers_total"])
        same(g, want, "golden, a call per read", st)
    # one read 300 times: its counts stay at 255
    thread(g, [GOLDEN["calls"][0]["read"]] * 300, stats=st)
    want.thread([GOLDEN["calls"][0]["read"]] * 300)
    text = same(g, want, "a count pinned at 255", st)
    assert b" 255 " in text and max(want.links.values()) == 255
    # reset, then again, two-way
    g.links_reset()
    want.reset()
    same(g, want, "after links_reset")
    reads = [c["read"] for c in GOLDEN["calls"]]
    same(g, want.thread(reads, two_way=True), "golden two-way", thread(g, reads, two_way=True))
    g.close()


@pytest.mark.parametrize("k", TC.KS)
def test_random_case(k):
    TC.check_reach(k)
    graph, reads, aimed = TC.case(k)
    g = load(graph, k)
    whole = {}
    for two_way in (False, True):
        g.links_reset()
        st = thread(g, reads, two_way=two_way)
        whole[two_way] = same(g, TC.expected(k, two_way), "k=%d two_way=%d" % (k, two_way), st)
    want = TC.expected(k)
    # in three calls (and one of no reads): the same bytes
    g.links_reset()
    st = mcx.graph.ThreadStats()
    n = len(reads)
    for a, b in ((0, n // 3), (n // 3, n // 3), (n // 3, n - 7), (n - 7, n)):
        thread(g, reads[a:b], stats=st)
    assert same(g, want, "in calls", st) == whole[False]
    # the reads aimed at a structure (they make most of the links, many of them several times): in one call, in three
    # and one read per call, where every call leaves a segment of its own to be merged
    sub = reads[min(a for a, _ in aimed.values()):]
    assert 50 <= len(sub) <= 90
    wsub = TC.store(k).thread(sub)
    assert wsub.info()["num_paths"] > 100 and max(wsub.links.values()) > 2
    ways = []
    for cuts in ((0, len(sub)), (0, 20, 21, len(sub)), tuple(range(len(sub) + 1))):
        g.links_reset()
        st = mcx.graph.ThreadStats()
        for a, b in zip(cuts, cuts[1:]):
            thread(g, sub[a:b], stats=st)
        ways.append(same(g, wsub, "the aimed reads in %d calls" % (len(cuts) - 1), st))
    assert ways[0] == ways[1] == ways[2]
    # the launches capped at one workgroup
    g.links_reset()
    g.configure("grid", 1)
    st = thread(g, reads)
    assert same(g, want, "grid 1", st) == whole[False]
    g.configure("grid", 0)
    # chunks of 256 stream bytes: the 600-base reads go in pieces, and the error at base 250 of each lies over a seam
    lo, hi = aimed["long"]
    assert all(len(s) > 512 for s in reads[lo:hi]) and hi - lo == 3
    g.links_reset()
    g.configure("reads_chunk", 256)
    st = thread(g, reads, two_way=True)
    assert same(g, TC.expected(k, True), "chunks of 256", st) == whole[True]
    g.links_reset()
    st = thread(g, reads[lo:hi])
    same(g, TC.store(k).thread(reads[lo:hi]), "long reads alone in chunks of 256", st)
    g.configure("reads_chunk", 0)
    # links cut to three junctions merge behind the cut
    g.links_reset()
    st = thread(g, reads, max_juncs=3)
    cut = same(g, TC.expected(k, False, 3), "max_juncs 3", st)
    assert cut != whole[False]
    # other bounds
    g.links_reset()
    st = thread(g, reads, gap_variance=0.3, gap_wiggle=2.0)
    same(g, TC.store(k).thread(reads, D=0.3, d=2.0), "D=0.3 d=2", st)  # (other stats than the defaults' from k = 31 on)
    g.close()
    # a table of another size
    g = load(graph, k, cap=1 << 18)
    st = thread(g, reads)
    assert same(g, want, "a larger table", st) == whole[False]
    g.close()


def test_refusals():
    k = GOLDEN["k"]
    graph = R.build([GOLDEN["graph_seqs"]], k)
    reads = [c["read"] for c in GOLDEN["calls"]]
    g = load(graph, k)
    assert thread(g, []).as_dict() == T.new_stats()
    for kw in ({"gap_variance": -0.1}, {"gap_wiggle": float("nan")}, {"gap_variance": float("inf")}, {"gap_wiggle": -1.0}, {"max_juncs": 32768}):
        with pytest.raises(mcx.graph.McxError) as e:
            thread(g, reads, **kw)
        assert e.value.code == mcx.graph.MCX_ERR_ARG, kw
    bases, offs = arrays(reads)
    prm = mcx.graph.ThreadParams(2, 0.1, 5.0, 0)  # unknown flags
    assert g.L.mcx_graph_thread(g.h, bases.ctypes.data, offs.ctypes.data, len(reads), prm, None) == mcx.graph.MCX_ERR_ARG
    assert g.L.mcx_graph_links_text(g.h, 2, mcx.graph.SINK_FN(lambda *_: 0), None) == mcx.graph.MCX_ERR_ARG
    assert g.links_info()["num_paths"] == 0
    g.close()
    # two colours
    two = R.build([GOLDEN["graph_seqs"], GOLDEN["graph_seqs"][:1]], k)
    g = load(two, k, 2)
    with pytest.raises(mcx.graph.McxError) as e:
        thread(g, reads)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    # intersect mode
    g.configure("intersect", 1)
    with pytest.raises(mcx.graph.McxError) as e:
        thread(g, reads)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
    # a graph split over devices (two shards on the one device there is)
    g = mcx.Graph(k, 1, 1 << 16, devices=[0, 0])
    with pytest.raises(mcx.graph.McxError) as e:
        thread(g, reads)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
