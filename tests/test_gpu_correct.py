"""`correct` on the MI355X (Graph.correct, csrc/mcx_correct.h) against the CPU restatement in correct_restate.py: the
bytes, out_off and every count of mcx_correct_stats, by exact equality.  The golden graphs (k = 9 and k = 11) and the
random case of correct_cases.py (k = 11, 31, 33, 63, 65, 95, 97, 127: keys of one to four words; one colour, and three with the
sample in colour 1), with and without qualities, one-way and two-way, in tables of two sizes, with "grid" = 1 and with
"reads_chunk" = 256, which cuts the 600-base reads into pieces with an error over a seam.  The case first asserts on
the restatement alone that it reaches every rule at least three times (test_correct_restate.py asserts the same on the
CPU)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import correct_cases as CC  # noqa: E402
import correct_restate as X  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "correct.json")))


def load(graph, k, ncols, cap=1 << 16):
    g = mcx.Graph(k, ncols, cap)
    g.add_records(R.pack(graph, k, ncols), ncols, [(c, c) for c in range(ncols)])
    g.sync()
    assert g.nkmers == len(graph)
    return g


def arrays(reads, quals=None):
    seqs = [s.encode() for s in reads]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    bases = np.frombuffer(b"".join(seqs) or b"\n", dtype=np.uint8)
    if quals is None:
        return bases, offs, None
    return bases, offs, np.frombuffer("".join(quals).encode() or b"\n", dtype=np.uint8)


def check(g, reads, quals, want, what, **kw):
    bases, offs, q = arrays(reads, quals)
    out, off, st = g.correct(bases, offs, quals=q, **kw)
    text, woff, wstats = want
    print("correct %s: %s" % (what, st.as_dict()))
    assert off.dtype == np.uint64 and off.tolist() == list(woff), (what, next(i for i, (a, b) in enumerate(zip(off.tolist(), woff)) if a != b))
    if out != text:
        r = next(i for i in range(len(reads)) if out[woff[i]:woff[i + 1]] != text[woff[i]:woff[i + 1]])
        raise AssertionError((what, r, reads[r], out[woff[r]:woff[r + 1]], text[woff[r]:woff[r + 1]]))
    assert st.as_dict() == wstats, what
    return out


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_graphs(name):
    sec = GOLDEN[name]
    k = sec["k"]
    graph = R.build([sec["graph_seqs"]], k)
    reads = [c["read"] for c in sec["cases"]]
    g = load(graph, k, 1)
    for two_way in (False, True):
        out = check(g, reads, None, X.batch(graph, k, reads, two_way=two_way), "%s two_way=%d" % (name, two_way), two_way=two_way)
        assert out.decode() == "".join(c["corrected"] for c in sec["cases"])
    if any(c.get("qual") for c in sec["cases"]):
        quals = [c["qual"] or "I" * len(c["read"]) for c in sec["cases"]]
        check(g, reads, quals, X.batch(graph, k, reads, quals), name + " with qualities")
        check(g, reads, quals, X.batch(graph, k, reads, quals, fq_zero="#"), name + " fq_zero", fq_zero="#")
    g.close()


@pytest.mark.parametrize("ncols", (1, 3))
@pytest.mark.parametrize("k", CC.KS)
def test_random_case(k, ncols):
    CC.check_reach(k, ncols)
    graph, colour, reads, quals, aimed = CC.case(k, ncols)
    g = load(graph, k, ncols)
    whole = {}
    for two_way in (False, True):
        for wq in (False, True):
            whole[two_way, wq] = check(g, reads, quals if wq else None, CC.records(k, ncols, wq, two_way),
                                       "k=%d c=%d two_way=%d quals=%d" % (k, ncols, two_way, wq), colour=colour, two_way=two_way)
    assert whole[False, False] != whole[True, False]
    # the launches capped at one workgroup
    g.configure("grid", 1)
    check(g, reads, quals, CC.records(k, ncols, True), "grid 1", colour=colour)
    g.configure("grid", 0)
    # chunks of 256 stream bytes: the 600-base reads go in pieces, and the error at base 250 of each lies over a seam
    lo, hi = aimed["long"]
    assert all(len(s) > 512 for s in reads[lo:hi]) and hi - lo == 3
    g.configure("reads_chunk", 256)
    check(g, reads, quals, CC.records(k, ncols, True, True), "chunks of 256", colour=colour, two_way=True)
    check(g, reads[lo:hi], None, X.batch(graph, k, reads[lo:hi], colour=colour), "long reads alone in chunks of 256", colour=colour)
    g.configure("reads_chunk", 0)
    # other bounds: D and d, and another fq_zero
    nodes, stats, _ = CC.expected(k, ncols, False, 0.3, 2.0)
    want = CC.records(k, ncols, True, False, 0.3, 2.0, "#")
    assert want[0] != CC.records(k, ncols, True)[0]
    check(g, reads, quals, want, "D=0.3 d=2 fq_zero=#", colour=colour, gap_variance=0.3, gap_wiggle=2.0, fq_zero="#")
    # the stats are added to the structure that is passed in
    st = mcx.graph.CorrectStats()
    b, o, q = arrays(reads, quals)
    g.correct(b, o, colour=colour, stats=st)
    g.correct(b, o, quals=q, colour=colour, stats=st)
    assert st.as_dict() == {n: 2 * v for n, v in CC.records(k, ncols, False)[2].items()}
    g.close()
    # a table of another size
    g = load(graph, k, ncols, cap=1 << 18)
    check(g, reads, quals, CC.records(k, ncols, True), "a table of 2^18", colour=colour)
    g.close()


def test_colour_zero_of_three_and_stream_entry():
    import torch
    k, ncols = 31, 3
    graph, colour, reads, quals, aimed = CC.case(k, ncols)
    g = load(graph, k, ncols)
    want = X.batch(graph, k, reads, colour=0)
    assert want[0] != CC.records(k, ncols, False)[0]
    check(g, reads, None, want, "colour 0", colour=0)
    # the stream entry: the same walks, the records' lengths only
    text = ("\n".join(reads) + "\n").encode()
    so = np.zeros(len(reads) + 1, dtype=np.int64)
    so[1:] = np.cumsum([len(s) + 1 for s in reads])
    pitch = (len(text) + 63) // 64 * 64
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d_so = torch.from_numpy(so).cuda()
    d_node = torch.zeros(pitch, dtype=torch.int64).cuda()
    d_len = torch.zeros(len(reads), dtype=torch.int64).cuda()
    st = g.correct_stream_dev(d_text, len(text), d_so, len(reads), d_node, pitch, d_len, colour=colour)
    g.sync()
    text1, off1, stats1 = CC.records(k, ncols, False)
    assert d_len.cpu().numpy().tolist() == np.diff(off1).tolist()
    assert st.as_dict() == stats1
    with pytest.raises(mcx.graph.McxError, match="multiple of 64"):
        g.correct_stream_dev(d_text, len(text), d_so, len(reads), d_node, pitch - 1, d_len)
    g.close()


def test_refusals_and_no_reads():
    k = 31
    graph, colour, reads, quals, aimed = CC.case(k, 1)
    bases, offs, _ = arrays(reads[:20])
    g = load(graph, k, 1)
    out, off, st = g.correct(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert out == b"" and off.tolist() == [0] and not any(st.as_dict().values())
    before = g.checksum()
    for kw, msg in (({"colour": 1}, "colour 1 is not one of the graph's 1"), ({"gap_wiggle": -1.0}, "finite and not negative"),
                    ({"gap_variance": float("nan")}, "finite and not negative"), ({"gap_variance": float("inf")}, "finite and not negative")):
        with pytest.raises(mcx.graph.McxError, match=msg) as e:
            g.correct(bases, offs, **kw)
        assert e.value.code == mcx.graph.MCX_ERR_ARG
    prm = mcx.graph.CorrectParams(0, 2, 0.1, 5.0, b".")
    with pytest.raises(mcx.graph.McxError, match="unknown flags") as e:
        mcx.graph._check(g.L.mcx_graph_correct(g.h, mcx.graph._ptr(bases), None, mcx.graph._ptr(offs), 20, prm, mcx.graph.SINK_FN(lambda *_: 0),
                                               None, None, None))
    assert e.value.code == mcx.graph.MCX_ERR_ARG and g.checksum() == before
    g.close()
    g = mcx.Graph(k, 2, 1 << 16)
    g.add_records(R.pack({key: ((1, 1), [0, 0]) for key in graph}, k, 2), 2, [(0, 0), (1, 1)])
    g.configure("intersect", 1)
    with pytest.raises(mcx.graph.McxError, match="correct does not take a graph in intersect mode") as e:
        g.correct(bases, offs)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
    g = mcx.Graph(k, 1, 1 << 16, devices=[0, 0])
    g.add_records(R.pack(graph, k, 1), 1, [(0, 0)])
    with pytest.raises(mcx.graph.McxError, match="correct needs the whole table on one device, not a graph split over devices") as e:
        g.correct(bases, offs)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
