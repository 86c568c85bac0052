"""tests/join_restate.py pinned: hand-computed cases for the drop rule, saturation, gaps in the colours, the swap and
the rank-0 mask, KEEP_EMPTY; and the invariants the reference's tests/join/Makefile asserts, replayed on
golden/tiny_k31.ctx and graphs derived from it.  Every case first shows, on the restatement alone, that it reaches what
it is there to reach."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_restate as J  # noqa: E402
from oracle import ctxio  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G31 = os.path.join(ROOT, "tests", "golden", "tiny_k31.ctx")
U32 = 0xFFFFFFFF


def test_pack_parse_round_trip():
    for k in (9, 33, 65, 127):
        W = ctxio.words_for_k(k)
        recs = [(5, [1, 2], [3, 4]), ((1 << (2 * k)) - 1, [U32, 0], [0xFF, 0])]
        body = J.pack(recs, k, 2)
        assert len(body) == 2 * (8 * W + 10) and J.parse(body, k, 2) == recs
    # key words most significant first, little-endian inside a word
    assert J.pack([((7 << 64) | 9, [1], [2])], 33, 1) == bytes([7] + [0] * 7 + [9] + [0] * 7 + [1, 0, 0, 0, 2])


def test_drop_rule():
    # a two-colour file of which the filter selects colour 1 only
    f = J.pack([(10, [5, 0], [0x01, 0x02]),     # coverage only in the unselected colour: goes
                (11, [0, 0], [0x03, 0x03]),     # edges but no coverage: goes
                (12, [0, 7], [0x10, 0x21])], 9, 2)
    body, st, out = J.join_records(9, 1, [(f, 2, [(1, 0)])])
    assert out == {12: ([7], [0x21])}
    assert body == J.pack([(12, [7], [0x21])], 9, 1)
    assert (st["recs_read"], st["recs_kept"], st["kmers_written"]) == (3, 1, 1)
    # selecting both colours keeps the first record as well, and still not the second
    _, st2, out2 = J.join_records(9, 2, [(f, 2, [(0, 0), (1, 1)])])
    assert sorted(out2) == [10, 12] and out2[10] == ([5, 0], [0x01, 0x02]) and st2["recs_kept"] == 2


def test_saturation_within_and_across_files():
    a = J.pack([(3, [0xFFFFFFF0, 0x20], [1, 2]), (4, [0x80000000, 0], [4, 0])], 9, 2)
    b = J.pack([(4, [0x80000000], [8]), (5, [1], [0])], 9, 1)
    assert 0xFFFFFFF0 + 0x20 > U32 and 0x80000000 + 0x80000000 > U32  # both really overflow 32 bits
    _, _, out = J.join_records(9, 1, [(a, 2, [(0, 0), (1, 0)]), (b, 1, [(0, 0)])])
    assert out[3] == ([U32], [3])      # within one file's filter
    assert out[4] == ([U32], [12])     # across files
    assert out[5] == ([1], [0])
    # the same file twice into one colour is summed like any other
    _, _, out = J.join_records(9, 1, [(b, 1, [(0, 0)]), (b, 1, [(0, 0)])])
    assert out[4] == ([U32], [8]) and out[5] == ([2], [0])


def test_gaps_in_the_colours():
    a = J.pack([(1, [2], [0x11])], 9, 1)
    body, _, out = J.join_records(9, 5, [(a, 1, [(0, 1)]), (a, 1, [(0, 4)])])
    assert out[1] == ([0, 2, 0, 0, 2], [0, 0x11, 0, 0, 0x11])
    assert body == bytes([1] + [0] * 7) + np.array([0, 2, 0, 0, 2], dtype="<u4").tobytes() + bytes([0, 0x11, 0, 0, 0x11])


def _file(k, samples, recs):
    gi = []
    for s in samples:
        g = ctxio.GraphInfo()
        g.sample_name = s
        gi.append(g)
    return ctxio.header_bytes(k, gi) + J.pack(recs, k, len(samples))


def test_swap_and_rank0_mask():
    big = _file(9, ["big"], [(1, [1], [0xF0]), (2, [1], [0xFF]), (3, [1], [0xFF])])
    small = _file(9, ["small"], [(1, [1], [0x0F]), (2, [1], [0x3C])])
    inp = _file(9, ["in"], [(1, [4], [0xFF]), (2, [5], [0xFF]), (3, [6], [0xFF]), (4, [7], [0xFF])])
    files = {"big.ctx": big, "small.ctx": small, "in.ctx": inp}
    exp = J.pack([(1, [4], [0x0F]), (2, [5], [0x3C])], 9, 1)  # the mask is the smaller graph's, whichever comes first
    for order in (["big.ctx", "small.ctx"], ["small.ctx", "big.ctx"]):
        hdr, body, st, ncols = J.join_command(["in.ctx"], files, order)
        assert body == exp and ncols == 1
        assert st["kmers_intersection"] == 2 and st["recs_kept"] == 4 and st["kmers_written"] == 2
        h, _ = ctxio.read_header(hdr)
        c = h["ginfo"][0].cleaning
        assert c.is_graph_intersection == 1 and c.intersection_name == "small,big"
        assert h["ginfo"][0].sample_name == "in"
    # equal sizes: no swap, the first given is rank 0
    big2 = _file(9, ["big2"], [(1, [1], [0xF0]), (2, [1], [0xC3])])
    files["big2.ctx"] = big2
    _, body, _, _ = J.join_command(["in.ctx"], files, ["big2.ctx", "small.ctx"])
    assert body == J.pack([(1, [4], [0xF0]), (2, [5], [0xC3])], 9, 1)
    hdr, body, _, _ = J.join_command(["in.ctx"], files, ["small.ctx", "big2.ctx"])
    assert body == exp
    assert ctxio.read_header(hdr)[0]["ginfo"][0].cleaning.intersection_name == "small,big2"


def test_keep_empty():
    isec = J.pack([(1, [1], [0xFF]), (2, [1], [0xFF]), (9, [0], [0xFF])], 9, 1)  # key 9 has no coverage: not in the set
    inp = J.pack([(2, [3], [0x81]), (7, [3], [0x81])], 9, 1)
    _, st, out = J.join_records(9, 2, [(inp, 1, [(0, 1)])], [(isec, 1, [(0, 0)])], keep_empty=False)
    assert 1 not in out and out == {2: ([0, 3], [0, 0x81])}  # key 1: in the intersection, in no input
    assert (st["kmers_intersection"], st["kmers_written"], st["kmers_written_no_covg"]) == (2, 1, 0)
    assert (st["isec_recs_read"], st["isec_recs_kept"]) == (3, 2)
    body, st, out = J.join_records(9, 2, [(inp, 1, [(0, 1)])], [(isec, 1, [(0, 0)])], keep_empty=True)
    assert out == {1: ([0, 0], [0, 0]), 2: ([0, 3], [0, 0x81])}
    assert (st["kmers_written"], st["kmers_written_no_covg"]) == (2, 1)
    assert body == J.pack([(1, [0, 0], [0, 0]), (2, [0, 3], [0, 0x81])], 9, 2)
    # the command sets it with -i and (more than one input or --sort)
    f = {"i.ctx": _file(9, ["i"], J.parse(isec, 9, 1)), "a.ctx": _file(9, ["a"], J.parse(inp, 9, 1))}
    assert J.join_command(["a.ctx"], f, ["i.ctx"])[2]["kmers_written"] == 1
    assert J.join_command(["a.ctx"], f, ["i.ctx"], sort=True)[2]["kmers_written"] == 2
    assert J.join_command(["a.ctx", "a.ctx"], f, ["i.ctx"])[2]["kmers_written"] == 2
    assert J.join_command(["a.ctx", "a.ctx"], f)[2]["kmers_written"] == 2  # (no -i: nothing to keep)


# ---- the reference's tests/join/Makefile on golden/tiny_k31.ctx -------------------------------------------------------
def samples():
    """three one-colour graphs: tiny_k31's two colours, and a third derived from them (every third k-mer, coverage + 1)"""
    buf = open(G31, "rb").read()
    hdr, hs = ctxio.read_header(buf)
    recs = J.parse(buf[hs:], 31, 2)
    gi = hdr["ginfo"]
    third = ctxio.GraphInfo()
    third.sample_name = "carol"
    a = ctxio.header_bytes(31, [gi[0]]) + J.pack([(k, [c[0]], [e[0]]) for k, c, e in recs], 31, 1)
    b = ctxio.header_bytes(31, [gi[1]]) + J.pack([(k, [c[1]], [e[1]]) for k, c, e in recs[::2]], 31, 1)
    c = ctxio.header_bytes(31, [third]) + J.pack([(k, [c[0] + 1], [e[1] & 0x3C]) for k, c, e in recs[1::3]], 31, 1)
    return {"a.ctx": a, "b.ctx": b, "c.ctx": c}


def ctxio_body(buf):
    return buf[ctxio.read_header(buf)[1]:]


EIGHT = ["0:a.ctx", "1:b.ctx", "2:c.ctx", "3:a.ctx", "3:a.ctx", "4:b.ctx", "4:c.ctx", "5:c.ctx"]


def test_makefile_eight_argument_line():
    files = samples()
    hdr, body, st, ncols = J.join_command(EIGHT, files)
    assert ncols == 6
    recs = J.parse(body, 31, 6)
    assert recs
    src = {n: {k: (c[0], e[0]) for k, c, e in J.parse(ctxio_body(files[n]), 31, 1) if c[0]} for n in ("a.ctx", "b.ctx", "c.ctx")}
    assert 0 < len(src["a.ctx"]) < 3261  # some of the fixture's k-mers have no coverage in colour 0: they are dropped
    assert sorted(set().union(*src.values())) == [k for k, _, _ in recs]  # sorted, each key once
    assert any(c[1] and c[2] for _, c, _ in recs) and any(c[1] and not c[2] for _, c, _ in recs)  # col4 is a real sum
    for _, c, e in recs:
        assert c[3] == 2 * c[0] and c[4] == c[1] + c[2] and c[5] == c[2]
        assert e[3] == e[0] and e[4] == e[1] | e[2] and e[5] == e[2]
    h, _ = ctxio.read_header(hdr)
    assert [g.sample_name for g in h["ginfo"]] == ["alice", "bob", "carol", "alice,alice", "bob,carol", "carol"]
    assert st["recs_read"] == 3 * 3261 + 2 * 1631 + 3 * 1087
    assert st["recs_kept"] == 3 * len(src["a.ctx"]) + 2 * len(src["b.ctx"]) + 3 * len(src["c.ctx"])
    files["in.ctx"] = hdr + body

    # 0:in:1 0:in:0 0:in:3-3 flattens
    hdr2, body2, _, ncols2 = J.join_command(["0:in.ctx:1", "0:in.ctx:0", "0:in.ctx:3-3"], files)
    assert ncols2 == 1
    flat = J.parse(body2, 31, 1)
    assert [(k, [c[1] + c[0] + c[3]], [e[1] | e[0] | e[3]]) for k, c, e in recs if c[1] + c[0] + c[3]] == flat
    assert 0 < len(flat) < len(recs)  # the k-mers of carol alone have no coverage in colours 0, 1, 3
    assert ctxio.read_header(hdr2)[0]["ginfo"][0].sample_name == "bob,alice,alice,alice"

    # 1:in:0 0:in:1 4:in:3 leaves colours 2 and 3 empty with default header entries
    hdr3, body3, _, ncols3 = J.join_command(["1:in.ctx:0", "0:in.ctx:1", "4:in.ctx:3"], files)
    assert ncols3 == 5
    gaps = J.parse(body3, 31, 5)
    assert [(k, [c[1], c[0], 0, 0, c[3]], [e[1], e[0], 0, 0, e[3]]) for k, c, e in recs if c[1] + c[0] + c[3]] == gaps
    h3 = ctxio.read_header(hdr3)[0]["ginfo"]
    assert [g.sample_name for g in h3] == ["bob", "alice", "undefined", "undefined", "alice,alice"]
    assert h3[2].total_sequence == 0 and h3[2].mean_read_length == 0 and h3[2].cleaning.intersection_name == "undefined"
