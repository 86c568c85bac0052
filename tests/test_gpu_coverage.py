"""`coverage` on the MI355X (Graph.coverage*, csrc/mcx_coverage.h) against the CPU restatement in coverage_restate.py:
the arrays, the text, line_off and the stats, all by exact equality.  The cases are built on the CPU (the functions
named case_*), where each first asserts on the restatement alone what it is there to reach; the shapes are the smallest
that reach every branch: k = 9, 31, 63, 95, 127 (keys of one to four words), one and three colours, batches of a few
tiles of 4096 positions, tables of 2^16 slots."""
import functools
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import coverage_restate as V  # noqa: E402
import reads_restate as S  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (9, 31, 63, 95, 127)
TILE, WAVE, LANE = 4096, 1024, 16
LONG_STARTS = 4096  # kRtLongStarts of mcx_reads.h: a line of more values is measured by a whole wave
MAXC = 2**32 - 1
WIDTHS = (5, 42, 100, 1000, 10**4, 10**5, 10**6, 10**7, 10**8, 10**9, MAXC)  # "%2u" in 2, 2, 3 .. 10, 10 characters
VALUES = (9, 10, 99, 100, MAXC)


def rseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def key_of(k, s):
    return S.read_kmers(k, s)[0]


def junk(rng, graph, k, n):
    """a random sequence of n bases with no k-mer in the graph"""
    for _ in range(10000):
        s = rseq(rng, n)
        if not any(x in graph for x in S.read_kmers(k, s)):
            return s
    raise AssertionError("no junk found")


def rev_bits_swap(e):  # what the line the reference commented out would give
    return V.rev_nibble(e >> 4) | (V.rev_nibble(e & 15) << 4)


def load(graph, k, ncols, cap=1 << 16, twice=None):
    """the graph in a table; the keys in `twice` are loaded a second time with the coverage they had in `twice`"""
    g = mcx.Graph(k, ncols, cap)
    filt = [(c, c) for c in range(ncols)]
    first = dict(graph)
    twice = twice or {}
    for key, (cv, ed) in twice.items():
        first[key] = (cv, ed)
    g.add_records(R.pack(first, k, ncols), ncols, filt)
    if twice:
        g.add_records(R.pack(dict(twice), k, ncols), ncols, filt)
    g.sync()
    assert g.nkmers == len(graph)
    return g


def arrays(reads):
    seqs = [s.encode() for s in reads]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) or b"\n", dtype=np.uint8), offs


class Expect:
    """what the restatement says of a batch, computed once"""

    def __init__(self, graph, k, ncols, reads):
        self.ncols, self.reads = ncols, reads
        per = [V.values(graph, k, ncols, s) for s in reads]
        self.covg = np.array([sum((p[0][c] for p in per), []) for c in range(ncols)], dtype=np.uint64).astype(np.uint32).reshape(ncols, -1)
        self.edges = np.array([sum((p[1][c] for p in per), []) for c in range(ncols)], dtype=np.uint8).reshape(ncols, -1)
        nk, nf = V.counts(graph, k, reads)
        self.stats = {"num_reads": len(reads), "num_kmers": nk, "num_kmers_found": nf}
        self.lines = {}
        for e in (False, True):
            for d in (False, True):
                self.lines[e, d] = [ln for s, p in zip(reads, per) for ln in self._lines(k, s, p, e, d)]

    def _lines(self, k, seq, per, e, d):
        n, out = V.klen(k, seq), []
        for c in range(self.ncols):
            if e:
                out.append(V.edges_line(per[1][c][:n]))
            if d:
                out.append(V.degree_line(per[1][c][:n]))
            out.append(V.covg_line(per[0][c][:n]))
        return out


def check_arrays(g, exp, what=""):
    cv, ed, st = g.coverage(*arrays(exp.reads), edges=True)
    print("coverage %s: %s" % (what, st.as_dict()))
    assert cv.dtype == np.uint32 and ed.dtype == np.uint8
    assert np.array_equal(cv, exp.covg), (what, np.argwhere(cv != exp.covg)[:5])
    assert np.array_equal(ed, exp.edges), (what, np.argwhere(ed != exp.edges)[:5])
    assert st.as_dict() == exp.stats
    return cv, ed


def check_text(g, exp, what="", combos=((False, False), (True, False), (False, True), (True, True))):
    out = {}
    for e, d in combos:
        text, loff, st = g.coverage_text(*arrays(exp.reads), edges=e, degrees=d)
        want = exp.lines[e, d]
        off = np.zeros(len(want) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in want])
        assert text == "".join(want).encode(), (what, e, d)
        assert loff.dtype == np.uint64 and np.array_equal(loff, off), (what, e, d)
        assert st.as_dict() == exp.stats
        out[e, d] = text
    return out


# ---- cases (CPU only) ---------------------------------------------------------------------------------------------
def random_values(rng, ncols):
    cv = tuple(rng.choice(VALUES + (rng.randrange(1, 1000), rng.randrange(1, MAXC))) for _ in range(ncols))
    return cv, [rng.randrange(1, 256) for _ in range(ncols)]


@functools.lru_cache(maxsize=None)
def case_classes(k, ncols):
    """(graph, twice, reads, names): every class of read and of value"""
    rng = random.Random(7100 + 10 * k + ncols)
    gen = rseq(rng, 900 + k)
    graph = {key: random_values(rng, ncols) for key in S.keys_of([gen], k)}
    pos = {}  # key -> a position of the genome that holds it
    for p, key, o in V.oriented_kmers(k, gen):
        pos.setdefault(key, (p, o))
    assert len(pos) > 850  # (k = 9: a few k-mers repeat)
    # found forwards and found only as the reverse complement, with edge bytes that tell the three readings apart
    fw = next(key for key, (p, o) in pos.items() if o == 0 and p > 50)
    rv = next(key for key, (p, o) in pos.items() if o == 0 and p > 200 and key != fw)
    graph[fw] = ((7,) * ncols, [0x12] + [0x80] * (ncols - 1))
    graph[rv] = ((8,) * ncols, [0x12] + [0x80] * (ncols - 1))
    r_fw = gen[pos[fw][0]:pos[fw][0] + k]
    r_rv = rc(gen[pos[rv][0]:pos[rv][0] + k])
    assert V.oriented_kmers(k, r_fw) == [(0, fw, 0)] and V.oriented_kmers(k, r_rv) == [(0, rv, 1)]
    _, e_fw = V.values(graph, k, ncols, r_fw)
    _, e_rv = V.values(graph, k, ncols, r_rv)
    assert e_fw[0][0] == 0x12 and e_rv[0][0] == 0x21 != rev_bits_swap(0x12) and 0x21 != 0x12
    if ncols > 1:
        assert e_rv[1][0] == 0x08 != rev_bits_swap(0x80) and e_fw[1][0] == 0x80
    # every width of "%2u" in one line, and the listed values, on consecutive k-mers of the genome
    at = 300
    run = [key for _, key, _ in V.oriented_kmers(k, gen[at:at + k - 1 + len(WIDTHS) + 6])]
    assert len(set(run)) == len(run) and fw not in run and rv not in run
    vals = WIDTHS + (0, 9, 10, 99, 100, MAXC)
    for key, v in zip(run, vals):
        cv = tuple((v,) + tuple(vals[(vals.index(v) + c) % len(vals)] for c in range(1, ncols)))
        graph[key] = (cv, [0x41 if x == 0 else 0x23 for x in cv] if v == 0 else [rng.randrange(1, 256) for _ in range(ncols)])
        if v == 0 and ncols == 1:
            del graph[key]  # (a record without coverage in any colour is not loaded, graphs_load.c:121-125: its 0 is an absent k-mer's)
    r_widths = gen[at:at + k - 1 + len(vals)]
    line = V.value_lines(graph, k, ncols, r_widths)[0]
    assert line == " 5 42 100 1000 10000 100000 1000000 10000000 100000000 1000000000 4294967295  0  9 10 99 100 4294967295\n"
    if ncols > 1:  # present with coverage 0 in colour 0 (and edges there), coverage in the other colours
        zero = run[len(WIDTHS)]
        assert graph[zero][0][0] == 0 and graph[zero][1][0] == 0x41 and graph[zero][0][1] > 0
        assert V.values(graph, k, ncols, r_widths)[1][0][len(WIDTHS)] in (0x41, 0x14)
    # a slot whose stored sum exceeds 2^32 - 1: the record is loaded twice with 0xFFFFFFFF
    sat = next(key for key, (p, o) in pos.items() if p > 600 and key not in (fw, rv))
    graph[sat] = ((MAXC,) * ncols, [0x11] * ncols)
    twice = {sat: graph[sat]}
    assert 2 * MAXC > MAXC and V.values(graph, k, ncols, gen[pos[sat][0]:pos[sat][0] + k])[0][0][0] == 4294967295
    names = {"fw": r_fw, "rv": r_rv, "widths": r_widths, "sat": gen[pos[sat][0] - 3:pos[sat][0] + k + 2]}
    names["absent"] = junk(rng, graph, k, k + 7)
    names["n"] = gen[100:100 + k + 4] + "N" + gen[100 + k + 5:100 + 2 * k + 9]
    names["short"], names["empty"], names["lower"] = gen[50:50 + k - 1], "", gen[700:700 + k + 11].lower()
    names["all_n"] = "N" * (k + 3)
    assert V.counts(graph, k, [names["absent"]]) == (8, 0) and V.counts(graph, k, [names["n"]]) == (10, 10)
    assert V.klen(k, names["short"]) == 0 and V.counts(graph, k, [names["lower"]]) == (12, 12)
    reads = list(names.values())
    for i in range(60):  # genome reads in both strands, some with N, and junk between them
        q = rng.randrange(0, len(gen) - k - 60)
        s = list(gen[q:q + rng.randrange(k, k + 60)])
        if i % 4 == 0:
            s = [c if rng.random() > 0.02 else "N" for c in s]
        s = "".join(s)
        reads.append(rc(s) if i % 2 else s)
        if i % 5 == 0:
            reads.append(rseq(rng, rng.randrange(1, k + 30)))
    return graph, twice, reads, names


@functools.lru_cache(maxsize=None)
def case_seams(k, ncols):
    """(graph, reads): three tiles and a bit of reads cut from one genome, in both strands, so that nearly every position
    holds values; asserts that found k-mers straddle a lane, a wave and a tile boundary of the unchunked stream, and
    holds one read of more than LONG_STARTS start positions among the short ones"""
    rng = random.Random(8200 + 10 * k + ncols)
    gen = rseq(rng, LONG_STARTS + 700 + k)
    graph = {key: random_values(rng, ncols) for key in S.keys_of([gen], k)}
    reads, pos = [], 0
    long_at = None
    while pos < 3 * TILE + 500:
        if long_at is None and pos > 2000:
            s = gen[100:100 + LONG_STARTS + 300 + k]
            long_at = len(reads)
        else:
            q = rng.randrange(0, len(gen) - k - 70)
            s = gen[q:q + rng.randrange(k, k + 70)]
            if len(reads) % 7 == 3:
                s = s[:len(s) // 2] + "N" + s[len(s) // 2 + 1:]
            if len(reads) % 2:
                s = rc(s)
        reads.append(s)
        pos += len(s) + 1
    assert V.klen(k, reads[long_at]) > LONG_STARTS
    # stream position of every found k-mer: read r starts at offs[r] + r (one separator behind every read)
    starts, at = [], 0
    for s in reads:
        starts += [at + p for p, key, _ in V.oriented_kmers(k, s) if key in graph]
        at += len(s) + 1
    for unit in (LANE, WAVE, TILE):
        assert any(p // unit != (p + k - 1) // unit and (p + k - 1) // TILE < 3 for p in starts), unit
    assert any(p % TILE == TILE - 1 for p in starts) or any(p % LANE == LANE - 1 for p in starts)
    return graph, reads


# ---- on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", (1, 3))
@pytest.mark.parametrize("k", KS)
def test_classes_and_values(k, ncols):
    graph, twice, reads, names = case_classes(k, ncols)
    exp = Expect(graph, k, ncols, reads)
    g = load(graph, k, ncols, twice=twice)
    cv, ed = check_arrays(g, exp, "classes k=%d c=%d" % (k, ncols))
    idx = list(names).index
    offs = arrays(reads)[1]
    assert ed[0, int(offs[idx("rv")])] == 0x21 and ed[0, int(offs[idx("fw")])] == 0x12
    assert cv[0, int(offs[idx("sat")]) + 3] == 4294967295
    text = check_text(g, exp, "classes")
    assert b" 5 42 100 1000 10000 100000 1000000 10000000 100000000 1000000000 4294967295  0  9 10 99 100 4294967295\n" in text[False, False]
    # edges=None: no edges array, the same coverage
    cv2, none, st = g.coverage(*arrays(reads), edges=False)
    assert none is None and np.array_equal(cv2, exp.covg) and st.as_dict() == exp.stats
    # the k-mer counts are those of `reads`
    hit, ts = g.reads_touch(*arrays(reads))
    assert (ts.num_kmers, ts.num_kmers_found) == (exp.stats["num_kmers"], exp.stats["num_kmers_found"])
    # no reads
    cv0, ed0, st0 = g.coverage(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), edges=True)
    assert cv0.shape == (ncols, 0) and st0.as_dict() == {"num_reads": 0, "num_kmers": 0, "num_kmers_found": 0}
    t0, l0, _ = g.coverage_text(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), edges=True, degrees=True)
    assert t0 == b"" and l0.tolist() == [0]
    # the stats are added to the structure that is passed in
    st = mcx.graph.CoverageStats()
    g.coverage(*arrays(reads), stats=st)
    g.coverage_text(*arrays(reads), stats=st)
    assert st.as_dict() == {n: 2 * v for n, v in exp.stats.items()}
    g.close()


@pytest.mark.parametrize("ncols", (1, 3))
@pytest.mark.parametrize("k", KS)
def test_seams_grid_chunks_and_long_read(k, ncols):
    graph, reads = case_seams(k, ncols)
    exp = Expect(graph, k, ncols, reads)
    g = load(graph, k, ncols)
    check_arrays(g, exp, "default grid")
    whole = check_text(g, exp, "default grid", combos=((True, True),))
    g.configure("grid", 1)
    check_arrays(g, exp, "grid 1")
    assert check_text(g, exp, "grid 1", combos=((True, True),)) == whole
    g.configure("grid", 0)
    # chunks of 256 and 1024 stream bytes: seams between reads, and the long read in pieces that overlap by k - 1
    assert max(len(s) for s in reads) > 1024 and sum(len(s) <= 255 for s in reads) > 10
    for chunk in (256, 1024):
        g.configure("reads_chunk", chunk)
        check_arrays(g, exp, "chunks of %d" % chunk)
        assert check_text(g, exp, "chunks of %d" % chunk, combos=((True, True),)) == whole
    g.close()


@pytest.mark.parametrize("k", (31, 127))
def test_stream_entry_against_host_entry(k):
    import torch
    ncols = 3
    graph, reads = case_seams(k, ncols)
    exp = Expect(graph, k, ncols, reads)
    g = load(graph, k, ncols)
    text = ("\n".join(reads) + "\n").encode()
    pitch = (len(text) + 63) // 64 * 64
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d_cv = torch.full((ncols, pitch), 7, dtype=torch.int32).cuda()
    d_ed = torch.full((ncols, pitch), 7, dtype=torch.uint8).cuda()
    g.coverage_stream_dev(d_text, len(text), d_cv, d_ed, pitch)
    g.sync()
    cv = d_cv.cpu().numpy().view(np.uint32)
    ed = d_ed.cpu().numpy()
    # stream position of base p of read r is offs[r] + r + p: drop the separators
    keep = np.ones(len(text), dtype=bool)
    keep[np.cumsum([len(s) + 1 for s in reads]) - 1] = False
    assert np.array_equal(cv[:, :len(text)][:, keep], exp.covg) and np.array_equal(ed[:, :len(text)][:, keep], exp.edges)
    assert not cv[:, :len(text)][:, ~keep].any() and not ed[:, :len(text)][:, ~keep].any()
    # without edges the edges array is not touched
    d_cv.fill_(9)
    g.coverage_stream_dev(d_text, len(text), d_cv, None, pitch)
    g.sync()
    assert np.array_equal(d_cv.cpu().numpy().view(np.uint32)[:, :len(text)][:, keep], exp.covg)
    with pytest.raises(mcx.graph.McxError, match="multiple of 64"):
        g.coverage_stream_dev(d_text, len(text), d_cv, d_ed, pitch - 1)
    g.close()


def test_table_filled_to_ninety_percent_and_pending_inserts():
    k, ncols = 31, 3
    graph, twice, reads, _ = case_classes(k, ncols)
    exp = Expect(graph, k, ncols, reads)
    g = load(graph, k, ncols, twice=twice)
    slots = g.capacity()[0]
    rng = random.Random(99)
    extra = {}
    while len(extra) < int(0.92 * slots) - len(graph):
        key = S.canon(rng.getrandbits(2 * k), k)
        if key not in graph:
            extra[key] = ((1, 2, 3), [1, 2, 3])
    g.add_records(R.pack(extra, k, ncols), ncols, [(c, c) for c in range(ncols)])
    g.sync()
    assert g.nkmers == len(graph) + len(extra) >= 0.9 * slots
    full = dict(graph)
    full.update(extra)
    assert Expect(full, k, ncols, reads[:20]).stats == Expect(graph, k, ncols, reads[:20]).stats
    check_arrays(g, exp, "table at %.0f %%" % (100.0 * g.nkmers / slots))
    check_text(g, exp, "full table", combos=((True, True),))
    g.close()
    # pending add_reads with no sync in between: the lookups see them
    g = mcx.Graph(k, 1, 1 << 16)
    rng = random.Random(5)
    gen = rseq(rng, 400)
    g.add_reads(0, *arrays([gen, gen[100:300]]))
    cv, ed, st = g.coverage(*arrays([gen, rc(gen[50:150])]), edges=True)
    built = R.build([[gen, gen[100:300]]], k)
    e2 = Expect(built, k, 1, [gen, rc(gen[50:150])])
    assert cv[0].max() == 2 and np.array_equal(cv, e2.covg) and np.array_equal(ed, e2.edges) and st.as_dict() == e2.stats
    g.close()


def test_refusals():
    """a handle in intersect mode, a graph split over devices, unknown flags.  (No entry can be handed degrees without
    edges: the text entry gathers the edges whenever a flag is set, which `-E` without `-e` needs; that degrees alone
    print the real degrees is what check_text's (False, True) case compares.)"""
    k = 31
    graph, twice, reads, _ = case_classes(k, 1)
    recs2 = R.pack({key: ((1, 1), [0, 0]) for key in graph}, k, 2)
    g = mcx.Graph(k, 2, 1 << 16)
    g.add_records(recs2, 2, [(0, 0), (1, 1)])
    g.configure("intersect", 1)
    before = g.checksum()
    for call in (lambda: g.coverage(*arrays(reads)), lambda: g.coverage_text(*arrays(reads))):
        with pytest.raises(mcx.graph.McxError, match="coverage does not take a graph in intersect mode") as e:
            call()
        assert e.value.code == mcx.graph.MCX_ERR_ARG and g.checksum() == before
    g.close()
    g = mcx.Graph(k, 1, 1 << 16, devices=[0, 0])
    g.add_records(R.pack(graph, k, 1), 1, [(0, 0)])
    with pytest.raises(mcx.graph.McxError, match="coverage needs the whole table on one device, not a graph split over devices") as e:
        g.coverage(*arrays(reads))
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
    g = mcx.Graph(k, 1, 1 << 16, nparts=2, part=0)
    with pytest.raises(mcx.graph.McxError, match="split over devices"):
        g.coverage_text(*arrays(reads))
    g.close()
    g = load(graph, k, 1, twice=twice)
    bases, offs = arrays(reads)
    with pytest.raises(mcx.graph.McxError, match="unknown flags") as e:
        mcx.graph._check(g.L.mcx_graph_coverage_text(g.h, mcx.graph._ptr(bases), mcx.graph._ptr(offs), len(reads), 4,
                                                     mcx.graph.SINK_FN(lambda *_: 0), None, None, None))
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
