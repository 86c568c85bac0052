"""`breakpoints` on the MI355X (Graph.breakpoints, csrc/mcx_breakpoints.h) against the CPU restatement in
breakpoints_restate.py, by exact equality: every record field, the text bytes and every stat (but `reruns`, which says how
often the "breakpoints_runs" knob was outgrown).  Every case of breakpoints_cases.py (k = 11, 31, 33: keys of one and two
words); the same, on the handle that holds the reference by then, with "breakpoints_batch" 1 and 2, "grid" 1,
"breakpoints_chunk" 1, 7 and 64 and "breakpoints_runs" 1; a random 2 kb genome per k whose two sample colours carry
substitutions, indels, an inversion and a translocation, at two table capacities; second calls with other limits on one
handle; the breakpoint1 fixture; the ABI symbol and the refusals.  At k = 63, 65, 95, 97 and 127 (keys of two, three and
four words): the wide cases without a knob, with "breakpoints_batch" 1 and with "breakpoints_chunk" 7, and the random
genome.  stop_bound is 0 everywhere."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breakpoints_cases as BC  # noqa: E402
import breakpoints_restate as B  # noqa: E402
import clean_restate as R  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu
REC_FIELDS = ("fork_orient", "succ_base", "num_cols", "path_kmers", "flank5p_kmers", "flank3p_kmers", "flank5p_runs", "flank3p_runs", "text_off",
              "text_len")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(graph, k, ncols, cap=1 << 14):
    g = mcx.Graph(k, ncols, cap)
    g.add_records(R.pack(graph, k, ncols), ncols, [(c, c) for c in range(ncols)])
    g.sync()
    assert g.nkmers == len(graph)
    return g


def want_of(recs, text, stats):
    st = dict(stats)
    st.pop("reruns")
    assert st["stop_bound"] == 0
    return [(r["fork_key"],) + tuple(r[f] for f in REC_FIELDS) for r in recs], text.encode(), st


def got_of(recs, text, st, k):
    W = (2 * k + 63) // 64
    out = []
    for r in recs:
        key = 0
        for i in range(W):
            key = (key << 64) | int(r["fork_key"][i])
        assert all(int(x) == 0 for x in r["fork_key"][W:])
        out.append((key,) + tuple(int(r[f]) for f in REC_FIELDS))
    d = st.as_dict()
    d.pop("reruns")
    assert d["stop_bound"] == 0
    return out, text, d


def device_run(g, k, ref, names, min_ref, max_ref, ref_edges=True, ref_loaded=False):
    st = mcx.graph.BreakpointsStats()
    recs, text = g.breakpoints(ref, names, min_ref, max_ref, ref_edges, ref_loaded, stats=st)
    return got_of(recs, text, st, k), st.reruns


def text_pieces(g, ref, names, min_ref, max_ref):
    """the sizes in which the text sink receives the text (the reference is loaded)"""
    pieces = []

    def sink(_ctx, _ptr, n):
        pieces.append(n)
        return 0
    bases = ctypes.create_string_buffer("".join(ref).encode())
    nbuf = ctypes.create_string_buffer("".join(names).encode())
    off = (ctypes.c_uint64 * (len(ref) + 1))(*[sum(len(s) for s in ref[:i]) for i in range(len(ref) + 1)])
    noff = (ctypes.c_uint64 * (len(ref) + 1))(*[sum(len(s) for s in names[:i]) for i in range(len(ref) + 1)])
    prm = mcx.graph.BreakpointsParams(min_ref, max_ref, mcx.graph.BREAKPOINTS_REF_LOADED)
    assert g.L.mcx_graph_breakpoints(g.h, bases, off, len(ref), nbuf, noff, ctypes.byref(prm), ctypes.cast(None, mcx.graph.SINK_FN), None,
                                     mcx.graph.SINK_FN(sink), None, None) == mcx.graph.MCX_OK
    return pieces


def check(got, want, what):
    if got != want:
        assert got[2] == want[2], (what, got[2], want[2])
        for a, b in zip(got[0], want[0]):
            assert a == b, (what, a, b)
        assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
        n = next((i for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b), min(len(got[1]), len(want[1])))
        raise AssertionError((what, "the text differs at byte %d" % n, got[1][max(0, n - 80):n + 80], want[1][max(0, n - 80):n + 80]))


def test_abi_symbol_and_wrapper():
    assert hasattr(mcx.lib(), "mcx_graph_breakpoints")
    assert callable(mcx.Graph.breakpoints) and set(B.STAT_NAMES) == set(mcx.graph.BreakpointsStats().as_dict())
    assert mcx.graph.BREAKPOINT_REC.itemsize == 80


KNOBS = ((("breakpoints_batch", 1),), (("breakpoints_batch", 2),), (("grid", 1),), (("breakpoints_chunk", 1),), (("breakpoints_chunk", 7),),
         (("breakpoints_chunk", 64),), (("breakpoints_runs", 1),))


WIDE_KNOBS = ((("breakpoints_batch", 1),), (("breakpoints_chunk", 7),))  # (beside the first call of every case, which sets no knob)


@pytest.mark.parametrize("k", BC.KS)
def test_cases(k):
    assert run_cases(k, BC.cases(), KNOBS) > 0


@pytest.mark.parametrize("k", BC.WIDE_KS)
def test_wide_cases(k):
    """the same structures at keys of two, three and four words with a full and a 2-bit top word, without a knob and under
    two: a text seam every 7 bytes falls inside k-mers of up to 127 bases"""
    assert run_cases(k, BC.wide_cases(), WIDE_KNOBS) == 0


def run_cases(k, cases, knobs):
    """every case of `cases` at k, without a knob and under every knob, against the restatement -> the reruns seen under the
    "breakpoints_runs" knob"""
    reruns_seen = 0
    for case in (c for c in cases if c["k"] == k):
        p = case["params"]
        ref, names = case["ref"], case["names"]
        recs, text, stats, _, with_ref = BC.run(case)
        want = want_of(recs, text, stats)
        g = load(case["graph"], k, case["ncols"])
        got, _ = device_run(g, k, ref, names, p["min_ref"], p["max_ref"], p["ref_edges"])
        print(case["name"], got[2])
        check(got, want, case["name"])
        assert g.nkmers == len(with_ref)
        # the knobs, on the handle that holds the reference now
        want = want_of(*B.call(with_ref, k, case["ncols"], ref, names, p["min_ref"], p["max_ref"], p["ref_edges"], ref_loaded=True)[:3])
        assert want[:2] == want_of(recs, text, stats)[:2]
        for kn in knobs:
            for key, v in kn:
                g.configure(key, v)
            got, reruns = device_run(g, k, ref, names, p["min_ref"], p["max_ref"], p["ref_edges"], ref_loaded=True)
            for key, _ in kn:
                g.configure(key, 0)
            check(got, want, (case["name"], kn))
            if kn[0][0] == "breakpoints_runs":
                reruns_seen += reruns
                if case["name"].startswith("repeat"):  # two runs at one node do not fit a range of one
                    assert reruns > 0, case["name"]
            else:
                assert reruns == 0, (case["name"], kn)
            if kn[0][0] == "breakpoints_chunk":  # the text arrives in pieces as small as asked
                g.configure(*kn[0])
                pieces = text_pieces(g, ref, names, p["min_ref"], p["max_ref"])
                g.configure(kn[0][0], 0)
                assert all(n <= kn[0][1] for n in pieces) and sum(pieces) == len(want[1]) and len(pieces) >= len(want[1]) // kn[0][1]
        g.close()
    return reruns_seen


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def genome_case(k):
    """a 2 kb reference of two chromosomes; both colours carry six substitutions, colour 0 more substitutions and indels,
    colour 1 others, an inversion and a translocation (a stretch of chromosome 2 moved into chromosome 1)"""
    rng = random.Random(7300 + k)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    chr1, chr2 = rs(1200), rs(800)
    shared = []  # substitutions that both colours carry: their calls merge
    for q in (chr1, chr2):
        s = list(q)
        for at in rng.sample(range(50, len(s) - 50), 3):
            s[at] = rng.choice([c for c in "ACGT" if c != s[at]])
        shared.append("".join(s))
    cols = []
    for col in range(2):
        seqs = []
        for q in shared:
            s = list(q)
            for at in rng.sample(range(50, len(s) - 50), 5):
                s[at] = rng.choice([c for c in "ACGT" if c != s[at]])
            for at in sorted(rng.sample(range(50, len(s) - 50), 2), reverse=True):
                if rng.random() < 0.5:
                    del s[at:at + rng.randrange(1, 4)]
                else:
                    s[at:at] = list(rs(rng.randrange(1, 4)))
            seqs.append("".join(s))
        if col == 1:
            a, b = seqs
            a = a[:300] + rc(a[300:300 + 3 * k]) + a[300 + 3 * k:]
            seqs = [a[:700] + b[400:400 + 4 * k] + a[700:], b[:400] + b[400 + 4 * k:]]
        cols.append(seqs)
    return R.build(cols + [[]], k), [chr1, chr2]


@pytest.mark.parametrize("k", BC.KS + BC.WIDE_KS)
def test_random_genome(k):
    graph, ref = genome_case(k)
    names = ["one", "two"]
    recs, text, stats, events, _ = B.call(graph, k, 3, ref, names, 5, 1000)
    want = want_of(recs, text, stats)
    assert stats["calls"] > 10 and events["allele_run_minus"] and stats["stop_runs"]
    for cap in (1 << 13, 1 << 16):
        for batch in (0, 5):
            g = load(graph, k, 3, cap)
            g.configure("breakpoints_batch", batch)
            got, _ = device_run(g, k, ref, names, 5, 1000)
            print("k=%d cap=%d batch=%d: %s" % (k, cap, batch, got[2]))
            check(got, want, (k, cap, batch))
            g.close()


def test_ref_loaded_second_calls():
    k = 11
    case = next(c for c in BC.cases() if c["name"] == "twosnps_k11")
    ref, names = case["ref"], case["names"]
    g = load(case["graph"], k, case["ncols"])
    recs, text, stats, _, with_ref = BC.run(case)
    check(device_run(g, k, ref, names, 5, 1000)[0], want_of(recs, text, stats), "first")
    texts = {text}
    for min_ref, max_ref in ((1, 0), (3, 6), (8, 8), (12, 1000), (40, 0)):
        want = B.call(with_ref, k, case["ncols"], ref, names, min_ref, max_ref, ref_loaded=True)
        texts.add(want[1])
        check(device_run(g, k, ref, names, min_ref, max_ref, ref_loaded=True)[0], want_of(*want[:3]), (min_ref, max_ref))
    assert len(texts) >= 3  # the limits change the calls
    g.close()
    # the reference loaded by a call of its own, then the calls
    g = load(case["graph"], k, case["ncols"])
    st = mcx.graph.BreakpointsStats()
    assert g.breakpoints(ref, names, stats=st, load_only=True)[1] == b"" and g.nkmers == len(with_ref)
    assert st.as_dict() == dict(dict.fromkeys(B.STAT_NAMES, 0), ref_added=stats["ref_added"])
    want = B.call(with_ref, k, case["ncols"], ref, names, 5, 1000, ref_loaded=True)
    check(device_run(g, k, ref, names, 5, 1000, ref_loaded=True)[0], want_of(*want[:3]), "loaded apart")
    g.close()


def fasta(name):
    names, seqs = [], []
    with open(os.path.join(GOLDEN, name)) as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].strip())
                seqs.append("")
            else:
                seqs[-1] += line.strip()
    return names, seqs


def test_breakpoint1_fixture():
    k = 11
    names, ref = fasta("breakpoint1_ref.fa")
    _, sample = fasta("breakpoint1_sample.fa")
    graph = R.build([[s.upper() for s in sample], []], k)
    recs, text, stats, _, _ = B.call(graph, k, 2, ref, names, 5, 1000)
    assert stats["calls"] >= 7
    g = load(graph, k, 2)
    check(device_run(g, k, ref, names, 5, 1000)[0], want_of(recs, text, stats), "breakpoint1")
    g.close()
    # without the reference's edges
    recs, text, stats, _, _ = B.call(graph, k, 2, ref, names, 5, 1000, ref_edges=False)
    g = load(graph, k, 2)
    check(device_run(g, k, ref, names, 5, 1000, ref_edges=False)[0], want_of(recs, text, stats), "breakpoint1 -E")
    g.close()


def test_no_ref_edges_changes_the_outcome():
    cases = {c["name"]: c for c in BC.cases()}
    for k in BC.KS:
        assert BC.run(cases["exact_k%d" % k])[1] != BC.run(cases["exact_edges_k%d" % k])[1]


def test_refusals():
    k = 11
    case = next(c for c in BC.cases() if c["name"] == "snp_k11")
    ref, names = case["ref"], case["names"]
    g = load(case["graph"], k, case["ncols"])
    for kw in ({"min_ref": 0}, {"min_ref": 9, "max_ref": 8}, {"ref_seqs": [], "names": []}):
        args = dict(ref_seqs=ref, names=names, min_ref=5, max_ref=1000)
        args.update(kw)
        with pytest.raises(mcx.graph.McxError) as e:
            g.breakpoints(**args)
        assert e.value.code == mcx.graph.MCX_ERR_ARG, kw
    st = mcx.graph.BreakpointsStats()
    none = ctypes.cast(None, mcx.graph.SINK_FN)
    bases = ctypes.create_string_buffer(ref[0].encode())
    off = (ctypes.c_uint64 * 2)(0, len(ref[0]))
    nbuf = ctypes.create_string_buffer(b"chr1")
    noff = (ctypes.c_uint64 * 2)(0, 4)
    call = lambda prm, n=1, o=off: g.L.mcx_graph_breakpoints(g.h, bases, o, n, nbuf, noff, prm, none, None, none, None, ctypes.byref(st))  # noqa: E731
    assert call(None) == mcx.graph.MCX_ERR_ARG
    assert call(ctypes.byref(mcx.graph.BreakpointsParams(5, 1000, 8))) == mcx.graph.MCX_ERR_ARG  # an unknown flag
    assert call(ctypes.byref(mcx.graph.BreakpointsParams(5, 1000, 2 | 4))) == mcx.graph.MCX_ERR_ARG  # loaded and load only
    assert call(ctypes.byref(mcx.graph.BreakpointsParams(5, 1000, 0)), n=(1 << 30) + 1) == mcx.graph.MCX_ERR_ARG  # too many sequences
    assert "2^30" in mcx.lib().mcx_last_error().decode()
    assert call(ctypes.byref(mcx.graph.BreakpointsParams(5, 1000, 0)), o=(ctypes.c_uint64 * 2)(0, (1 << 32) + 1)) == mcx.graph.MCX_ERR_ARG  # too long
    assert "2^32" in mcx.lib().mcx_last_error().decode()
    assert not any(st.as_dict().values()) and g.nkmers == len(case["graph"])  # a refused call adds nothing
    # both sinks NULL: fine; the stats add up over calls
    assert call(ctypes.byref(mcx.graph.BreakpointsParams(5, 1000, 0))) == mcx.graph.MCX_OK
    once = st.as_dict()
    assert once["calls"] == BC.run(case)[2]["calls"] > 0
    assert call(ctypes.byref(mcx.graph.BreakpointsParams(5, 1000, mcx.graph.BREAKPOINTS_REF_LOADED))) == mcx.graph.MCX_OK
    assert st.calls == 2 * once["calls"] and st.breaks == 2 * once["breaks"] and st.ref_added == once["ref_added"]
    g.close()
    g = mcx.Graph(k, 1, 1 << 14)
    with pytest.raises(mcx.graph.McxError, match="colour") as e:
        g.breakpoints(ref, names)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
    g = mcx.Graph(k, 2, 1 << 14, devices=[0, 0])
    with pytest.raises(mcx.graph.McxError, match="split over devices") as e:
        g.breakpoints(ref, names)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
    g = mcx.Graph(k, 3, 1 << 14)
    g.configure("intersect", 1)
    with pytest.raises(mcx.graph.McxError, match="intersect") as e:
        g.breakpoints(ref, names)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
