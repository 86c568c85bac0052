"""`bubbles` on the MI355X (Graph.bubbles, csrc/mcx_bubbles.h) against the CPU restatement in bubbles_restate.py, by exact
equality: every record field, the text bytes and every stat.  Every case of bubbles_cases.py (k = 11, 31, 33: keys of one
and two words); the same with "bubbles_batch" 1 and 2, "grid" 1 and "bubbles_chunk" 1, 7 and 64, where a seam falls inside
headers, sequences and the blank line; a random 2 kb genome per k (with a repeat that differs in one base) whose second and third colour carry 10 substitutions
and 2 indels, with and without a haploid colour and at two table capacities; a graph without a fork; the ABI symbol and the
refusals.  At k = 63, 65, 95, 97 and 127 (keys of two, three and four words): the wide cases without a knob, with
"bubbles_batch" 1 and with "bubbles_chunk" 7, and the random genome."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bubbles_cases as BC  # noqa: E402
import bubbles_restate as B  # noqa: E402
import clean_restate as R  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu
REC_FIELDS = ("fork_orient", "num_branches", "flank5p_kmers", "flank3p_kmers", "text_off", "text_len")


def load(graph, k, ncols, cap=1 << 14):
    g = mcx.Graph(k, ncols, cap)
    g.add_records(R.pack(graph, k, ncols), ncols, [(c, c) for c in range(ncols)])
    g.sync()
    assert g.nkmers == len(graph)
    return g


def want_of(recs, text, stats):
    return [(r["fork_key"],) + tuple(r[f] for f in REC_FIELDS) for r in recs], text.encode(), dict(stats)


def got_of(recs, text, st, k):
    W = (2 * k + 63) // 64
    out = []
    for r in recs:
        key = 0
        for i in range(W):
            key = (key << 64) | int(r["fork_key"][i])
        assert all(int(x) == 0 for x in r["fork_key"][W:])
        out.append((key,) + tuple(int(r[f]) for f in REC_FIELDS))
    return out, text, st.as_dict()


def device_run(g, k, max_allele, max_flank, haploid=(), keep_serial=False):
    st = mcx.graph.BubblesStats()
    recs, text = g.bubbles(max_allele, max_flank, haploid, keep_serial, stats=st)
    return got_of(recs, text, st, k)


def text_pieces(g, p):
    """the sizes in which the text sink receives the text"""
    pieces = []

    def sink(_ctx, _ptr, n):
        pieces.append(n)
        return 0
    hap = (ctypes.c_uint32 * max(1, len(p["haploid"])))(*p["haploid"])
    prm = mcx.graph.BubblesParams(p["max_allele"], p["max_flank"], mcx.graph.BUBBLES_KEEP_SERIAL if p["keep_serial"] else 0, len(p["haploid"]),
                                  ctypes.cast(hap, ctypes.c_void_p))
    assert g.L.mcx_graph_bubbles(g.h, ctypes.byref(prm), ctypes.cast(None, mcx.graph.SINK_FN), None, mcx.graph.SINK_FN(sink), None, None) == mcx.graph.MCX_OK
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
    assert hasattr(mcx.lib(), "mcx_graph_bubbles")
    assert callable(mcx.Graph.bubbles) and set(B.STAT_NAMES) == set(mcx.graph.BubblesStats().as_dict())
    assert mcx.graph.BUBBLE_REC.itemsize == 64


KNOBS = ((), (("bubbles_batch", 1),), (("bubbles_batch", 2),), (("grid", 1),), (("bubbles_chunk", 1),), (("bubbles_chunk", 7),), (("bubbles_chunk", 64),))


WIDE_KNOBS = ((), (("bubbles_batch", 1),), (("bubbles_chunk", 7),))


@pytest.mark.parametrize("k", BC.KS)
def test_cases(k):
    run_cases(k, BC.cases(), KNOBS)


@pytest.mark.parametrize("k", BC.WIDE_KS)
def test_wide_cases(k):
    """the same structures at keys of two, three and four words with a full and a 2-bit top word, under three of the knobs:
    a text seam every 7 bytes falls inside k-mers of up to 127 bases"""
    run_cases(k, BC.wide_cases(), WIDE_KNOBS)


def run_cases(k, cases, knobs):
    """every case of `cases` at k under every knob against the restatement"""
    handles = {}
    for case in (c for c in cases if c["k"] == k):
        g = handles.get(id(case["graph"]))
        if g is None:
            g = handles[id(case["graph"])] = load(case["graph"], k, case["ncols"])
        recs, text, stats, _ = BC.run(case)
        want = want_of(recs, text, stats)
        p = case["params"]
        for kn in knobs:
            for key, v in kn:
                g.configure(key, v)
            got = device_run(g, k, p["max_allele"], p["max_flank"], p["haploid"], p["keep_serial"])
            for key, _ in kn:
                g.configure(key, 0)
            print(case["name"], kn, got[2])
            check(got, want, (case["name"], kn))
            if kn and kn[0][0] == "bubbles_chunk":  # the text arrives in pieces as small as asked
                g.configure(*kn[0])
                pieces = text_pieces(g, p)
                g.configure(kn[0][0], 0)
                assert all(n <= kn[0][1] for n in pieces) and sum(pieces) == len(want[1]) and len(pieces) >= len(want[1]) // kn[0][1]
    for g in handles.values():
        g.close()


def genome_case(k):
    rng = random.Random(5200 + k)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    rep = rs(3 * k)  # a repeat with a substitution in its second copy: a bubble inside every colour, which a haploid colour drops
    rep2 = rep[:len(rep) // 2] + next(c for c in "ACGT" if c != rep[len(rep) // 2]) + rep[len(rep) // 2 + 1:]
    gen = rs(600) + rep + rs(700) + rep2 + rs(700 - 2 * len(rep))
    cols = [gen]
    for _ in range(2):
        s = list(gen)
        for at in rng.sample(range(50, 1950), 10):
            s[at] = rng.choice([c for c in "ACGT" if c != s[at]])
        for at in sorted(rng.sample(range(50, 1950), 2), reverse=True):
            if rng.random() < 0.5:
                del s[at:at + rng.randrange(1, 4)]
            else:
                s[at:at] = list(rs(rng.randrange(1, 4)))
        cols.append("".join(s))
    return R.build([[c] for c in cols], k)


@pytest.mark.parametrize("k", BC.KS + BC.WIDE_KS)
def test_random_genome(k):
    graph = genome_case(k)
    max_allele = BC.limit(100, k)  # (100 at every k of KS; at k = 127 no allele is as short as 100 k-mers)
    wants = {hap: want_of(*B.call(graph, k, 3, max_allele, 60, hap)[:3]) for hap in ((), (0,))}
    assert wants[()][2]["bubbles"] > 0 and wants[(0,)][2]["haploid_dropped"] > 0 and wants[()][2]["haploid_dropped"] == 0
    for cap in (1 << 13, 1 << 16):
        g = load(graph, k, 3, cap)
        for hap in ((), (0,)):
            for batch in (0, 5):
                g.configure("bubbles_batch", batch)
                got = device_run(g, k, max_allele, 60, hap)
                print("k=%d cap=%d hap=%s batch=%d: %s" % (k, cap, hap, batch, got[2]))
                check(got, wants[hap], (k, cap, hap, batch))
        g.close()


def test_no_fork_gives_an_empty_body():
    k = 11
    graph = R.build([["ACGTTGCATGTCGCATGATGCATGAGAGCT"], ["ACGTTGCATGTCGCATGATGCATGAGAGCT"]], k)
    g = load(graph, k, 2)
    got = device_run(g, k, 50, 50)
    assert got == ([], b"", dict.fromkeys(B.STAT_NAMES, 0))
    g.close()
    g = mcx.Graph(k, 2, 1 << 10)  # no k-mer at all
    assert device_run(g, k, 50, 50) == ([], b"", dict.fromkeys(B.STAT_NAMES, 0))
    g.close()


def test_refusals():
    k = 11
    case = next(c for c in BC.cases() if c["name"] == "snp_k11")
    g = load(case["graph"], k, case["ncols"])
    for kw in ({"max_allele": 0}, {"max_flank": 0}, {"haploid": (3,)}, {"haploid": tuple([0] * 65)}, {"max_allele": 1 << 30}):
        args = dict(max_allele=50, max_flank=50)
        args.update(kw)
        with pytest.raises(mcx.graph.McxError) as e:
            g.bubbles(**args)
        assert e.value.code == mcx.graph.MCX_ERR_ARG, kw
    st = mcx.graph.BubblesStats()
    none = ctypes.cast(None, mcx.graph.SINK_FN)
    assert g.L.mcx_graph_bubbles(g.h, None, none, None, none, None, ctypes.byref(st)) == mcx.graph.MCX_ERR_ARG
    prm = mcx.graph.BubblesParams(100, 5, 2, 0, None)  # an unknown flag
    assert g.L.mcx_graph_bubbles(g.h, ctypes.byref(prm), none, None, none, None, ctypes.byref(st)) == mcx.graph.MCX_ERR_ARG
    assert not any(st.as_dict().values())
    # both sinks NULL and no stats: fine; the stats add up over calls
    prm = mcx.graph.BubblesParams(100, 5, 0, 0, None)
    assert g.L.mcx_graph_bubbles(g.h, ctypes.byref(prm), none, None, none, None, None) == mcx.graph.MCX_OK
    assert g.L.mcx_graph_bubbles(g.h, ctypes.byref(prm), none, None, none, None, ctypes.byref(st)) == mcx.graph.MCX_OK
    assert g.L.mcx_graph_bubbles(g.h, ctypes.byref(prm), none, None, none, None, ctypes.byref(st)) == mcx.graph.MCX_OK
    once = BC.run(case)[2]
    assert st.as_dict() == {n: 2 * v for n, v in once.items()}
    g.close()
    g = mcx.Graph(k, 2, 1 << 14, devices=[0, 0])
    with pytest.raises(mcx.graph.McxError, match="split over devices") as e:
        g.bubbles(50, 50)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
    g = mcx.Graph(k, 2, 1 << 14)
    g.configure("intersect", 1)
    with pytest.raises(mcx.graph.McxError, match="intersect") as e:
        g.bubbles(50, 50)
    assert e.value.code == mcx.graph.MCX_ERR_ARG
    g.close()
