"""`contigs` on the MI355X (Graph.links_load_text, Graph.contigs, csrc/mcx_contigs.h) against the CPU restatement in
contigs_restate.py, by exact equality: every record field (the doubles bit for bit), the sequence bytes and the stats.
Every case of contigs_cases.py (k = 5, 9, 31, 33: keys of one and two words); the same with "contigs_batch" 1 and 2,
"contigs_nodes" 2, "contigs_held" 1 and "grid" 1, where the output is identical and the rerun counter moves; the load
round trip of links made by Graph.thread; a k-mer that is not in the graph; a random 2 kb genome with a repeat per k,
threaded on the device, every key a seed, both seeding modes; the refusals.  At k = 63, 65, 95, 97 and 127 (keys of two,
three and four words): the wide cases under three of the knobs, the random genome, and at k = 63, 95, 127 the file of keys
that agree in their high words, loaded, written back and walked from every key and from shuffled seed reads."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import contigs_cases as CC  # noqa: E402
import contigs_restate as G  # noqa: E402
import links_cases as LC  # noqa: E402
import thread_restate as T  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("contigs", "num_reseed_abort", "seeds_not_found", "stop_causes", "wlk_steps", "total_nodes", "total_junc", "corrupt_links")


def load(graph, k, ncols=1, cap=1 << 14):
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


def words(key, k):
    W = (2 * k + 63) // 64
    return [(key >> (64 * (W - 1 - i))) & (2**64 - 1) for i in range(W)] + [0] * (4 - W)


def want_of(recs, seq, st, k):
    out = []
    for r in recs:
        out.append((words(r["seed"], k), r["len_nodes"], r["seq_off"], r["num_junc"], r["paths_held"], r["paths_cntr"], r["max_step_gap"],
                    [G.bits(x) for x in r["gap_conf"]], r["stop_causes"], r["outdegree_rv"], r["outdegree_fw"]))
    return out, seq, {f: st[f] for f in STAT_FIELDS}


def got_of(recs, seq, st):
    out = []
    for r in recs:
        out.append(([int(x) for x in r["seed_key"]], int(r["len_nodes"]), int(r["seq_off"]), int(r["num_junc"]), [int(x) for x in r["paths_held"]],
                    [int(x) for x in r["paths_cntr"]], [int(x) for x in r["max_step_gap"]], [int(x) for x in r["gap_conf"].view(np.uint64)],
                    [int(x) for x in r["stop_causes"]], int(r["outdegree_rv"]), int(r["outdegree_fw"])))
    d = st.as_dict()
    return out, seq, {f: d[f] for f in STAT_FIELDS}


def device_run(g, case):
    p = case["params"]
    flags = p.get("flags", 0)
    return g.contigs(case["conf"], colour=p.get("colour", 0), seeds=p.get("seeds"), reseed=bool(flags & G.RESEED), missing_check=not (flags & G.NO_MISSING_CHECK),
                     ncontigs=p.get("ncontigs", 0), min_step_confid=p.get("min_step", -1.0), min_cumul_confid=p.get("min_cumul", -1.0))


def check(got, want, what):
    if got != want:
        for a, b in zip(got[0], want[0]):
            assert a == b, (what, a, b)
        assert got[2] == want[2], (what, got[2], want[2])
        assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
        raise AssertionError((what, "the sequences differ", got[1][:200], want[1][:200]))


KNOBS = ((), (("contigs_batch", 1),), (("contigs_batch", 2),), (("contigs_nodes", 2),), (("contigs_held", 1),), (("grid", 1),))


WIDE_KNOBS = ((), (("contigs_batch", 1),), (("contigs_nodes", 2),))


@pytest.mark.parametrize("k", CC.KS)
def test_cases(k):
    reruns = run_cases(k, CC.cases(), KNOBS)
    assert reruns[()] == 0 and reruns[(("contigs_batch", 1),)] == 0 and reruns[(("grid", 1),)] == 0
    assert reruns[(("contigs_nodes", 2),)] > 0 and reruns[(("contigs_held", 1),)] > 0, reruns


@pytest.mark.parametrize("k", CC.WIDE_KS)
def test_wide_cases(k):
    """the same structures at keys of two, three and four words with a full and a 2-bit top word, under three of the knobs"""
    reruns = run_cases(k, CC.wide_cases(), WIDE_KNOBS)
    assert reruns[()] == 0 and reruns[(("contigs_batch", 1),)] == 0
    assert reruns[(("contigs_nodes", 2),)] > 0, reruns


def run_cases(k, cases, knobs):
    """every case of `cases` at k under every knob against the restatement -> the reruns per knob"""
    handles = {}
    reruns = {kn: 0 for kn in knobs}
    for case in (c for c in cases if c["k"] == k):
        g = handles.get(id(case["graph"]))
        if g is None:
            g = handles[id(case["graph"])] = load(case["graph"], k, case["ncols"])
        g.links_reset()
        text = CC.links_text(case)
        if text:
            assert g.links_load_text(text) == (len(case["links"]), 0)
        want = want_of(*CC.run(case), k)
        for kn in knobs:
            for key, v in kn:
                g.configure(key, v)
            recs, seq, st = device_run(g, case)
            for key, _ in kn:
                g.configure(key, 0)
            print(case["name"], kn, "contigs", int(st.contigs), "reruns", int(st.reruns))
            check(got_of(recs, seq, st), want, (case["name"], kn))
            if case["name"].startswith("rho"):  # stopped by the repeat rule after rounds with a link held
                assert any(6 in list(r["stop_causes"]) and r["num_junc"] > 0 for r in recs)
            reruns[kn] += int(st.reruns)
    for g in handles.values():
        g.close()
    return reruns


def genome_case(k):
    rng = random.Random(4100 + k)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    rep = rs(k + 20)
    gen = rs(600) + rep + rs(650) + rep + rs(2000 - 1250 - 2 * len(rep))
    reads = []
    # (at k = 5 the 2 kb genome holds nearly every k-mer, every node is a junction and a read makes a link per node: a
    # dozen short reads give some thousand links there, which is what keeps this case to seconds)
    for _ in range(150 if k > 5 else 12):
        n = rng.randrange(max(2 * k, 80), 400) if k > 5 else rng.randrange(30, 80)
        a = rng.randrange(0, len(gen) - n)
        s = gen[a:a + n]
        reads.append(s if rng.random() < 0.5 else s[::-1].translate(str.maketrans("ACGT", "TGCA")))
    return R.build([[gen]], k), reads


@pytest.mark.parametrize("k", CC.KS + CC.WIDE_KS)
def test_random_genome_round_trip_and_all_seeds(k):
    graph, reads = genome_case(k)
    g = load(graph, k)
    g.thread(*arrays(reads))
    store = T.Store(graph, k).thread(reads)
    text, info = g.links_text(seq=True), g.links_info()
    assert text == store.text(seq=True) and info == store.info()
    # the load round trip: with the tags and without them
    for seq in (True, False):
        body = g.links_text(seq=seq)
        g.links_reset()
        assert g.links_info()["num_paths"] == 0
        assert g.links_load_text(body) == (info["num_paths"], 0)
        assert g.links_text(seq=True) == text and g.links_info() == info
    # loading the same links again adds the counts
    g.links_load_text(text)
    twice = T.Store(graph, k).thread(reads + reads)
    assert g.links_text(seq=False) == twice.text(seq=False)
    g.links_reset()
    g.links_load_text(text)
    links = [(key, o, b, n) for (key, o, b), n in store.links.items()]
    conf = G.conf_table(dict(store.contig_hist()), len(graph))
    for flags, ncontigs in ((0, 0), (G.RESEED, 40), (G.NO_MISSING_CHECK, 0)):
        want = want_of(*G.assemble(graph, k, links, conf, 0, flags, ncontigs), k)
        for batch in (0, 7):
            g.configure("contigs_batch", batch)
            recs, seq, st = g.contigs(conf, reseed=bool(flags & G.RESEED), missing_check=not (flags & G.NO_MISSING_CHECK), ncontigs=ncontigs)
            print("k=%d flags=%d batch=%d: %s" % (k, flags, batch, st.as_dict()))
            check(got_of(recs, seq, st), want, (k, flags, batch))
    g.configure("contigs_batch", 0)
    assert want[2]["wlk_steps"][G.USELINKS] > 0
    g.close()


@pytest.mark.parametrize("k", LC.SHARED_KS)
def test_keys_that_agree_in_their_high_words(k):
    """the file of links_cases.shared_high_words on a graph of exactly its k-mers (no edges): groups of keys that differ in
    their last word only, or first in a middle word with the lower words sorting the other way round, and k-mer lines
    that hold the reverse complement.  The load (k_cg_kmers), the store's key sort and its text (k_th_text), then contigs
    with every key a seed (k_cg_keyword and the key sort) and with the k-mers as seed reads in shuffled order"""
    text, groups = LC.shared_high_words(k)
    kmers = [s for _, ks, _ in groups for s in ks]
    graph = R.build([kmers], k)
    assert sorted(graph) == sorted(R.kmer_int(s) for s in kmers) and not any(ed[0] for _, ed in graph.values())
    g = load(graph, k)
    links = LC.stored(text, k)
    nlines = sum(ln[:2] in (b"F ", b"R ") for ln in text.split(b"\n"))
    assert g.links_load_text(text) == (nlines, 0)
    body = CC.links_text({"k": k, "links": links})
    info = {"num_kmers_with_paths": len({l[0] for l in links}), "num_paths": len(links), "path_bytes": sum((len(l[2]) + 3) // 4 for l in links)}
    assert g.links_text(seq=False) == body and g.links_info() == info
    g.links_reset()
    assert g.links_load_text(body) == (len(links), 0)
    assert g.links_text(seq=False) == body and g.links_info() == info
    conf = G.conf_table({}, len(graph))
    rng = random.Random(k)
    seeds = [s if rng.random() < 0.5 else LC.revcomp(s) for s in kmers] + kmers[:2]
    rng.shuffle(seeds)
    for sd in (None, seeds):
        for flags in (0, G.RESEED):
            want = want_of(*G.assemble(graph, k, links, conf, 0, flags, 0, -1.0, -1.0, sd), k)
            recs, seq, st = g.contigs(conf, seeds=sd, reseed=bool(flags & G.RESEED))
            check(got_of(recs, seq, st), want, (k, sd is None, flags))
            keys = [r[0] for r in want[0]]
            assert len(keys) == len(kmers) + (2 if sd and flags else 0) and (keys == sorted(keys)) == (sd is None)
    g.close()


def test_missing_kmers_and_bad_lines():
    k = 9
    case = next(c for c in CC.cases() if c["name"] == "repeat_k9")
    g = load(case["graph"], k)
    text = CC.links_text(case)
    absent = next(s for s in ("ACGTTGCAA", "AAAAAAAAC", "CCCCCCCCA") if R.canon(R.kmer_int(s), k) not in case["graph"])
    with pytest.raises(mcx.graph.McxError) as e:
        g.links_load_text(text + ("%s 1\nF 1 1 A\n" % absent).encode())
    assert e.value.code == mcx.graph.MCX_ERR_INVAL and e.value.nmissing == 1
    assert g.links_info()["num_paths"] == 0
    for bad in (b"F 1 1 A\n", text + b"X 1 1 A\n", text + b"F 2 1 A\n", text + b"F 1 1 N\n", text + b"F 1 1,2 A\n", text + b"F 0 1 \n"):
        with pytest.raises(mcx.graph.McxError) as e:
            g.links_load_text(bad)
        assert e.value.code == mcx.graph.MCX_ERR_INVAL and e.value.nmissing == 0, bad
        assert g.links_info()["num_paths"] == 0
    # a k-mer line that holds the reverse complement: the links turn round
    key, o, b, n = case["links"][0]
    rc = T.kmer_str(R.revcomp(key, k), k)
    if rc != T.kmer_str(key, k):
        g.links_load_text(("%s 1\n%s %d %d %s\n" % (rc, "FR"[1 - o], len(b), n, "".join("ACGT"[x] for x in b))).encode())
        assert g.links_text(seq=False) == CC.links_text({"k": k, "links": [case["links"][0]]})
    g.close()


def test_refusals():
    k = 9
    case = next(c for c in CC.cases() if c["name"] == "repeat_k9")
    g = load(case["graph"], k)
    for kw in ({"colour": 1}, {"min_step_confid": float("nan")}):
        with pytest.raises(mcx.graph.McxError) as e:
            g.contigs(case["conf"], **kw)
        assert e.value.code == mcx.graph.MCX_ERR_ARG
    prm = mcx.graph.ContigsParams(0, 4, 0, -1.0, -1.0, None, 0)
    import ctypes
    st = mcx.graph.ContigsStats()
    none = ctypes.cast(None, mcx.graph.SINK_FN)
    assert g.L.mcx_graph_contigs(g.h, None, None, 0, ctypes.byref(prm), none, None, none, None, ctypes.byref(st)) == mcx.graph.MCX_ERR_ARG
    prm = mcx.graph.ContigsParams(0, 0, 0, -1.0, -1.0, None, 5)
    assert g.L.mcx_graph_contigs(g.h, None, None, 0, ctypes.byref(prm), none, None, none, None, ctypes.byref(st)) == mcx.graph.MCX_ERR_ARG
    for seeds in (["ACGT"], ["ACGTNACGT"]):
        with pytest.raises(mcx.graph.McxError) as e:
            g.contigs(case["conf"], seeds=seeds)
        assert e.value.code == mcx.graph.MCX_ERR_INVAL
    # no links, no seeds, both sinks NULL: fine
    recs, seq, st = g.contigs((), seeds=[])
    assert len(recs) == 0 and seq == b"" and st.contigs == 0
    prm = mcx.graph.ContigsParams(0, 0, 0, -1.0, -1.0, None, 0)
    st = mcx.graph.ContigsStats()
    assert g.L.mcx_graph_contigs(g.h, None, None, 0, ctypes.byref(prm), none, None, none, None, ctypes.byref(st)) == mcx.graph.MCX_OK
    assert st.contigs == CC.run(next(c for c in CC.cases() if c["name"] == "repeat_no_links_k9"))[2]["contigs"]
    g.close()
    g = mcx.Graph(k, 1, 1 << 14, devices=[0, 0])
    with pytest.raises(mcx.graph.McxError):
        g.contigs(())
    with pytest.raises(mcx.graph.McxError):
        g.links_load_text(b"ACGTTGCAA 1\nF 1 1 A\n")
    g.close()
