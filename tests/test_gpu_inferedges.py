"""`inferedges` on the MI355X: the replays of the reference's tests/inferedges/Makefile (CAAGG at k = 5,
the mix graphs at k = 11, all three I/O modes), randomised parity against a restatement of
infer_kmer_edges (src/tools/infer_edges.c) for k = 3 .. 127, and the C ABI / Python entry points.
The restatement is pinned on the CPU (C oracle build of the CAAGG graphs) before it serves as the
expectation."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from oracle import ctxio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mccortex_amd", "bin")


# ---- restatement ------------------------------------------------------------------------------
def kmer_int(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def revcomp(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canon(x, k):
    return min(x, revcomp(x, k))  # binary_kmer_get_key: top word first == integer order


def parse(buf, k, ncols, hdr_size=0):
    """.ctx body bytes -> [(key int, covgs tuple, edges list)]"""
    W = (2 * k + 63) // 64
    keys, covgs, edges = ctxio.records(buf, {"num_words": W, "num_cols": ncols}, hdr_size)
    out = []
    for i in range(len(keys)):
        key = 0
        for w in keys[i]:
            key = (key << 64) | int(w)
        out.append((key, tuple(int(c) for c in covgs[i]), [int(e) for e in edges[i]]))
    return out


def pack(recs, k, ncols):
    W = (2 * k + 63) // 64
    parts = []
    for key, cv, ed in recs:
        words = [(key >> (64 * (W - 1 - i))) & (2**64 - 1) for i in range(W)]
        parts.append(struct.pack("<%dQ%dI" % (W, ncols), *words, *cv) + bytes(ed))
    return b"".join(parts)


def infer_kmer_edges(key, covgs, edges, k, pop, present):
    """infer_edges.c:infer_kmer_edges; present(neighbour key, colour) -> bool, None when not in the graph"""
    uedges, iedges = 0, 0xF
    for e in edges:
        uedges |= e
        iedges &= e
    add = (uedges & ~iedges if pop else ~iedges) & 0xFF
    new = list(edges)
    if not add:
        return new
    mask = (1 << (2 * k)) - 1
    for orient in (0, 1):
        for nuc in range(4):
            bit = 1 << (nuc + 4 * orient)
            if not bit & add:
                continue
            nb = ((key << 2) | nuc) & mask if orient == 0 else (key >> 2) | ((3 - nuc) << (2 * k - 2))
            nk = canon(nb, k)
            for c in range(len(edges)):
                if covgs[c] > 0 and present(nk, c):
                    new[c] |= bit
    return new


def expect_file(recs, k, ncols, pop):
    """file mode: presence = covg || edges per colour of every loaded record (graphs_load.c:121-154)"""
    pres = {}
    for key, cv, ed in recs:
        if any(cv):
            m = pres.get(key, 0)
            for c in range(ncols):
                if cv[c] or ed[c]:
                    m |= 1 << c
            pres[key] = m
    out, nmod = [], 0
    for key, cv, ed in recs:
        new = infer_kmer_edges(key, cv, ed, k, pop, lambda nk, c: (pres.get(nk, 0) >> c) & 1)
        nmod += new != ed
        out.append((key, cv, new))
    return out, nmod, len(pres)


def merge(recs, ncols):
    m = {}
    for key, cv, ed in recs:
        if not any(cv):
            continue
        c0, e0 = m.get(key, ([0] * ncols, [0] * ncols))
        m[key] = ([min(0xFFFFFFFF, a + b) for a, b in zip(c0, cv)], [a | b for a, b in zip(e0, ed)])
    return m


def expect_stream(recs, k, ncols, pop):
    """stream mode: the merged graph, presence = coverage (infer_edges.c:_add_edge_to_colours)"""
    m = merge(recs, ncols)
    out, nmod = [], 0
    for key, (cv, ed) in m.items():
        new = infer_kmer_edges(key, cv, ed, k, pop, lambda nk, c: nk in m and m[nk][0][c] > 0)
        nmod += new != ed
        out.append((key, tuple(cv), new))
    return sorted(out), nmod, len(m)


# ---- the CAAGG graphs (tests/inferedges/Makefile) ------------------------------------------------
LEFT_EDGES = ["ACAAG", "CCAAGG", "GCAAG", "TCAAG"]
RIGHT_EDGES = ["AAGGA", "AAGGC", "AAGGG", "CAAGGT"]
LEFT_KMERS = ["CAAGG", "ACAAG", "CCAAG", "GCAAG", "TCAAG"]
RIGHT_KMERS = ["CAAGG", "AAGGA", "AAGGC", "AAGGG", "AAGGT"]
CAAGG_COLS = [LEFT_EDGES + RIGHT_EDGES, LEFT_KMERS, RIGHT_KMERS, LEFT_KMERS + RIGHT_KMERS, []]


def colour_set(recs, c):
    """`view --kmers <graph>:c | sort`: the k-mers with coverage in colour c"""
    return sorted((key, cv[c], ed[c]) for key, cv, ed in recs if cv[c] > 0)


def test_restatement_pinned_on_caagg(orc):
    """CPU: the restatement, run on the C oracle's build of the CAAGG graph, gives what the Makefile's
    diff lines say `inferedges --pop` gives, and the hand-written edges of the drawing in its comment"""
    def graph(cols):
        og = orc.Graph(5, len(cols), 1 << 10)
        for c, reads in enumerate(cols):
            if reads:
                og.add_reads(c, *orc.pack_reads(reads))
        return parse(og.body_bytes(True), 5, len(cols))

    recs = graph(CAAGG_COLS)
    out, nmod, _ = expect_file(recs, 5, 5, pop=True)
    left, right = graph([LEFT_EDGES]), graph([RIGHT_EDGES])
    assert colour_set(out, 0) == colour_set(recs, 0)
    assert colour_set(out, 1) == colour_set(left, 0)
    assert colour_set(out, 2) == colour_set(right, 0)
    assert colour_set(out, 3) == colour_set(recs, 0)
    assert colour_set(out, 4) == []
    # by hand: CCAAG -> CAAGG -> AAGGT are the only edges.  CAAGG is its own key (< CCTTG): forward edge to T
    # (bit 3), reverse edge to CCAAG, whose first base C is added as its complement G (bit 4 + 2)
    caagg = kmer_int("CAAGG")
    edges = {key: ed for key, _, ed in out}[caagg]
    assert edges == [0x48, 0x40, 0x08, 0x48, 0]
    assert nmod == sum(1 for a, b in zip(recs, out) if a[2] != b[2]) == 3  # CAAGG, CCAAG (cols 1, 3), AAGGT (cols 2, 3)


# ---- GPU ---------------------------------------------------------------------------------------
def run(maxk, *args, stdin=None, check=True):
    p = subprocess.run([os.path.join(BIN, "mccortex%d" % maxk)] + [str(a) for a in args], input=stdin,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if check:
        assert p.returncode == 0, p.stderr.decode(errors="replace")
    return p.stdout, p.stderr.decode(errors="replace")


def modified_line(nmod, nk):
    """the status line of ctx_infer_edges.c (ulong_to_str: thousands separated)"""
    return "{:,} of {:,} ({:.2f}%) nodes modified".format(nmod, nk, 100.0 * nmod / nk)


def maxk_for(k):
    return ((k + 31) // 32) * 32 - 1


def read_ctx(path):
    buf = open(path, "rb").read()
    hdr, hs = ctxio.read_header(buf)
    return buf, hdr, hs, parse(buf, hdr["kmer_size"], hdr["num_cols"], hs)


@pytest.fixture(scope="module")
def built(mcx):
    return mcx


def build_cli(tmp_path, k, samples, out):
    """`build -s <name> --seq <file>...` one sample per entry of samples: [(name, [reads])]"""
    args = ["build", "-q", "-m", "8M", "-k", k]
    for i, (name, reads) in enumerate(samples):
        f = tmp_path / ("%s.%d.txt" % (os.path.basename(out), i))
        f.write_text("".join(r + "\n" for r in reads) if reads else "\n")
        args += ["-s", name, "--seq", f]
    run(maxk_for(k), *args, out)
    return out


@pytest.mark.gpu
def test_caagg_replay(built, tmp_path):
    g = build_cli(tmp_path, 5, [("c%d" % c, reads) for c, reads in enumerate(CAAGG_COLS)], tmp_path / "CAAGG.k5.ctx")
    left = build_cli(tmp_path, 5, [("LeftEdges", LEFT_EDGES)], tmp_path / "left.ctx")
    right = build_cli(tmp_path, 5, [("RightEdges", RIGHT_EDGES)], tmp_path / "right.ctx")
    out = tmp_path / "CAAGG.infer.k5.ctx"
    _, err = run(31, "inferedges", "--pop", "-o", out, g)
    buf, _, hs, recs = read_ctx(g)
    obuf, _, ohs, orecs = read_ctx(out)
    assert obuf[:ohs] == buf[:hs]
    assert colour_set(orecs, 0) == colour_set(recs, 0)
    assert colour_set(orecs, 1) == colour_set(read_ctx(left)[3], 0)
    assert colour_set(orecs, 2) == colour_set(read_ctx(right)[3], 0)
    assert colour_set(orecs, 3) == colour_set(recs, 0)
    assert colour_set(orecs, 4) == []
    exp, nmod, nk = expect_file(recs, 5, 5, pop=True)
    assert orecs == exp
    assert modified_line(nmod, nk) in err


def random_reads(rng, n, length):
    return ["".join(rng.choice("ACGT") for _ in range(length)) for _ in range(n)]


@pytest.mark.gpu
def test_mix_replay(built, orc, tmp_path):
    k = 11
    rng = random.Random(11)
    seq = build_cli(tmp_path, k, [("PinkPanther", random_reads(rng, 100, 100))], tmp_path / "seq.ctx")
    run(31, "inferedges", "-q", "--all", seq)
    sbuf, shdr, shs, srecs = read_ctx(seq)
    # every k-mer repeated coverage times: the same k-mers, no edges
    kreads = []
    for key, cv, _ in srecs:
        s = "".join("ACGT"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k))
        kreads += [s] * cv[0]
    noedges = build_cli(tmp_path, k, [("Puma", kreads)], tmp_path / "noedges.ctx")
    nbuf = open(noedges, "rb").read()
    assert all(not any(ed) for _, _, ed in read_ctx(noedges)[3])
    src = {"1": sbuf, "0": nbuf}

    def mix(xy):  # `join`: file X into colour 0, file Y into colour 1
        og = orc.Graph(k, 2, 1 << 16)
        gi = [ctxio.GraphInfo(), ctxio.GraphInfo()]
        ctxio.load_into(og, gi, src[xy[0]], [(0, 0)])
        ctxio.load_into(og, gi, src[xy[1]], [(0, 1)])
        p = tmp_path / ("mix.%s.ctx" % xy)
        p.write_bytes(ctxio.header_bytes(k, gi) + og.body_bytes(True))
        return p

    mixes = {xy: mix(xy) for xy in ("00", "01", "10", "11")}
    recset = lambda p: sorted(read_ctx(p)[3])
    m11, m00 = recset(mixes["11"]), recset(mixes["00"])

    def stream(src_path, mode):
        out, _ = run(31, "inferedges", "-q", "-m", "1M", mode, "-", stdin=open(src_path, "rb").read())
        p = tmp_path / ("stream%s.%s.ctx" % (mode, os.path.basename(str(src_path))))
        p.write_bytes(out)
        return p

    def in_place(src_path, mode):
        p = tmp_path / ("inplace%s.%s" % (mode, os.path.basename(str(src_path))))
        p.write_bytes(open(src_path, "rb").read())
        run(31, "inferedges", "-q", mode, p)
        return p

    def to_file(src_path, mode):
        p = tmp_path / ("out%s.%s" % (mode, os.path.basename(str(src_path))))
        run(31, "inferedges", "-q", mode, "-o", p, src_path)
        return p

    fix1a = recset(stream(mixes["10"], "--all"))
    assert recset(stream(mixes["10"], "--pop")) == m11
    for xy in ("00", "01", "10", "11"):
        outs = {}
        for fn in (in_place, to_file):
            a, p = fn(mixes[xy], "--all"), fn(mixes[xy], "--pop")
            assert recset(a) == fix1a, (xy, fn.__name__)
            assert recset(p) == (m00 if xy == "00" else m11), (xy, fn.__name__)
            outs[fn] = (open(a, "rb").read(), open(p, "rb").read())
        assert outs[in_place] == outs[to_file], xy


def random_graph(rng, k, ncols, nkmers):
    """records of a random genome's k-mers: edges cleared at random per colour, records with zero coverage
    but edges, records with no coverage at all, duplicate keys, unsorted order"""
    mask = (1 << (2 * k)) - 1
    genome = [rng.randrange(4) for _ in range(nkmers + k - 1)]
    keys, x = [], 0
    for i, b in enumerate(genome):
        x = ((x << 2) | b) & mask
        if i >= k - 1:
            keys.append(canon(x, k))
    keys = list(dict.fromkeys(keys))
    recs = []
    for key in keys:
        cv = tuple(rng.choice((0, 0, 1, 2, 7, 0xFFFFFFFF)) if rng.random() < 0.9 else 0 for _ in range(ncols))
        ed = [rng.randrange(256) if rng.random() < 0.5 else 0 for _ in range(ncols)]
        ed = [e if (cv[c] or rng.random() < 0.2) else 0 for c, e in enumerate(ed)]
        recs.append((key, cv, ed))
    recs += [(key, tuple(0 for _ in range(ncols)), [rng.randrange(256) for _ in range(ncols)]) for key in rng.sample(keys, len(keys) // 20)]
    recs += [(key, tuple(rng.randrange(1, 4) for _ in range(ncols)), [rng.randrange(256) for _ in range(ncols)])
             for key in rng.sample(keys, len(keys) // 10)]  # duplicates
    rng.shuffle(recs)
    return recs


PARITY_K = [(3, 1), (5, 3), (11, 9), (21, 1), (31, 3), (33, 9), (47, 1), (63, 3), (65, 9), (95, 1), (97, 3), (127, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("k,ncols", PARITY_K)
def test_randomised_parity(built, tmp_path, k, ncols):
    rng = random.Random(k * 100 + ncols)
    recs = random_graph(rng, k, ncols, min(4 ** k // 3, 3000))
    hdr = ctxio.header_bytes(k, [ctxio.GraphInfo() for _ in range(ncols)])
    src = tmp_path / "in.ctx"
    src.write_bytes(hdr + pack(recs, k, ncols))
    maxk = maxk_for(k)
    for pop in (False, True):
        mode = "--pop" if pop else "--all"
        exp, nmod, nk = expect_file(recs, k, ncols, pop)
        want = hdr + pack(exp, k, ncols)
        line = modified_line(nmod, nk)
        out = tmp_path / ("o%s.ctx" % mode)
        _, err = run(maxk, "inferedges", mode, "-o", out, src)
        assert open(out, "rb").read() == want, mode
        assert line in err, (mode, err)
        ip = tmp_path / ("ip%s.ctx" % mode)
        ip.write_bytes(open(src, "rb").read())
        _, err = run(maxk, "inferedges", mode, ip)
        assert open(ip, "rb").read() == want, mode
        assert line in err, (mode, err)
        sexp, snmod, snk = expect_stream(recs, k, ncols, pop)
        sout, err = run(maxk, "inferedges", mode, "-", stdin=open(src, "rb").read())
        assert sout[:len(hdr)] == hdr
        assert sorted(parse(sout[len(hdr):], k, ncols)) == sexp, mode
        assert modified_line(snmod, snk) in err


def loaded_graph(mcx, k, ncols, recs, capacity):
    g = mcx.Graph(k, ncols, capacity)
    g.add_records(pack(recs, k, ncols), ncols, [(c, c) for c in range(ncols)])
    return g


@pytest.mark.gpu
def test_abi_full_table_device_records_and_chunks(built):
    mcx = built
    k, ncols = 31, 3
    probe = mcx.Graph(k, ncols, 1 << 14)
    slots = probe.capacity()[0] * 32 // 33  # (the hash-addressed slots; the overflow area is 1/32 on top)
    probe.close()
    rng = random.Random(5)
    recs = random_graph(rng, k, ncols, int(slots * 0.95))
    recs = [(key, (max(cv[0], 1),) + cv[1:], ed) for key, cv, ed in recs]  # every key loaded
    g = loaded_graph(mcx, k, ncols, recs, 1 << 14)
    assert g.nkmers >= 0.94 * slots  # (a table this full has sub-tables that spilled into the overflow area)
    body = pack(recs, k, ncols)
    for pop in (False, True):
        exp, nmod, _ = expect_file(recs, k, ncols, pop)
        got, n = g.infer_edges(body, pop=pop)
        assert got == pack(exp, k, ncols) and n == nmod
    sexp = {key: (cv, ed) for key, cv, ed in expect_stream(recs, k, ncols, False)[0]}
    m = merge(recs, ncols)
    gs = mcx.Graph(k, ncols, 1 << 14)
    gs.add_records(body, ncols, [(c, c) for c in range(ncols)])
    exported = gs.export(sorted_=True)
    got, _ = gs.infer_edges(exported, presence="covg")
    assert {key: (cv, ed) for key, cv, ed in parse(got, k, ncols)} == sexp and len(m) == len(sexp)
    # records already in HBM
    import torch
    exp, nmod, _ = expect_file(recs, k, ncols, False)
    d = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to("cuda:0")
    assert g.infer_edges_dev(d, len(recs)) == nmod
    assert d.cpu().numpy().tobytes() == pack(exp, k, ncols)
    # one chunk against 1000-record chunks over 200 K records
    big = (body * (200000 // len(recs) + 1))[:200000 * (8 + 5 * ncols)]
    one, n1 = g.infer_edges(big)
    os.environ["MCX_INFER_CHUNK"] = "1000"
    try:
        many, n2 = g.infer_edges(big)
    finally:
        del os.environ["MCX_INFER_CHUNK"]
    assert one == many and n1 == n2 > 0
    g.close(); gs.close()


@pytest.mark.gpu
def test_abi_refusals(built):
    import ctypes as C
    mcx = built
    from mccortex_amd.graph import McxError, _check, _ptr
    rng = random.Random(9)
    recs = random_graph(rng, 31, 2, 200)
    body = np.frombuffer(pack(recs, 31, 2), dtype=np.uint8).copy()
    g = mcx.Graph(31, 2, 1 << 12)
    n = C.c_uint64(0)
    with pytest.raises(McxError, match="colours"):
        _check(g.L.mcx_graph_infer_edges(g.h, _ptr(body), 1, 3, 0, C.byref(n)))
    with pytest.raises(McxError, match="flags"):
        _check(g.L.mcx_graph_infer_edges(g.h, _ptr(body), len(recs), 2, 4, C.byref(n)))
    g.close()
    gm = mcx.Graph(31, 2, 1 << 12, devices=[0, 0])
    with pytest.raises(McxError, match="split over devices"):
        gm.infer_edges(body.tobytes())
    gm.close()
    gi = mcx.Graph(31, 2, 1 << 12)
    gi.configure("intersect", 1)
    with pytest.raises(McxError, match="intersect"):
        gi.infer_edges(body.tobytes())
    gi.close()
