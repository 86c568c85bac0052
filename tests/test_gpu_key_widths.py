"""k = 65 .. 127 (three- and four-word keys) through the build features beside the plain insert: the duplicate filter
(`--remove-pcr`), `--intersect`, the ranged export whose prefix crosses a key word, arbitrary bytes / every path of the
front end, and the command line of mccortex95 / mccortex127.  Every comparison is byte for byte against the oracle.

The unmarked tests need no GPU: they show on the oracle alone that the inputs reach the states the device tests are
about (duplicates present, cutoffs effective, k-mers removed by the intersection, a found k-mer next to an absent one,
a prefix longer than the top key word, a range fuller than its arrays)."""
import ctypes as C
import functools

import numpy as np
import pytest

import synth
from oracle import ctxio
from test_cli import _write_inputs, run
from test_ctxio import _oracle_intersect
from test_gpu_fuzz import _gpu_stream, _oracle_body
from test_gpu_parity import _compare
from test_gpu_pcr import FIELDS, _dev_stats, _fuzz_bytes_lengths_and_cutoffs, _same_graph

gpu = pytest.mark.gpu


# ---- 1. the duplicate filter ------------------------------------------------------------------------------------
PCR_CASES = [(65, False, "FF", 1), (95, True, "FR", 3), (97, True, "RF", 2), (127, False, "RR", 2), (127, True, "FF", 1)]
PCR_N = 4000


def _pcr_batches(k, nbatches):
    bases, offs = synth.reads(PCR_N, 260, genome_len=1500, seed=k + nbatches, n_frac=0.02, lower_frac=0.1, var_len=(nbatches > 1))
    cuts = [2 * (PCR_N // 2 * i // nbatches) for i in range(nbatches + 1)]
    return bases, [offs[lo:hi + 1] for lo, hi in zip(cuts[:-1], cuts[1:])]


@functools.lru_cache(maxsize=None)
def _pcr_oracle(orc, k, paired, matedir, nbatches):
    bases, batches = _pcr_batches(k, nbatches)
    og, ot, odup = orc.Graph(k, 1, 1 << 16), orc.Stats(), [0, 0, 0]
    for o in batches:
        _, d = og.add_reads_pcr(0, bases, o, paired=paired, matedir=matedir, stats=ot)
        odup = [x + y for x, y in zip(odup, d)]
    return og, ot, odup


@pytest.mark.parametrize("k,paired,matedir,nbatches", PCR_CASES)
def test_pcr_inputs_hold_duplicates_and_reads_that_are_none(orc, k, paired, matedir, nbatches):
    _, ot, odup = _pcr_oracle(orc, k, paired, matedir, nbatches)
    assert odup[1 if paired else 0] > PCR_N // 20
    assert ot.num_good_reads > PCR_N // 20


@gpu
@pytest.mark.parametrize("k,paired,matedir,nbatches", PCR_CASES)
def test_pcr_filter_matches_walk_in_input_order(mcx, orc, k, paired, matedir, nbatches):
    og, ot, odup = _pcr_oracle(orc, k, paired, matedir, nbatches)
    bases, batches = _pcr_batches(k, nbatches)
    g = mcx.Graph(k, 1, 1 << 16)
    st = mcx.LoadStats()
    for o in batches:
        g.add_reads_pcr(0, bases, o, paired=paired, matedir=matedir, stats=st)
    _dev_stats(g, st)
    assert (st.num_dup_se_reads, st.num_dup_pe_pairs, st.num_pe_reads) == tuple(odup)
    assert {f: getattr(st, f) for f in FIELDS} == {f: getattr(ot, f) for f in FIELDS}
    _same_graph(mcx, g, og, k, 1)
    g.close()


# (k, share of the qualities at 70, -Q of mate 1, of mate 2, -H).  A k-mer of 95 bases under a cutoff needs 95 good
# qualities in a row: with one in ten drawn from 33 .. 73 a handful of k-mers survive (the filter then sees pairs
# without a start k-mer, which count as duplicates: build_graph.c:78-84); with one in a hundred most reads keep contigs.
PCR_QUAL_CASES = [(95, 0.9, 55, 64, 4), (95, 0.9, 0, 0, 3), (127, 0.9, 55, 64, 4), (127, 0.9, 0, 0, 3),
                  (95, 0.99, 55, 64, 4), (127, 0.99, 55, 64, 4), (95, 0.99, 0, 0, 5), (127, 0.99, 50, 60, 9)]


@functools.lru_cache(maxsize=None)
def _pcr_qual_input(share):
    bases, offs = synth.reads(PCR_N, 260, genome_len=1500, seed=5, n_frac=0.05)
    rng = np.random.default_rng(9)
    quals = rng.integers(33, 74, len(bases)).astype(np.uint8)
    quals[rng.random(len(bases)) < share] = 70
    # the reference compares `char` qualities as signed: a byte >= 128 is below every cutoff, like one below '!'
    quals[rng.integers(0, len(bases), 50)] = rng.integers(128, 256, 50).astype(np.uint8)
    quals[rng.integers(0, len(bases), 50)] = rng.integers(0, 33, 50).astype(np.uint8)
    return bases, offs, quals


@functools.lru_cache(maxsize=None)
def _pcr_qual_oracle(orc, k, share, fq1, fq2, hp):
    bases, offs, quals = _pcr_qual_input(share)
    og, ot = orc.Graph(k, 1, 1 << 16), orc.Stats()
    _, d = og.add_reads_pcr(0, bases, offs, quals=quals, fq_cutoff=fq1, fq_cutoff2=fq2, hp_cutoff=hp, paired=True, matedir="FR", stats=ot)
    return og, ot, d


@pytest.mark.parametrize("k,share,fq1,fq2,hp", PCR_QUAL_CASES)
def test_pcr_quality_cutoffs_change_what_is_loaded(orc, k, share, fq1, fq2, hp):
    _, ot, d = _pcr_qual_oracle(orc, k, share, fq1, fq2, hp)
    _, plain, d0 = _pcr_qual_oracle(orc, k, share, 0, 0, 0)
    assert ot.num_kmers_loaded != plain.num_kmers_loaded and d[1] > 0 and d0[1] > 0
    if share > 0.95:
        assert ot.num_kmers_loaded > 10000 and d[1] < PCR_N // 2 - 100   # pairs that are loaded, pairs that are filtered


@gpu
@pytest.mark.parametrize("k,share,fq1,fq2,hp", PCR_QUAL_CASES)
def test_pcr_filter_with_quality_and_homopolymer_cutoffs(mcx, orc, k, share, fq1, fq2, hp):
    """the start k-mer is the one seq_contig_start finds under -Q / -H; mates carry their own cutoff; qualities are
    signed bytes"""
    og, ot, d = _pcr_qual_oracle(orc, k, share, fq1, fq2, hp)
    bases, offs, quals = _pcr_qual_input(share)
    g = mcx.Graph(k, 1, 1 << 16)
    st = mcx.LoadStats()
    g.add_reads_pcr(0, bases, offs, quals=quals, fq_cutoff=fq1, fq_cutoff2=fq2, hp_cutoff=hp, paired=True, matedir="FR", stats=st)
    _dev_stats(g, st)
    assert (st.num_dup_se_reads, st.num_dup_pe_pairs, st.num_pe_reads) == tuple(d)
    assert {f: getattr(st, f) for f in FIELDS} == {f: getattr(ot, f) for f in FIELDS}
    _same_graph(mcx, g, og, k, 1)
    g.close()


@gpu
@pytest.mark.parametrize("seed", range(4))
def test_pcr_fuzz_arbitrary_bytes_lengths_and_cutoffs(mcx, orc, seed):
    _fuzz_bytes_lengths_and_cutoffs(mcx, orc, 400 + seed, [65, 95, 97, 127])


# A quality byte >= 128 is a negative `char`: seq_contig_end2 (seq_reader.c:148-149) ends a contig at `qual < cutoff`
# even when the cutoff is 0.  The case (95, 0.99, 0, 0, 5) above found that the library dropped the qualities of a
# batch without a cutoff; these go through every entry that takes qualities, at one- and three-word keys.
@pytest.mark.parametrize("k", [31, 95])
def test_quality_bytes_with_the_top_bit_matter_without_a_cutoff(orc, k):
    bases, offs, quals = _pcr_qual_input(0.99)
    with_q = orc.Graph(k, 1, 1 << 16).add_reads(0, bases, offs, quals=quals)
    without = orc.Graph(k, 1, 1 << 16).add_reads(0, bases, offs)
    assert with_q.num_kmers_loaded < without.num_kmers_loaded and with_q.contigs_parsed > without.contigs_parsed
    assert (quals >= 128).sum() >= 40


@gpu
@pytest.mark.parametrize("k", [31, 95])
def test_quality_bytes_with_the_top_bit_end_a_contig_without_a_cutoff(mcx, orc, k):
    bases, offs, quals = _pcr_qual_input(0.99)
    for hp in (0, 5):
        _compare(mcx, orc, k, 1, [(0, bases, offs, quals)], cap=1 << 16, hp_cutoff=hp)
    # the must-exist walk: the graph of the reads without qualities, the same reads again with them
    og, g = orc.Graph(k, 1, 1 << 16), mcx.Graph(k, 2, 1 << 16)
    og.add_reads(0, bases, offs)
    body = og.body_bytes(True)
    rs = 8 * og.W + 5
    rec = np.frombuffer(body, np.uint8).reshape(-1, rs)
    keys = rec[:, :8 * og.W].copy().view("<u8").reshape(-1, og.W)
    covgs = rec[:, 8 * og.W:8 * og.W + 4].copy().view("<u4").reshape(-1)
    og = orc.Graph(k, 1, 1 << 16)
    for i in range(len(keys)):
        og.add_isec_record(keys[i], int(covgs[i]), int(rec[i, -1]))
    og.set_must_exist(True)
    ost = og.add_reads(0, bases, offs, quals=quals)
    og.isec_finish()
    g.configure("intersect", 1)
    g.add_records(body, 1, [(0, 1)])
    g.configure("must_exist", 1)
    g.add_reads(0, bases, offs, quals=quals)
    g.intersect_finish()
    assert g.device_stats().num_kmers_loaded == ost.num_kmers_loaded
    assert g.export(True) == og.body_bytes(True)
    g.close()


# ---- 2. --intersect ---------------------------------------------------------------------------------------------
ISEC_KS = [65, 95, 127]
ISEC_FQ = 43


def _key_ints(keys):
    W = keys.shape[1]
    return [sum(int(w) << (64 * (W - 1 - i)) for i, w in enumerate(row)) for row in keys]


def _found_absent_neighbours(orc, k, present, bases, offs, quals, fq):
    """consecutive k-mers of one contig of which exactly one is in `present` (canonical k-mers as integers): where
    build_graph_from_str_mt's "edge only when BOTH were found" decides"""
    L = orc.lib()
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    pairs = 0
    for r in range(len(offs) - 1):
        seq = bytes(bases[int(offs[r]):int(offs[r + 1])])
        q = bytes(quals[int(offs[r]):int(offs[r + 1])])
        search = C.c_size_t(0)
        while True:
            cs = L.orc_contig_start(seq, len(seq), q, len(q), search.value, k, fq, 0)
            if cs >= len(seq):
                break
            ce = L.orc_contig_end(seq, len(seq), q, len(q), cs, k, fq, 0, C.byref(search))
            fw = rc = 0
            prev = None
            for i in range(cs, ce):
                nuc = ((seq[i] >> 1) ^ (seq[i] >> 2)) & 3
                fw = ((fw << 2) | nuc) & mask
                rc = (rc >> 2) | ((3 - nuc) << top)
                if i + 1 < cs + k:
                    continue
                found = min(fw, rc) in present
                pairs += prev is not None and prev != found
                prev = found
    return pairs


@functools.lru_cache(maxsize=None)
def _isec_input(orc, k):
    g0 = synth.genome(20000, 31)
    ra = synth.reads(700, 300, seed=1, g=g0)
    rq = synth.reads(600, 320, seed=3, g=g0, n_frac=0.01, lower_frac=0.1, err=0.002)
    rng = np.random.default_rng(5)
    quals = rng.integers(33, 74, len(rq[0])).astype(np.uint8)
    quals[rng.random(len(quals)) < 0.97] = 70
    oi = orc.Graph(k, 1, 1 << 20)
    oi.add_reads(0, *ra)
    isec = oi.ctx_bytes(True)
    hdr, hs = ctxio.read_header(isec)
    keys, covgs, edges = ctxio.records(isec, hdr, hs)
    return keys, covgs, edges, isec[hs:], rq, quals


@functools.lru_cache(maxsize=None)
def _isec_case(orc, k, fq=ISEC_FQ):
    keys, covgs, edges, body, rq, quals = _isec_input(orc, k)
    og = orc.Graph(k, 1, 1 << 20)
    for i in range(len(keys)):
        og.add_isec_record(keys[i], int(covgs[i, 0]), int(edges[i, 0]))
    before = og.nkmers
    og.set_must_exist(True)
    ost = og.add_reads(0, *rq, quals=quals, fq_cutoff=fq, hp_cutoff=0)
    og.isec_finish()
    return dict(rq=rq, quals=quals, body=body, keys=keys, og=og, ost=ost, before=before)


@pytest.mark.parametrize("k", ISEC_KS)
def test_intersect_inputs_reach_cutoff_removal_and_found_next_to_absent(orc, k):
    c = _isec_case(orc, k)
    plain = orc.Graph(k, 1, 1 << 20).add_reads(0, *c["rq"]).num_kmers_loaded
    nocut = _isec_case(orc, k, 0)
    assert 0 < c["ost"].num_kmers_loaded < nocut["ost"].num_kmers_loaded <= plain     # the cutoff matters
    assert c["og"].nkmers < nocut["og"].nkmers
    assert 0 < c["og"].nkmers < c["before"] == len(c["keys"])            # the finish removes k-mers
    assert _found_absent_neighbours(orc, k, set(_key_ints(c["keys"])), *c["rq"], c["quals"], ISEC_FQ) > 0


@gpu
@pytest.mark.parametrize("k", ISEC_KS)
def test_intersect_reads_with_quality_cutoff(mcx, orc, k):
    """ctx_build.c:341-413 through the library calls the build command makes, then the scans over the tombstones the
    finish wrote"""
    c = _isec_case(orc, k)
    og = c["og"]
    g = mcx.Graph(k, 2, 1 << 20, device=0)              # colour 1: the hidden holder of the intersection's edges
    g.configure("intersect", 1)
    g.add_records(c["body"], 1, [(0, 1)])
    g.configure("must_exist", 1)
    g.add_reads(0, *c["rq"], quals=c["quals"], fq_cutoff=ISEC_FQ, hp_cutoff=0)
    g.intersect_finish()
    assert 0 < og.nkmers == g.nkmers
    assert g.device_stats().num_kmers_loaded == c["ost"].num_kmers_loaded
    body = g.export(True)
    assert body == og.body_bytes(True)
    rs = 8 * g.W + 5
    cov = np.frombuffer(body, np.uint8).reshape(-1, rs)[:, 8 * g.W:8 * g.W + 4].copy().view("<u4").reshape(-1).astype(np.uint64)
    nk, sc = g.kmer_covg()
    assert (int(nk[0]), int(sc[0])) == (int((cov > 0).sum()), int(cov.sum()))
    assert g.covg_histogram(16).tolist() == np.bincount(np.minimum(cov, 15).astype(np.int64), minlength=16).tolist()
    g.close()


def _ctx_file(path, og):
    path.write_bytes(og.ctx_bytes(True))
    return str(path)


def _reads_ctx(orc, path, k, name, bases, offs):
    og = orc.Graph(k, 1, 1 << 20)
    og.set_sample(0, name)
    og.update_stats(0, og.add_reads(0, bases, offs))
    return _ctx_file(path, og)


@gpu
def test_intersect_two_graphs_two_colours_k95(mcx, orc, tmp_path):
    """two --intersect graphs, a --graph that only partly overlaps them, reads with errors, N and lower case"""
    k = 95
    g0, g1 = synth.genome(20000, 31), synth.genome(20000, 32)
    both = np.concatenate([g0[:12000], g1[:8000]])
    ra = synth.reads(700, 300, seed=1, g=both)
    rb = synth.reads(700, 300, seed=2, g=np.concatenate([g0[4000:16000], g1[2000:10000]]))
    rq = synth.reads(500, 320, seed=3, g=both, n_frac=0.05, lower_frac=0.1)
    rg = synth.reads(400, 280, seed=4, g=np.concatenate([g1[:5000], g0[5000:9000]]))
    I0 = _reads_ctx(orc, tmp_path / "I0.ctx", k, "a", *ra)
    I1 = _reads_ctx(orc, tmp_path / "I1.ctx", k, "b", *rb)
    G = _reads_ctx(orc, tmp_path / "G.ctx", k, "g", *rg)
    fq, fa = _write_inputs(tmp_path, *rq, "q", "fa"), _write_inputs(tmp_path, *ra, "a", "fa")
    out = str(tmp_path / "o.ctx")
    rc, _, err = run(95, "build", "-q", "-k", str(k), "-n", "1M", "--sort", "-I", I0, "-I", I1, "-g", G, "-s", "q", "--seq", fq, "--seq", fa, out)
    assert rc == 0, err
    rd = lambda p: open(p, "rb").read()
    want, og = _oracle_intersect(orc, k, 2, [rd(I0), rd(I1)], [(rd(G), G, 0)], {1: "q"}, [(1, *rq), (1, *ra)])
    hdr, hs = ctxio.read_header(want)
    _, covgs, _ = ctxio.records(want, hdr, hs)
    assert (covgs[:, 0] > 0).sum() > 100 and (covgs[:, 1] > 0).sum() > 1000    # either colour keeps k-mers
    assert rd(out) == want


# ---- 4. ranged export where the prefix crosses a key word ----------------------------------------------------------
RANGED_CASES = [(33, 1), (65, 2), (97, 1), (127, 1)]


def _export_scratch(nk):
    """what the device test lets the export take: the fixed part and room for about an eighth of the k-mers"""
    return 3 * (64 << 20) + nk * 72 // 8


@functools.lru_cache(maxsize=None)
def _ranged_case(orc, k, ncols):
    rng = np.random.default_rng(k)
    g0 = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, 400_000, p=[0.45, 0.05, 0.05, 0.45])]  # AT-rich
    bases, offs = synth.reads(6000, 150, seed=k, g=g0, n_frac=0.02) if k < 64 else synth.reads(3000, 300, seed=k, g=g0, n_frac=0.02)
    jobs = [(0, bases, offs)] + [(c, bases[:int(offs[1000])], offs[:1001]) for c in range(1, ncols)]
    og = orc.Graph(k, ncols, 1 << 21)
    for col, b, o in jobs:
        og.add_reads(col, b, o)
    return jobs, og.body_bytes(True)


def _export_plan(k, ncols, nk, avail):
    """export_t's size rule (mcx_api.hip): -> (bits of the first prefix, capacity of the arrays at `bits` bits)"""
    W = (2 * k + 63) // 64
    recsz = 8 * W + 5 * ncols
    chunk = max(1, (64 << 20) // recsz)
    per_kmer = 8 * W + 8 + 32 + (8 if W >= 2 else 0) + 8
    fixed = 2 * chunk * recsz + (64 << 20)
    pbits = 0
    while pbits < 16 and pbits + 2 <= 2 * k and (nk >> pbits) * per_kmer * 5 // 4 + fixed > avail:
        pbits += 1
    assert (nk >> pbits) * per_kmer * 5 // 4 + fixed <= avail
    return pbits, lambda bits: nk if bits == 0 else min(nk, (nk >> bits) * 5 // 4 + 65536)


@pytest.mark.parametrize("k,ncols", RANGED_CASES)
def test_ranged_export_inputs_cross_the_key_word_and_overfill_a_range(orc, k, ncols):
    _, want = _ranged_case(orc, k, ncols)
    W = (2 * k + 63) // 64
    rs = 8 * W + 5 * ncols
    nk = len(want) // rs
    assert 200_000 <= nk <= 400_000
    tops = [v >> (2 * k - 32) for v in _key_ints(np.frombuffer(want, np.uint8).reshape(-1, rs)[:, :8 * W].copy().view("<u8").reshape(-1, W))]
    tops = np.array(tops, dtype=np.int64)                    # the top 32 bits of every 2k-bit key
    pbits, cap = _export_plan(k, ncols, nk, _export_scratch(nk))
    nb0 = 2 * k - 64 * (W - 1)                               # key bits in the top word
    assert pbits == 4 and (pbits > nb0) == (k != 127) and nb0 == (62 if k == 127 else 2)
    count = lambda prefix, bits: int(((tops >> (32 - bits)) == prefix).sum())
    assert max(count(p, pbits) for p in range(1 << pbits)) > 1.1 * cap(pbits)
    # the export's walk: a range fuller than its arrays is split in two
    todo, done = [(p, pbits) for p in range(1 << pbits)], []
    while todo:
        prefix, bits = todo.pop()
        if count(prefix, bits) > cap(bits):
            todo += [(2 * prefix + 1, bits + 1), (2 * prefix, bits + 1)]
        else:
            done.append((prefix, bits))
    assert sum(count(p, b) for p, b in done) == nk
    assert {b for _, b in done} == {pbits, pbits + 1}


@gpu
@pytest.mark.parametrize("k,ncols", RANGED_CASES)
def test_export_in_key_ranges_across_the_key_word(mcx, orc, k, ncols, monkeypatch):
    """k = 33, 65, 97 keep 2 bits of the key in the top word: a 4-bit (after a split 5-bit) prefix takes the rest from
    the next word -- k_compact's two-word branch.  k = 127 (62 bits on top) is the one-word control with a four-word
    sort behind it."""
    jobs, want = _ranged_case(orc, k, ncols)
    g = mcx.Graph(k, ncols, 1 << 21)
    for col, b, o in jobs:
        g.add_reads(col, b, o)
    assert g.export(True) == want
    rs = 8 * g.W + 5 * ncols
    monkeypatch.setenv("MCX_EXPORT_SCRATCH", str(_export_scratch(len(want) // rs)))
    assert g.export(True) == want
    a = np.frombuffer(g.export(False), np.uint8).reshape(-1, rs)
    b = np.frombuffer(want, np.uint8).reshape(-1, rs)
    assert sorted(map(bytes, a)) == sorted(map(bytes, b))
    monkeypatch.setenv("MCX_EXPORT_SCRATCH", str(1 << 20))
    with pytest.raises(mcx.McxError):
        g.export(True)
    g.close()


# ---- 5. arbitrary bytes, hot keys and -Q / -H through k_stream<3> / k_stream<4> ------------------------------------
# The alphabet of test_arbitrary_bytes_and_ragged_lengths has one byte in five that is no base: a run of 65 bases or
# more hardly ever occurs (the lengths and seams are still walked, with nothing to insert).  "dense" keeps the same
# special bytes among ten times as many bases, a tenth of them lower case: about one position in four starts a 127-mer.
@gpu
@pytest.mark.parametrize("mix", ["sparse", "dense"])
@pytest.mark.parametrize("seed", range(3))
def test_arbitrary_bytes_and_ragged_lengths_wide(mcx, orc, seed, mix):
    """the ASCII device stream and the packed host entry are different instances of the kernel: both, on the same bytes"""
    rng = np.random.default_rng(700 + seed)
    letters = b"ACGT" * 40 if mix == "sparse" else b"ACGT" * 400 + b"acgt" * 40
    alphabet = np.concatenate([np.frombuffer(letters + b"acgtNn\n\r\t @+>", np.uint8), rng.integers(0, 256, 30 if mix == "sparse" else 8).astype(np.uint8)])
    loaded = 0
    for n in (0, 1, 30, 31, 32, 4095, 4096, 4097, 4096 + 15, 8192 + 33, 50001):
        s = bytes(rng.choice(alphabet, n)) if n else b""
        bases, offs = orc.pack_reads(s.split(b"\n"))
        for k in (65, 95, 97, 127):
            og, st, want = _oracle_body(orc, k, s, 1 << 17)
            loaded += st.num_kmers_loaded if k == 127 else 0
            g = _gpu_stream(mcx, k, s, 0, 1 << 17)
            assert g.export(True) == want, (n, k)
            assert g.device_stats().num_kmers_loaded == st.num_kmers_loaded
            g.close()
            g = mcx.Graph(k, 1, 1 << 17)
            g.add_reads(0, bases, offs)
            g.sync()
            assert g.export(True) == want, (n, k, "packed")
            assert g.device_stats().num_kmers_loaded == st.num_kmers_loaded
            g.close()
    assert mix == "sparse" or loaded > 10000


@gpu
@pytest.mark.parametrize("k", list(range(65, 128, 2)))
def test_every_odd_wide_k_on_long_contigs(mcx, orc, k):
    """test_every_odd_k's 6000-byte stream breaks every 9 bases: at k > 63 it holds next to no k-mer.  The same walk
    over a stream that breaks every 110 bases, a tenth of it lower case."""
    rng = np.random.default_rng(k)
    s = bytes(rng.choice(np.frombuffer(b"ACGT" * 50 + b"acgt" * 5 + b"N\n", np.uint8), 6000))
    og, st, want = _oracle_body(orc, k, s, 1 << 16)
    assert st.num_kmers_loaded > 500
    g = _gpu_stream(mcx, k, s, 0, 1 << 16)
    assert g.export(True) == want
    d = g.device_stats()
    assert (d.num_kmers_loaded, d.contigs_parsed, d.total_bases_loaded) == (st.num_kmers_loaded, st.contigs_parsed, st.total_bases_loaded)
    g.close()


@gpu
@pytest.mark.parametrize("k", [95, 127])
def test_hot_keys_contention_wide(mcx, orc, k):
    reads = ["A" * 300] * 3000 + ["AC" * 150] * 2000 + ["T" * 400] * 500
    og = _compare(mcx, orc, k, 1, [(0, *orc.pack_reads(reads))])
    assert og.nkmers == 3          # poly-A (= poly-T), ACAC..A and CACA..C (k is odd: neither is the other's reverse complement)
    assert og.lookup("A" * k)[0][0] == 3000 * (301 - k) + 500 * (401 - k)


@functools.lru_cache(maxsize=None)
def _qh_input():
    bases, offs = synth.reads(600, 260, genome_len=15000, seed=12, n_frac=0.02)
    rng = np.random.default_rng(3)
    quals = rng.integers(33, 74, len(bases)).astype(np.uint8)
    quals[rng.random(len(bases)) < 0.97] = 70        # (uniform qualities leave no run of k good ones at all)
    s = int(offs[4]) + 50
    bases[s:s + 150] = ord("A")                       # a homopolymer run longer than k inside read 4
    return bases, offs, quals


@gpu
@pytest.mark.parametrize("k", [97, 127])
def test_quality_and_homopolymer_cutoffs_wide(mcx, orc, k):
    bases, offs, quals = _qh_input()
    sizes = [_compare(mcx, orc, k, 1, [(0, bases, offs, quals)], fq_cutoff=fq, hp_cutoff=hc).nkmers for fq, hc in ((0, 0), (40, 0), (0, 6), (38, 9))]
    assert min(sizes) > 1000 and len(set(sizes)) == 4      # every cutoff still loads k-mers, and each changes the graph


# ---- 6. the command line of the wide binaries ---------------------------------------------------------------------
@gpu
def test_cli_mccortex127_remove_pcr_pairs_k97(mcx, orc, tmp_path):
    k, n = 97, 1000
    g0 = synth.genome(600, 5)
    b1, o1 = synth.reads(n, 260, seed=1, g=g0, n_frac=0.05)
    b2, o2 = synth.reads(n, 260, seed=2, g=g0, n_frac=0.05, lower_frac=0.2)
    f1, f2 = _write_inputs(tmp_path, b1, o1, "m1", "fq"), _write_inputs(tmp_path, b2, o2, "m2", "fa", gz=True)
    out = str(tmp_path / "pcr.ctx")
    rc, _, err = run(127, "build", "-k", str(k), "-n", "64K", "--sort", "-H", "9", "--sample", "w", "--remove-pcr", "--matepair", "RF",
                     "--seq2", f1 + ":" + f2, out)
    assert rc == 0, err
    bp, op = orc.pack_reads([r for i in range(n) for r in (bytes(b1[int(o1[i]):int(o1[i + 1])]), bytes(b2[int(o2[i]):int(o2[i + 1])]))])
    og = orc.Graph(k, 1, 1 << 16)
    og.set_sample(0, "w")
    st, d = og.add_reads_pcr(0, bp, op, hp_cutoff=9, paired=True, matedir="RF")
    og.update_stats(0, st)
    assert n // 20 < d[1] < n - n // 20
    assert "dup SE reads: 0  dup PE pairs: %s" % format(d[1], ",") in err
    assert open(out, "rb").read() == og.ctx_bytes(True)


@gpu
def test_cli_mccortex95_intersect_k65(mcx, orc, tmp_path):
    k = 65
    g0 = synth.genome(20000, 31)
    ra = synth.reads(700, 300, seed=1, g=g0)
    rq = synth.reads(2000, 150, seed=3, g=g0, n_frac=0.02, lower_frac=0.1, err=0.002)
    isec = _reads_ctx(orc, tmp_path / "isec.ctx", k, "ref", *ra)
    out = str(tmp_path / "o.ctx")
    rc, _, err = run(95, "build", "-q", "-k", str(k), "-n", "1M", "--sort", "--intersect", isec, "-s", "q", "--seq", _write_inputs(tmp_path, *rq, "q", "fa"), out)
    assert rc == 0, err
    want, og = _oracle_intersect(orc, k, 1, [open(isec, "rb").read()], [], {0: "q"}, [(0, *rq)])
    assert 1000 < og.nkmers
    assert open(out, "rb").read() == want
