"""The rare states of the table, reached on purpose: keys in the overflow area, value words whose 56-bit count has
passed 2^32 - 1, tombstoned slots, record chunks after the first -- and the kernels that must read them correctly
(the scans behind the full-size checks, the record loader's indices, the sortedness check of `index`).

Everything is compared bit for bit with the oracle (oracle/orc.py) or with a numpy / Python-int restatement in this
file.  A spill into the overflow area is proven by arithmetic: the table has `nmain` hash-addressed slots, so a
graph of more than `nmain` k-mers has keys in the area.  The tests that are not marked `gpu` check, on the
references alone, that the inputs reach the states the device tests are about.

The record loader's chunks depend on MCX_STAGE_BYTES, which is read once per process: that part runs in a child
process (this file, run as a script) and hands its results back as JSON."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clean_restate as R  # noqa: E402

U32 = 0xFFFFFFFF
CAP = 1 << 14  # requested capacity of the tables whose geometry the tests rely on


# ---- geometry and records ------------------------------------------------------------------------
def words(k):
    return (2 * k + 63) // 64


def geometry(k, cap=CAP):
    """(nmain, novf) of mcx_graph_create_shard on one device: sub-tables of 4096 (one key word) or 2048 slots in
    2^lb1 regions, and behind them an overflow area of 1 / 32 of the table, at least one sub-table"""
    ss = 4096 if words(k) == 1 else 2048
    nsub = -(-max(cap, 1024) // ss)
    lb1 = 0
    while lb1 < 9 and (2 << lb1) <= nsub:
        lb1 += 1
    while lb1 < 11 and -(-nsub // (1 << lb1)) > 2048:
        lb1 += 1
    nmain = (-(-nsub // (1 << lb1)) << lb1) * ss
    return nmain, max(ss, -(-(nmain // 32) // ss) * ss)


def check_geometry(g, k):
    """a later change of geometry fails here instead of silently no longer spilling"""
    nmain, novf = geometry(k)
    assert g.capacity()[0] == nmain + novf
    return nmain, novf


def random_keys(rng, k, n):
    """n uniform keys below 2^(2k), most significant word first"""
    W = words(k)
    keys = rng.integers(0, 1 << 64, (n, W), dtype=np.uint64)
    keys[:, 0] >>= np.uint64(64 * W - 2 * k)
    return keys


def pack_records(keys, cov, edg):
    n = len(keys)
    return np.concatenate([np.ascontiguousarray(keys, "<u8").view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(cov, "<u4").view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(edg, np.uint8).reshape(n, -1)], axis=1).tobytes()


def parse_records(body, W, ncols):
    rec = np.frombuffer(body, np.uint8).reshape(-1, 8 * W + 5 * ncols)
    keys = rec[:, :8 * W].copy().view("<u8").reshape(-1, W)
    cov = rec[:, 8 * W:8 * W + 4 * ncols].copy().view("<u4").reshape(-1, ncols)
    return keys, cov, rec[:, 8 * W + 4 * ncols:].copy()


def identity(ncols):
    return [(c, c) for c in range(ncols)]


def orc_add_records(og, keys, cov, edg, must_exist=False):
    """graph_load's per-record body over the records, in order -> number of records loaded"""
    return sum(og.add_record(keys[i], cov[i], edg[i], must_exist) == 1 for i in range(len(keys)))


def scan_expect(cov, nbins):
    """db_graph_get_kmer_covg and the coverage histogram over per-colour coverages (n x ncols, already <= 2^32 - 1)"""
    cov = cov.astype(np.uint64)
    tot = np.minimum(cov.sum(axis=1), U32)  # db_node_sum_covg saturates
    return (cov > 0).sum(axis=0).tolist(), cov.sum(axis=0).tolist(), \
        np.bincount(np.minimum(tot, nbins - 1).astype(np.int64), minlength=nbins).tolist()


def check_scans(mcx, g, k, ncols, body, nbins_list, cov=None):
    """checksum, kmer_covg and covg_histogram of the table against the expected records (`ncols` visible colours)"""
    W = words(k)
    cs, n = g.checksum()
    assert n == g.nkmers == len(body) // (8 * W + 5 * ncols)
    assert cs == mcx.records_checksum(body, k, ncols)
    if cov is None:
        cov = parse_records(body, W, ncols)[1]
    nk, sc = g.kmer_covg()
    want_nk, want_sc, _ = scan_expect(cov, 2)
    assert nk[:ncols].tolist() == want_nk and sc[:ncols].tolist() == want_sc
    for nbins in nbins_list:
        assert g.covg_histogram(nbins).tolist() == scan_expect(cov, nbins)[2], nbins


def test_geometry_of_the_small_tables():
    assert geometry(31) == (16384, 4096)
    assert geometry(63) == geometry(95) == geometry(127) == (16384, 2048)


# ---- A. the overflow area, over the path x key-width x colour matrix --------------------------------
A_READS = [("deferred", k, c) for k in (31, 63) for c in (1, 2)] + [("direct", k, c) for k in (31, 63, 95, 127) for c in (1, 2)]
A_RECORDS = [(k, c) for k in (31, 63, 95, 127) for c in (1, 3)]
A_REFS = sorted({("reads", k, c) for _, k, c in A_READS}) + [("records", k, c) for k, c in A_RECORDS]
_A = {}


def a_case(orc, kind, k, ncols):
    """the input of one case and the oracle's records after each step: load, load again, must-exist pass.
    nmain + novf / 2 distinct k-mers: every sub-table fills up and the overflow area ends half full."""
    if (kind, k, ncols) in _A:
        return _A[kind, k, ncols]
    from test_gpu_parity import _distinct_kmer_reads
    W = words(k)
    nmain, novf = geometry(k)
    N = nmain + novf // 2
    rng = np.random.default_rng(1000 * k + ncols)
    og = orc.Graph(k, ncols, 1 << 16)
    if kind == "reads":  # colour 0 takes all reads, colour 1 the first half
        bases, offs = _distinct_kmer_reads(N, k, seed=k)
        half = (len(offs) - 1) // 2
        inp = [(0, bases, offs)] + ([(1, bases[:int(offs[half])], offs[:half + 1])] if ncols > 1 else [])

        def load():
            for c, b, o in inp:
                og.add_reads(c, b, o)
    else:  # distinct keys, then the first third again: coverage sums, edges OR
        keys = np.unique(random_keys(rng, k, N), axis=0)
        n = len(keys)
        keys = keys[rng.permutation(n)]
        keys = np.concatenate([keys, keys[:n // 3]])
        cov = (rng.integers(0, 3, (len(keys), ncols)) * rng.integers(1, 50, (len(keys), ncols))).astype(np.uint32)
        cov[:n, 0] = rng.integers(1, 50, n)  # (the first record of every key is loaded; some repeats are all zero: skipped)
        edg = rng.integers(0, 256, (len(keys), ncols), dtype=np.uint8)
        edg[cov == 0] = 0
        inp = (keys, cov, edg)

        def load():
            orc_add_records(og, keys, cov, edg)
    load()
    nk, body1 = og.nkmers, og.body_bytes(True)
    load()
    assert og.nkmers == nk
    body2 = og.body_bytes(True)
    # the must-exist pass: every record of the graph and 500 keys that are not in it, shuffled
    kk, cc, ee = parse_records(body2, W, ncols)
    absent = random_keys(rng, k, 500)
    present = {row.tobytes() for row in kk}
    assert not any(row.tobytes() in present for row in absent)
    mk = np.concatenate([kk, absent])
    mc = np.concatenate([cc, rng.integers(1, 9, (500, ncols)).astype(np.uint32)])
    me = np.concatenate([ee, rng.integers(0, 256, (500, ncols), dtype=np.uint8)])
    p = rng.permutation(len(mk))
    mk, mc, me = mk[p], mc[p], me[p]
    loaded = orc_add_records(og, mk, mc, me, must_exist=True)
    assert og.nkmers == nk and loaded == int((cc.astype(np.uint64).sum(axis=1) > 0).sum())
    _A[kind, k, ncols] = dict(inp=inp, nk=nk, body1=body1, body2=body2, must=pack_records(mk, mc, me), nmust=len(mk),
                              loaded=loaded, body3=og.body_bytes(True))
    return _A[kind, k, ncols]


@pytest.mark.parametrize("kind,k,ncols", A_REFS)
def test_overflow_inputs_exceed_the_hash_addressed_slots(orc, kind, k, ncols):
    """a condition on the reference alone: more k-mers than `nmain`, and the overflow area between 1/4 and 3/4 full"""
    nmain, novf = geometry(k)
    assert nmain + novf // 4 <= a_case(orc, kind, k, ncols)["nk"] <= nmain + 3 * novf // 4


def a_run(mcx, orc, kind, k, ncols, defer=None):
    ref = a_case(orc, kind, k, ncols)
    g = mcx.Graph(k, ncols, CAP)
    nmain, _ = check_geometry(g, k)
    if defer is not None:
        g.configure("defer", defer)

    def load():
        if kind == "reads":
            for c, b, o in ref["inp"]:
                g.add_reads(c, b, o)
            g.sync()
            return None
        return g.add_records(pack_records(*ref["inp"]), ncols, identity(ncols))

    st = load()
    assert g.nkmers == ref["nk"] > nmain  # the spill, by arithmetic
    if st is not None:  # (some of the repeated records have no coverage at all: skipped, and the first is reported)
        cov = ref["inp"][1]
        assert (st.nkmers_novel, st.nkmers_loaded) == (ref["nk"], int((cov.sum(axis=1) > 0).sum()))
        assert (st.first_zero_covg, st.first_edges_no_covg) == (int(np.nonzero((cov == 0).all(axis=1))[0][0]), -1)
    assert g.export(True) == ref["body1"]
    st = load()  # every key is found again, in its sub-table or in the area: coverage doubles
    assert g.nkmers == ref["nk"] and (st is None or st.nkmers_novel == 0)
    assert g.export(True) == ref["body2"]
    st = g.add_records(ref["must"], ncols, identity(ncols), must_exist=True)
    assert (st.nkmers_read, st.nkmers_loaded, st.nkmers_novel) == (ref["nmust"], ref["loaded"], 0)
    assert g.nkmers == ref["nk"]
    assert g.export(True) == ref["body3"]
    check_scans(mcx, g, k, ncols, ref["body3"], (2, 64, 5000))
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path,k,ncols", A_READS)
def test_overflow_area_from_reads(mcx, orc, path, k, ncols):
    a_run(mcx, orc, "reads", k, ncols, defer=1 if path == "deferred" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k,ncols", A_RECORDS)
def test_overflow_area_from_records(mcx, orc, k, ncols):
    a_run(mcx, orc, "records", k, ncols)


# ---- B. saturation and the high histogram bins in the scans ---------------------------------------
B_CASES = [(31, 1), (31, 3), (63, 2), (95, 1), (127, 3)]  # S == 2 fast path, the general path, every W
B_NBINS = (2, 4096, 4097, 5000, 6000)
_B = {}


def b_case(orc, k, ncols):
    """records whose coverages straddle the 4096 LDS bins, the last bin of a 5000-bin histogram and 2^32 - 1;
    -> (record bytes, per-colour raw sums, the oracle's records) with one row of sums per node, in key order"""
    if (k, ncols) in _B:
        return _B[k, ncols]
    rng = np.random.default_rng(2000 + 10 * k + ncols)
    base = np.unique(random_keys(rng, k, 6000), axis=0)
    base = base[rng.permutation(len(base))]
    keys = np.concatenate([base, base[:3000]])
    shape = (len(keys), ncols)
    cls = rng.choice(5, shape, p=[0.25, 0.4, 0.2, 0.08, 0.07])
    cov = np.select([cls == 0, cls == 1, cls == 2, cls == 3], [0, rng.integers(1, 41, shape), rng.integers(4000, 5201, shape),
                                                               (1 << 31) + rng.integers(0, 1000, shape)], U32).astype(np.uint32)
    edg = rng.integers(0, 256, shape, dtype=np.uint8)
    edg[cov == 0] = 0
    # the restatement: records whose loaded colours are all zero are skipped; a node's count is the sum of its records
    loaded = cov.astype(np.uint64).sum(axis=1) > 0
    uk, gid = np.unique(keys, axis=0, return_inverse=True)
    gid = np.asarray(gid).ravel()
    raw = np.zeros((len(uk), ncols), dtype=np.uint64)
    np.add.at(raw, gid[loaded], cov[loaded].astype(np.uint64))
    present = np.zeros(len(uk), dtype=bool)
    present[gid[loaded]] = True
    og = orc.Graph(k, ncols, 1 << 16)
    orc_add_records(og, keys, cov, edg)
    _B[k, ncols] = (pack_records(keys, cov, edg), uk[present], raw[present], og.body_bytes(True))
    return _B[k, ncols]


@pytest.mark.parametrize("k,ncols", B_CASES)
def test_saturation_inputs_reach_the_clamp_and_the_high_bins(orc, k, ncols):
    _, uk, raw, body = b_case(orc, k, ncols)
    value = np.minimum(raw, U32)
    okeys, ocov, _ = parse_records(body, words(k), ncols)
    assert np.array_equal(okeys, uk) and np.array_equal(ocov.astype(np.uint64), value)  # the two references agree
    assert int((raw > U32).any(axis=1).sum()) >= 50
    tot = np.minimum(value.sum(axis=1), U32)
    for nbins in (5000, 6000):
        assert int(((tot >= 4096) & (tot <= nbins - 2)).sum()) >= 50
    assert int((tot < 4096).sum()) >= 50


@pytest.mark.gpu
@pytest.mark.parametrize("k,ncols", B_CASES)
def test_scans_of_saturated_counts_and_high_bins(mcx, orc, k, ncols):
    recs, uk, raw, body = b_case(orc, k, ncols)
    value = np.minimum(raw, U32)
    for grid in ((0, 1) if (k, ncols) == (31, 3) else (0,)):
        g = mcx.Graph(k, ncols, CAP)
        g.configure("grid", grid)
        g.add_records(recs, ncols, identity(ncols))
        assert g.nkmers == len(uk)
        assert g.export(True) == body
        check_scans(mcx, g, k, ncols, body, B_NBINS, cov=value)
        g.close()


# ---- C. tombstones: scans, then inserts over them -----------------------------------------------------
C_CASES = [(31, "deferred"), (31, "direct"), (63, "deferred"), (63, "direct"), (95, "direct"), (31, "records")]
_C = {}


def c_case(orc, k, kind):
    """reads with errors, the graph `clean(2, 2k)` leaves of them, and that graph after the same input again"""
    if (k, kind) in _C:
        return _C[k, kind]
    from test_gpu_clean import sample
    W = words(k)
    if (k, None) not in _C:
        seqs = sample(random.Random(300 + k), k, 1, 400 + 20 * k, 2000, 2 * k + 20, 0.1 / k)[0]
        bases, offs = orc.pack_reads(seqs)
        og = orc.Graph(k, 1, 1 << 18)
        og.add_reads(0, bases, offs)
        body0 = og.body_bytes(True)
        graph = R.parse(body0, k, 1)
        exp = R.clean(graph, k, 2, 2 * k)[0]
        _C[k, None] = (bases, offs, body0, len(graph) - len(exp), R.pack(exp, k, 1))
    bases, offs, body0, removed, body1 = _C[k, None]
    og = orc.Graph(k, 1, 1 << 18)
    orc_add_records(og, *parse_records(body1, W, 1))
    if kind == "reads":
        og.add_reads(0, bases, offs)
    else:
        orc_add_records(og, *parse_records(body0, W, 1))
    _C[k, kind] = dict(bases=bases, offs=offs, body0=body0, removed=removed, body1=body1, body2=og.body_bytes(True), nk2=og.nkmers)
    return _C[k, kind]


@pytest.mark.parametrize("k", [31, 63, 95])
def test_clean_inputs_leave_tombstones(orc, k):
    ref = c_case(orc, k, "reads")
    assert ref["removed"] >= 200
    rs = 8 * words(k) + 5
    assert ref["nk2"] == len(ref["body0"]) // rs  # the input holds every removed k-mer: the graph grows back


@pytest.mark.gpu
@pytest.mark.parametrize("k,path", C_CASES)
def test_scans_and_inserts_over_tombstones(mcx, orc, k, path):
    from test_gpu_clean import check
    ref = c_case(orc, k, "records" if path == "records" else "reads")
    g = mcx.Graph(k, 1, 1 << 17)
    g.configure("defer", 1 if path == "deferred" else 0)

    def load():
        if path == "records":
            g.add_records(ref["body0"], 1, [(0, 0)])
        else:
            g.add_reads(0, ref["bases"], ref["offs"])
        g.sync()

    load()
    assert g.export(True) == ref["body0"]
    st, _ = g.clean(2, 2 * k)
    assert st["nkmers_removed"] == ref["removed"]
    assert g.export(True) == ref["body1"]
    check_scans(mcx, g, k, 1, ref["body1"], (64,))  # the scans step over tombstones and their stale value words
    load()  # every removed k-mer comes back, past its tombstone
    assert g.nkmers == ref["nk2"]
    assert g.export(True) == ref["body2"]
    check_scans(mcx, g, k, 1, ref["body2"], (64,))
    check(g, k, 1, 2, 2 * k)  # a clean of the re-grown graph is the restatement's clean of it
    g.close()


_ISEC = {}


def isec_case(orc):
    """an intersection graph of which the must-exist reads cover a part: intersect_finish removes the rest"""
    if not _ISEC:
        import synth
        from oracle import ctxio
        k = 21
        g0 = synth.genome(20000, 31)
        ra = synth.reads(1500, 90, seed=1, g=g0)
        rq = synth.reads(1200, 100, seed=3, g=g0[:12000], n_frac=0.05, lower_frac=0.1)
        oi = orc.Graph(k, 1, 1 << 20)
        oi.add_reads(0, *ra)
        isec = oi.ctx_bytes(True)
        hdr, hs = ctxio.read_header(isec)
        keys, covgs, edges = ctxio.records(isec, hdr, hs)
        og = orc.Graph(k, 1, 1 << 20)
        for i in range(len(keys)):
            og.add_isec_record(keys[i], int(covgs[i, 0]), int(edges[i, 0]))
        og.set_must_exist(True)
        og.add_reads(0, *rq)
        before = og.nkmers
        og.isec_finish()
        _ISEC.update(k=k, isec=isec[hs:], rq=rq, removed=before - og.nkmers, nk=og.nkmers, body=og.body_bytes(True))
    return _ISEC


def test_intersect_input_leaves_tombstones(orc):
    ref = isec_case(orc)
    assert ref["removed"] >= 200 and ref["nk"] >= 200


@pytest.mark.gpu
def test_scans_after_intersect_finish(mcx, orc):
    ref = isec_case(orc)
    k = ref["k"]
    g = mcx.Graph(k, 2, 1 << 20)  # colour 1: the hidden holder of the intersection's edges
    g.configure("intersect", 1)
    g.add_records(ref["isec"], 1, [(0, 1)])
    g.configure("must_exist", 1)
    g.add_reads(0, *ref["rq"])
    g.intersect_finish()
    assert g.nkmers == ref["nk"]
    assert g.export(True) == ref["body"]
    check_scans(mcx, g, k, 1, ref["body"], (2, 64))
    g.close()


# ---- D. record-loader indices across chunks and calls (a child process with 1 KiB staging chunks) -----------
D_CASES = [(31, 1), (127, 3)]  # 78 and 21 records per chunk of 1024 bytes
D_SPLIT = 350                  # call 1 loads records [0, 350), call 2 the other 250
D_ZERO = (200, 90, D_SPLIT + 10)                 # no coverage in any colour
D_EDGES = (340, D_SPLIT + 5, D_SPLIT + 240)      # edges without coverage in the last colour
D_OVERSIZED = 250


def d_records(k, ncols, clean_call1=False):
    """600 records, keys repeating across chunks and calls, with the dirty records planted (not those of call 1
    when `clean_call1`)"""
    rng = np.random.default_rng(4000 + k)
    n = 600
    keys = random_keys(rng, k, n)
    keys[300:] = keys[rng.integers(0, 300, 300)]
    cov = rng.integers(1, 1000, (n, ncols)).astype(np.uint32)
    edg = rng.integers(0, 256, (n, ncols), dtype=np.uint8)
    for i in D_ZERO:
        if not (clean_call1 and i < D_SPLIT):
            cov[i], edg[i] = 0, 0
    for i in D_EDGES:
        if not (clean_call1 and i < D_SPLIT):
            cov[i, ncols - 1], edg[i, ncols - 1] = 0, edg[i, ncols - 1] | 1
    return keys, cov, edg


def d_first_dirty(calls):
    """graph_file_read_raw's checks restated over consecutive calls that share one stats object: after each call
    (first record without coverage, first record with edges but no coverage in some colour), the first seen kept"""
    base, fz, fe, out = 0, -1, -1, []
    for cov, edg in calls:
        zero = np.nonzero((cov == 0).all(axis=1))[0]
        enc = np.nonzero(((edg != 0) & (cov == 0)).any(axis=1))[0]
        if fz < 0 and len(zero):
            fz = base + int(zero[0])
        if fe < 0 and len(enc):
            fe = base + int(enc[0])
        base += len(cov)
        out.append([fz, fe])
    return out


def d_calls(k, ncols, clean_call1):
    keys, cov, edg = d_records(k, ncols, clean_call1)
    return [(keys[:D_SPLIT], cov[:D_SPLIT], edg[:D_SPLIT]), (keys[D_SPLIT:], cov[D_SPLIT:], edg[D_SPLIT:])]


def test_loader_plants_restated():
    """the expected indices, from the restatement: the lower of two plants in different chunks wins, a later call
    does not replace what an earlier one saw, a call's indices count from the records read before it"""
    for k, ncols in D_CASES:
        assert 1024 // (8 * words(k) + 5 * ncols) == {31: 78, 127: 21}[k]
        assert d_first_dirty([c[1:] for c in d_calls(k, ncols, False)]) == [[90, 340], [90, 340]]
        # a one-colour record with edges but no coverage is a record without coverage as well
        want = [D_SPLIT + 10, D_SPLIT + 5] if ncols > 1 else [D_SPLIT + 5, D_SPLIT + 5]
        assert d_first_dirty([c[1:] for c in d_calls(k, ncols, True)]) == [[-1, -1], want]


def child(out):
    sys.path.insert(0, ROOT)
    import mccortex_amd as mcx
    res = {}
    for k, ncols in D_CASES:
        r = {}
        for name, clean_call1 in (("dirty", False), ("clean_first", True)):
            g = mcx.Graph(k, ncols, CAP)
            st = mcx.RecordStats()
            after = []
            for call in d_calls(k, ncols, clean_call1):
                g.add_records(pack_records(*call), ncols, identity(ncols), stats=st)
                after.append(st.as_dict())
            r[name] = {"after": after, "nkmers": int(g.nkmers), "body": g.export(True).hex()}
            g.close()
        # an oversized key at index 250 of a call that follows 350 clean records
        g = mcx.Graph(k, ncols, CAP)
        st = mcx.RecordStats()
        g.add_records(pack_records(*d_calls(k, ncols, True)[0]), ncols, identity(ncols), stats=st)
        keys, cov, edg = (a[:300].copy() for a in d_records(k, ncols, True))
        keys[D_OVERSIZED, 0] |= np.uint64(1 << 62)
        try:
            g.add_records(pack_records(keys, cov, edg), ncols, identity(ncols), stats=st)
            r["oversized"] = {"raised": False}
        except mcx.McxError as e:
            r["oversized"] = {"raised": True, "code": e.code, "text": str(e), "stats": st.as_dict()}
        g.close()
        res["%d,%d" % (k, ncols)] = r
    json.dump(res, open(out, "w"))


@pytest.fixture(scope="module")
def loader_child(mcx, tmp_path_factory):
    out = tmp_path_factory.mktemp("loader") / "loader.json"
    env = dict(os.environ, MCX_STAGE_BYTES="1024")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return json.load(open(out))


@pytest.mark.gpu
@pytest.mark.parametrize("k,ncols", D_CASES)
def test_record_indices_across_chunks_and_calls(mcx, orc, loader_child, k, ncols):
    res = loader_child["%d,%d" % (k, ncols)]
    for name, clean_call1 in (("dirty", False), ("clean_first", True)):
        calls = d_calls(k, ncols, clean_call1)
        og = orc.Graph(k, ncols, 1 << 16)
        read = loaded = 0
        for call, st, dirty in zip(calls, res[name]["after"], d_first_dirty([c[1:] for c in calls])):
            read += len(call[0])
            loaded += orc_add_records(og, *call)
            print(k, ncols, name, st, dirty)
            assert [st["first_zero_covg"], st["first_edges_no_covg"]] == dirty, name
            assert (st["nkmers_read"], st["nkmers_loaded"], st["nkmers_novel"], st["first_oversized"]) == (read, loaded, og.nkmers, -1)
        # the whole load, chunk seams included: the oracle over the same records with the same skip rule
        assert res[name]["nkmers"] == og.nkmers and res[name]["body"] == og.body_bytes(True).hex(), name
    ov = res["oversized"]
    assert ov["raised"] and ov["code"] == mcx.graph.MCX_ERR_ARG and "record %d " % D_OVERSIZED in ov["text"], ov
    assert ov["stats"]["first_oversized"] == D_SPLIT + D_OVERSIZED and ov["stats"]["nkmers_read"] == D_SPLIT + 300


# ---- E. the sortedness check, at every position that matters ---------------------------------------------
E_CASES = [(31, 1), (63, 2), (95, 1), (127, 2)]
E_N = 1000


def e_sorted(k, ncols):
    """1000 sorted records: all 4^W combinations of four values per key word (as in
    test_ctxio.py::test_sort_records_every_lsd_pass_matters: keys that tie in every word but one) among random keys"""
    rng = np.random.default_rng(5000 + k)
    W = words(k)
    top_bits = 2 * k - 64 * (W - 1)
    pools = [np.array([0, 1, (1 << (top_bits - 1)) - 1, 1 << (top_bits - 1)], dtype=np.uint64)]
    pools += [np.array([0, 1, 1 << 63, (1 << 64) - 1], dtype=np.uint64) for _ in range(W - 1)]
    grid = np.stack(np.meshgrid(*pools, indexing="ij"), axis=-1).reshape(-1, W).astype(np.uint64)
    keys = np.unique(np.concatenate([grid, random_keys(rng, k, E_N - len(grid))]), axis=0)
    assert len(keys) == E_N
    cov = rng.integers(1, 1000, (E_N, ncols)).astype(np.uint32)
    return keys, cov, rng.integers(0, 256, (E_N, ncols), dtype=np.uint8)


def first_unsorted(keys):
    """binary_kmer_ge over adjacent records: the index of the second record of the first pair that does not
    increase, or -1"""
    rows = [tuple(int(w) for w in row) for row in keys]
    for i in range(1, len(rows)):
        if rows[i - 1] >= rows[i]:
            return i
    return -1


def e_mutations(keys):
    """{name: (order of the records, the index the check must report)}"""
    n = len(keys)
    low = next(i for i in range(n - 1) if np.array_equal(keys[i, :-1], keys[i + 1, :-1]))  # differ in the lowest word only

    def swap(*firsts):
        idx = np.arange(n)
        for a in firsts:
            idx[[a, a + 1]] = idx[[a + 1, a]]
        return idx

    def dup(i):
        idx = np.arange(n)
        idx[i] = idx[i - 1]
        return idx

    muts = {"sorted": (np.arange(n), -1), "lowest word": (swap(low), low + 1), "two violations": (swap(699, 299), 300)}
    for a in (0, 254, 255, 256, n - 2):  # the first pair, the seams of a 256-thread block, the last pair
        muts["swap %d" % a] = (swap(a), a + 1)
    for i in (1, 256, n - 1):
        muts["duplicate %d" % i] = (dup(i), i)
    return muts


@pytest.mark.parametrize("k,ncols", E_CASES)
def test_sortedness_mutations_restated(k, ncols):
    keys = e_sorted(k, ncols)[0]
    W = words(k)
    if W >= 2:  # some adjacent pair agrees in every word but the lowest
        assert any(np.array_equal(keys[i, :-1], keys[i + 1, :-1]) and keys[i, -1] != keys[i + 1, -1] for i in range(E_N - 1))
    for name, (idx, want) in e_mutations(keys).items():
        assert first_unsorted(keys[idx]) == want, name


@pytest.mark.gpu
@pytest.mark.parametrize("k,ncols", E_CASES)
def test_sortedness_check_at_every_position(mcx, k, ncols):
    keys, cov, edg = e_sorted(k, ncols)
    for name, (idx, _) in e_mutations(keys).items():
        assert mcx.records_sorted(pack_records(keys[idx], cov[idx], edg[idx]), k, ncols) == first_unsorted(keys[idx]), name
    for idx, want in (([0, 1], -1), ([1, 0], 1)):  # two records, both orders
        assert first_unsorted(keys[idx]) == want
        assert mcx.records_sorted(pack_records(keys[idx], cov[idx], edg[idx]), k, ncols) == want


if __name__ == "__main__":
    child(sys.argv[1])
