"""The one-word, one-colour LDS insert has a batch loop of its own (mcx_defer.h, k_lds_insert: run_lean; a version of
it that probed one tuple ahead was measured slower and is not kept, but its cases are).  The states in which a stale
bucket snapshot, a batch seam or the set-aside queue could go wrong, reached on purpose on the deferred path.  Every
case compares the sorted records, nkmers and the checksum with the oracle (reads) or with the dictionary of
tests/tuples_ref.py (ready-made tuples), and asserts that k_lds_insert ran.

Table size.  The partition path needs at least 64 regions (mcx_api.hip, ensure_defer: lb1 >= 6), so the smallest
table it serves has 64 sub-tables of 4096 slots, 2^18 slots, not the four sub-tables one might wish for.  To have ONE
workgroup meet every case all the same, each case also runs with grid_insert = 1: a single workgroup then visits
all 64 sub-tables in turn, every visit but the last with the next slice on its way (has_next), while the default
grid gives every sub-table a workgroup of its own (no next slice)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402
import tuples_ref as T  # noqa: E402

gpu = pytest.mark.gpu  # (the tests without it check, on the references alone, that the inputs reach their states)

CAP = 1 << 18            # 64 regions x 1 sub-table of 4096 slots (one-word keys)
NMAIN = 1 << 18
K = 31
LBQ = 6                  # log2 regions of that table
KSTEP = 512 * 4          # tuples a workgroup applies per batch (LdsCfg: kThreads x kBatch)
GRIDS = [0, 1]           # grid_insert: default, one workgroup for all sub-tables


# ---- helpers -----------------------------------------------------------------------------------------
def new_graph(mcx, k, ncols, grid_insert, cap=CAP):
    g = mcx.Graph(k, ncols, cap)
    g.configure("defer", 1)
    g.configure("profile", 1)
    if grid_insert:
        g.configure("grid_insert", grid_insert)
    return g


def check_body(mcx, g, k, ncols, want_body, want_nkmers):
    """sorted records, nkmers and checksum; the LDS insert took the occurrences"""
    g.sync()
    assert "k_lds_insert" in g.profile(), sorted(g.profile())
    assert g.nkmers == want_nkmers
    body = g.export(True)
    if body != want_body:  # (say where, not megabytes of bytes)
        rs = 8 * T.words(k) + 5 * ncols
        assert len(body) == len(want_body), (len(body) // rs, len(want_body) // rs)
        a = np.frombuffer(body, np.uint8).reshape(-1, rs)
        b = np.frombuffer(want_body, np.uint8).reshape(a.shape)
        bad = np.nonzero((a != b).any(axis=1))[0]
        raise AssertionError("%d of %d records differ, first %d: got %s, want %s"
                             % (len(bad), len(a), bad[0], a[bad[0]].tobytes().hex(), b[bad[0]].tobytes().hex()))
    cs, n = g.checksum()
    assert (cs, n) == (mcx.records_checksum(want_body, k, ncols), want_nkmers)


def oracle_body(og):
    return og.ctx_bytes(True)[og.header_size():]


_ORACLE = {}


def oracle_of(orc, name, k, ncols, jobs_fn):
    """the oracle's (bodies after each job, nkmers after each job) of a named case, computed once"""
    if name not in _ORACLE:
        og = orc.Graph(k, ncols, 1 << 20)
        out = []
        for col, bases, offs in jobs_fn():
            og.add_reads(col, bases, offs)
            out.append((oracle_body(og), og.nkmers))
        _ORACLE[name] = out
    return _ORACLE[name]


def run_reads_case(mcx, orc, name, k, ncols, jobs_fn, grid_insert):
    want = oracle_of(orc, name, k, ncols, jobs_fn)
    g = new_graph(mcx, k, ncols, grid_insert)
    for (col, bases, offs), (body, nk) in zip(jobs_fn(), want):
        g.add_reads(col, bases, offs)
        check_body(mcx, g, k, ncols, body, nk)
    g.close()
    return want


def repeat_reads(read, times):
    bases = np.tile(read, times)
    offs = (np.arange(times + 1, dtype=np.uint64) * np.uint64(len(read)))
    return np.ascontiguousarray(bases), offs


def concat_reads(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.ascontiguousarray(np.concatenate(reads)), offs


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- 1. the same novel key in adjacent tuples of one thread and across lanes ---------------------------------
REPEAT = 4096


def _same_read_jobs():
    read = synth.genome(150, seed=9101)
    return [(0, *repeat_reads(read, REPEAT))]


def _same_read_subst_jobs():
    rng = np.random.default_rng(9102)
    bases, offs = repeat_reads(synth.genome(150, seed=9101), REPEAT)
    hit = rng.random(len(bases)) < 0.01
    bases = bases.copy()
    bases[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return [(0, bases, offs)]


@gpu
@pytest.mark.parametrize("grid_insert", GRIDS)
def test_one_read_many_times(mcx, orc, grid_insert):
    """Every k-mer of the read is novel 4096 times at once: first occurrences of one key sit in adjacent tuples of
    a thread and in many lanes, so most of them probe with a snapshot that predates the key's slot.  Coverage per
    k-mer must be the repeat count exactly."""
    run_reads_case(mcx, orc, "same", K, 1, _same_read_jobs, grid_insert)


@gpu
@pytest.mark.parametrize("grid_insert", GRIDS)
def test_one_read_many_times_with_substitutions(mcx, orc, grid_insert):
    run_reads_case(mcx, orc, "same-subst", K, 1, _same_read_subst_jobs, grid_insert)


def test_repeat_inputs_reach_their_states(orc):
    _, cov, _ = T.parse_body(oracle_of(orc, "same", K, 1, _same_read_jobs)[0][0], 1, 1)
    assert len(cov) == 150 - K + 1 and (cov == REPEAT).all()  # coverage per k-mer = the repeat count, exactly
    _, cov, _ = T.parse_body(oracle_of(orc, "same-subst", K, 1, _same_read_subst_jobs)[0][0], 1, 1)
    assert len(cov) > 5000 and int(cov.max()) > REPEAT // 2  # thousands of rare keys beside the hot ones


# ---- 2. full buckets and queue overflow -----------------------------------------------------------------------
def _dense_jobs():
    """a random genome whose k-mers fill 95 % of the hash-addressed slots, tiled by reads that overlap by k - 1
    (every k-mer once), twice"""
    nk = NMAIN * 95 // 100
    g = synth.genome(nk + K - 1, seed=9201)
    reads = [g[s:s + 120 + K - 1] for s in range(0, nk, 120)]
    bases, offs = concat_reads(reads)
    return [(0, bases, offs), (0, bases, offs)]


@gpu
@pytest.mark.parametrize("grid_insert", GRIDS)
def test_dense_table_then_all_hits(mcx, orc, grid_insert):
    """At load 0.95 most buckets are full: some 700 tuples per sub-table meet a full bucket and more lose their CAS,
    so the set-aside queue is long and lds_apply walks far.  Whether it passes the queue's 1856 entries here depends
    on timing; test_queue_overflow_in_the_batch_loop does so by construction.  The second batch of the same reads
    only hits."""
    run_reads_case(mcx, orc, "dense", K, 1, _dense_jobs, grid_insert)


def test_dense_input_fills_the_table(orc):
    want = oracle_of(orc, "dense", K, 1, _dense_jobs)
    assert NMAIN * 94 // 100 <= want[0][1] <= NMAIN * 95 // 100 and want[1][1] == want[0][1]
    _, cov, _ = T.parse_body(want[1][0], 1, 1)
    assert (cov == 2).all()


# ---- 3. batch seams ---------------------------------------------------------------------------------------------
SEAM_FILLS = [0, 1, KSTEP - 1, KSTEP, KSTEP + 1, 2 * KSTEP + 1]
SEAM_SUBS = [3, 7, 12, 20, 41, 63]  # the sub-table given each fill (fill 0: no tuple, and no visit)
MAX_DISTINCT = 1500


def sub_of(keys):
    """sub-table of one-word keys in the 2^18-slot table (mcx_kernels.h, "Table addressing"): key = q << 6 | r,
    region = r ^ top 6 bits of mix(q), one sub-table per region"""
    q = keys >> np.uint64(LBQ)
    x = ((q & np.uint64(0xFFFFFFFF)) ^ (q >> np.uint64(32))).astype(np.uint64)
    m = (x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((keys & np.uint64((1 << LBQ) - 1)) ^ (m >> np.uint64(32 - LBQ))).astype(np.int64)


def keys_in_sub(rng, sub, n):
    """n distinct keys of sub-table `sub`"""
    q = np.unique(rng.integers(1, 1 << (2 * K - LBQ), 2 * n + 16, dtype=np.uint64))
    q = q[rng.permutation(len(q))[:n]]
    assert len(q) == n
    probe = q << np.uint64(LBQ)
    keys = probe | (np.uint64(sub) ^ sub_of(probe).astype(np.uint64))
    assert (sub_of(keys) == sub).all()
    return keys


def seam_tuples():
    rng = np.random.default_rng(9301)
    parts = []
    for sub, fill in zip(SEAM_SUBS, SEAM_FILLS):
        if fill:
            distinct = keys_in_sub(rng, sub, min(fill, MAX_DISTINCT))
            parts.append(distinct[np.arange(fill) % len(distinct)])
    keys = np.concatenate(parts)
    keys = keys[rng.permutation(len(keys))].reshape(-1, 1)
    return keys, T.random_edges(rng, len(keys))


def test_seam_tuples_fill_their_subtables():
    keys, _ = seam_tuples()
    fills = np.bincount(sub_of(keys[:, 0]), minlength=64)
    assert [int(fills[s]) for s in SEAM_SUBS] == SEAM_FILLS and int(fills.sum()) == sum(SEAM_FILLS)


@gpu
@pytest.mark.parametrize("grid_insert", GRIDS)
def test_batch_seams(mcx, grid_insert):
    """Sub-table bins of 0, 1, kStep - 1, kStep, kStep + 1 and 2 kStep + 1 tuples: a thread's index past
    the fill loads tuple 0 of the bin, which must not be applied, and the last tuple before a seam must be.  The unsorted export
    runs in slot order, so it also shows that sub_of() above is the table's own addressing."""
    import torch
    keys, edges = seam_tuples()
    g = new_graph(mcx, K, 1, grid_insert)
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    de = torch.from_numpy(edges).cuda()
    g.insert_tuples_dev(0, dk, de, len(keys))
    uk, cov, edg = T.ref_table(keys, edges, 0, 1)
    assert int(cov.sum()) == sum(SEAM_FILLS)
    check_body(mcx, g, K, 1, T.pack_body(uk, cov, edg), len(uk))
    prof = g.profile()
    assert "k_tuples_bin" in prof and "k_insert_tuples" not in prof, sorted(prof)
    tk, _, _ = T.parse_body(g.export(False), 1, 1)
    subs = sub_of(tk[:, 0])
    assert (np.diff(subs) >= 0).all()
    assert np.bincount(subs, minlength=64).tolist() == np.bincount(sub_of(uk[:, 0]), minlength=64).tolist()
    g.close()


# ---- 3b. the set-aside queue overflows whatever the timing ----------------------------------------------------------
QUEUE = 1856                       # LdsQueue<1>::kTuples
CHAIN_SUB, CHAIN_BUCKET = 29, 777  # every key of the chain starts at this bucket of this sub-table
CHAIN_KEYS = QUEUE + 4 + KSTEP + 40        # distinct keys: four fit the bucket, the rest are set aside
CHAIN_TUPLES = 3 * KSTEP + 5               # with repeats: a second pass of the batch loop, and a ragged end
MARK_SUB, MARK_BUCKETS = 9, [5, 200, 600, 1000]


def bucket_of(keys):
    """start bucket inside the sub-table: the 10 bits of mix(q) below the region's 6 (mcx_kernels.h, mix_bucket)"""
    q = keys >> np.uint64(LBQ)
    x = ((q & np.uint64(0xFFFFFFFF)) ^ (q >> np.uint64(32))).astype(np.uint64)
    m = (x * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return ((m >> np.uint64(22 - LBQ)) & np.uint64(1023)).astype(np.int64)


def keys_in_buckets(rng, sub, buckets, n):
    """n distinct keys of sub-table `sub` for each of `buckets`, the start bucket of their probe sequence"""
    got = {b: np.zeros(0, np.uint64) for b in buckets}
    while min(len(v) for v in got.values()) < n:
        cand = keys_in_sub(rng, sub, 1 << 21)
        bk = bucket_of(cand)
        for b in buckets:
            got[b] = np.unique(np.concatenate([got[b], cand[bk == b]]))
    return [got[b][rng.permutation(len(got[b]))[:n]] for b in buckets]


_CHAIN = []


def chain_tuples():
    if not _CHAIN:
        rng = np.random.default_rng(9351)
        chain = keys_in_buckets(rng, CHAIN_SUB, [CHAIN_BUCKET], CHAIN_KEYS)[0]
        # every distinct key once, then repeats (hits for the four stored keys, set aside again for the others)
        keys = np.concatenate([chain, chain[rng.integers(0, CHAIN_KEYS, CHAIN_TUPLES - CHAIN_KEYS)]])
        keys = keys[rng.permutation(len(keys))]
        marks = np.concatenate(keys_in_buckets(rng, MARK_SUB, MARK_BUCKETS, 3))
        keys = np.concatenate([keys, marks]).reshape(-1, 1)
        _CHAIN.append((keys, T.random_edges(rng, len(keys))))
    return _CHAIN[0]


def test_chain_input_overflows_the_queue():
    """The straight-line probe looks at the start bucket only, and that bucket holds four keys: whatever order the
    tuples reach the bin in, every tuple of the other keys is set aside, by the probe that finds the bucket full or
    by the CAS it loses.  A batch of kStep tuples therefore sets aside at least kStep - (the tuples of four keys),
    which is more than the queue holds: the queue overflows inside the FIRST batch, and every set-aside tuple of the
    second batch and of the second pass of the batch loop finds it full."""
    keys, _ = chain_tuples()
    k = keys[:, 0]
    chain = k[sub_of(k) == CHAIN_SUB]
    assert len(chain) == CHAIN_TUPLES > 2 * KSTEP and (bucket_of(chain) == CHAIN_BUCKET).all()
    uniq, mult = np.unique(chain, return_counts=True)
    assert len(uniq) == CHAIN_KEYS >= QUEUE + 4 + KSTEP and CHAIN_KEYS <= 4096  # (they all fit the sub-table)
    assert KSTEP - 4 * int(mult.max()) > QUEUE
    marks = k[sub_of(k) == MARK_SUB]
    assert bucket_of(marks).tolist() == [b for b in MARK_BUCKETS for _ in range(3)]


@gpu
@pytest.mark.parametrize("grid_insert", GRIDS)
def test_queue_overflow_in_the_batch_loop(mcx, grid_insert):
    """(why the queue must overflow: test_chain_input_overflows_the_queue.)  drain() runs behind both batches, in
    both passes of the batch loop.  The marker keys (three per bucket, four buckets of another sub-table) come out
    of the unsorted export in bucket order, which shows that bucket_of() above is the table's own start bucket."""
    import torch
    keys, edges = chain_tuples()
    g = new_graph(mcx, K, 1, grid_insert)
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    de = torch.from_numpy(edges).cuda()
    g.insert_tuples_dev(0, dk, de, len(keys))
    uk, cov, edg = T.ref_table(keys, edges, 0, 1)
    assert len(uk) == CHAIN_KEYS + 3 * len(MARK_BUCKETS) and int(cov.sum()) == len(keys)
    check_body(mcx, g, K, 1, T.pack_body(uk, cov, edg), len(uk))
    prof = g.profile()
    assert "k_tuples_bin" in prof and "k_insert_tuples" not in prof, sorted(prof)
    tk, _, _ = T.parse_body(g.export(False), 1, 1)
    tk = tk[:, 0]
    assert (np.diff(sub_of(tk)) >= 0).all()
    assert bucket_of(tk[sub_of(tk) == MARK_SUB]).tolist() == [b for b in MARK_BUCKETS for _ in range(3)]
    g.close()


# ---- 4. edge bits that arrive late ----------------------------------------------------------------------------------
def _late_edges_jobs():
    """500 copies of a read, then the bare k-mers of that read (no edges at all), then 40 variants that each change
    one base, 30 copies each: the k-mers next to the changed base gain a successor or predecessor bit they did not
    have, long after their coverage started counting.  One call, one flush."""
    rng = np.random.default_rng(9401)
    read = synth.genome(150, seed=9402)
    reads = [read] * 500
    reads += [read[i:i + K] for i in range(0, 150 - K + 1, 3)]
    for _ in range(40):
        p = int(rng.integers(K, 150 - K))
        v = read.copy()
        v[p] = ACGT[(int(np.nonzero(ACGT == read[p])[0][0]) + int(rng.integers(1, 4))) % 4]
        reads += [v] * 30
    bares = [synth.genome(K, seed=9500 + i) for i in range(64)]  # keys whose FIRST occurrence has no edge ...
    tails = [np.concatenate([b, ACGT[rng.integers(0, 4, 5)]]) for b in bares]  # ... and whose later ones do
    reads = bares + reads + tails
    return [(0, *concat_reads(reads))]


@gpu
@pytest.mark.parametrize("grid_insert", GRIDS)
def test_edges_gained_late_in_a_visit(mcx, orc, grid_insert):
    """(the records hold the edge bytes: the body comparison is byte for byte)"""
    run_reads_case(mcx, orc, "late-edges", K, 1, _late_edges_jobs, grid_insert)


def test_late_edges_input_branches(orc):
    _, cov, edg = T.parse_body(oracle_of(orc, "late-edges", K, 1, _late_edges_jobs)[0][0], 1, 1)
    assert int(cov.max()) >= 500 + 30
    nbits = np.unpackbits(edg.reshape(-1, 1), axis=1).sum(axis=1)
    assert int((nbits >= 3).sum()) >= 40  # k-mers next to a changed base: bits from more than one variant
    assert int((nbits == 1).sum()) >= 64  # the k-mers first seen bare, then once with a successor


# ---- 5. the paths that are not restructured ----------------------------------------------------------------------------
def _k63_jobs():
    return [(0, *synth.reads(2000, 150, genome_len=30000, seed=9501, n_frac=0.05))]


def _two_colour_jobs():
    bases, offs = synth.reads(3000, 120, genome_len=30000, seed=9502, n_frac=0.05)
    return [(0, bases, offs), (1, bases[: int(offs[1200])], offs[:1201])]


@gpu
def test_two_word_keys(mcx, orc):
    run_reads_case(mcx, orc, "k63", 63, 1, _k63_jobs, 0)


@gpu
def test_two_colours(mcx, orc):
    run_reads_case(mcx, orc, "two-colours", K, 2, _two_colour_jobs, 0)
