"""The entries that take ready-made (key words, edge byte) tuples -- mcx_graph_insert_tuples_dev,
mcx_graph_insert_tuple_segments_dev, mcx_graph_hashtest -- against the dictionary of tests/tuples_ref.py:

    coverage[key][colour] += 1;  edges[key][colour] |= e        for every tuple

Every device test compares the sorted export byte for byte with the reference's body, and nkmers and kmer_covg()
with its sums; each asserts which path ran (the profile names k_insert_tuples = direct or k_tuples_bin = deferred;
insert_stats gives the flushes and the foreign inserts).  Keys are handed over exactly as generated: all-zero,
all-ones, both strands of a k-mer, small integers with bits above 2k.  The tests that are not marked `gpu` show on
the reference alone that the inputs reach the states the device tests are about."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tuples_ref as T  # noqa: E402
from test_gpu_table_states import geometry  # noqa: E402  (nmain, novf) of a table on one device

U32 = T.U32
CAP = 1 << 18      # 64 sub-tables of one-word keys, 128 of longer ones: the smallest table with the deferred path
N = 100_000        # tuples per key set
WIDTHS = (21, 31, 33, 63, 65, 95, 97, 127)
NARROW = (21, 31, 33, 63)


# ---- inputs, made once -----------------------------------------------------------------------------
_SETS, _REFS = {}, {}


def key_set(name, k):
    """(keys, edges) of a named key set at k"""
    if (name, k) not in _SETS:
        rng = np.random.default_rng(7000 + 10 * k + ("uniform", "corners", "hot").index(name))
        if name == "hot":
            keys, edges, _ = T.hot(rng, k)
        else:
            keys = T.uniform(rng, k, N) if name == "uniform" else T.corners(rng, k, N)
            edges = T.random_edges(rng, len(keys))
        _SETS[name, k] = (keys, edges)
    return _SETS[name, k]


def calls_of(n, cmode, seed=0):
    """-> (ncols, [(lo, hi, colour)]): one colour; three colours, all tuples in colour 2; three colours, six calls of
    uneven sizes each with its own colour"""
    if cmode == "one":
        return 1, [(0, n, 0)]
    if cmode == "col2":
        return 3, [(0, n, 2)]
    rng = np.random.default_rng(seed)
    cuts = [0] + sorted(rng.choice(np.arange(1, n), 5, replace=False).tolist()) + [n]
    colours = rng.permutation([0, 1, 2, 2, 0, 1]).tolist()
    return 3, [(cuts[i], cuts[i + 1], colours[i]) for i in range(6)]


def cols_of(n, calls):
    cols = np.zeros(n, dtype=np.int64)
    for lo, hi, c in calls:
        cols[lo:hi] = c
    return cols


def set_ref(name, k, cmode):
    if (name, k, cmode) not in _REFS:
        keys, edges = key_set(name, k)
        ncols, calls = calls_of(len(keys), cmode, seed=k)
        _REFS[name, k, cmode] = T.ref_table(keys, edges, cols_of(len(keys), calls), ncols)
    return _REFS[name, k, cmode]


_BIG = {}


def big_uniform(k):
    """3 x 2^20 uniform tuples (the oversized segments call; its first 2.5 M are the many-reservations case)"""
    if k not in _BIG:
        rng = np.random.default_rng(7700 + k)
        keys = T.uniform(rng, k, 3 << 20)
        _BIG[k] = (keys, T.random_edges(rng, len(keys)))
    return _BIG[k]


def big_ref(k, n):
    if (k, n) not in _BIG:
        keys, edges = big_uniform(k)
        _BIG[k, n] = T.ref_table(keys[:n], edges[:n], 0, 1)
    return _BIG[k, n]


# ---- device helpers ----------------------------------------------------------------------------------
def dev(a):
    """numpy array -> tensor in HBM (64-bit words as their int64 bit patterns)"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def insert(g, colour, keys, edges, hold):
    """one call of the tuple entry; the buffers stay in `hold` until the caller has synced the graph"""
    dk, de = dev(keys), dev(edges)
    hold.append((dk, de))
    g.insert_tuples_dev(colour, dk, de, len(keys))


def insert_calls(g, keys, edges, calls):
    hold = []
    for lo, hi, c in calls:
        insert(g, c, keys[lo:hi], edges[lo:hi], hold)
    g.sync()


def new_graph(mcx, k, ncols, cap=CAP, defer=None, **kw):
    g = mcx.Graph(k, ncols, cap, **kw)
    if defer is not None:
        g.configure("defer", defer)
    g.configure("profile", 1)
    return g


def check(g, table):
    """the table's contents against the reference (keys, unclamped coverage, edges)"""
    uk, cov, edg = table
    assert g.nkmers == len(uk)
    nk, sc = g.kmer_covg()
    want_nk, want_sc = T.covg_expect(cov)
    assert (nk.tolist(), sc.tolist()) == (want_nk, want_sc)
    body = g.export(True)
    want = T.pack_body(uk, cov, edg)
    if body != want:  # (say where, not two megabytes of bytes)
        W, ncols = uk.shape[1], cov.shape[1]
        assert len(body) == len(want), (len(body), len(want))
        a = np.frombuffer(body, np.uint8).reshape(-1, 8 * W + 5 * ncols)
        b = np.frombuffer(want, np.uint8).reshape(a.shape)
        bad = np.nonzero((a != b).any(axis=1))[0]
        raise AssertionError("%d of %d records differ, first %d: got %s, want %s"
                             % (len(bad), len(a), bad[0], a[bad[0]].tobytes().hex(), b[bad[0]].tobytes().hex()))


def path(g, direct, foreign=0, min_flushes=1):
    """which kernels took the tuples, and the counters of the rare branches"""
    prof, st = g.profile(), g.insert_stats()
    print("profile", sorted(prof), "stats", st)
    if direct:
        assert "k_insert_tuples" in prof and "k_tuples_bin" not in prof, prof
        assert (st["flushes"], st["fallback_inserts"]) == (0, 0), st
    else:
        assert "k_tuples_bin" in prof and "k_lds_insert" in prof and "k_insert_tuples" not in prof, prof
        assert st["flushes"] >= min_flushes, st
    assert st["foreign_inserts"] == foreign, st
    return st


# ---- the reference itself (no device) -----------------------------------------------------------------
def test_ref_body_by_hand():
    """4 tuples, 2 colours, two-word keys: key (1, 5) twice in colour 0 and once in colour 1, key (0, 9) once"""
    keys = np.array([[1, 5], [0, 9], [1, 5], [1, 5]], dtype=np.uint64)
    edges = np.array([0x81, 0x10, 0x02, 0x40], dtype=np.uint8)
    body = T.ref_body(keys, edges, [0, 1, 0, 1], 2)
    import struct
    want = struct.pack("<QQIIBB", 0, 9, 0, 1, 0x00, 0x10) + struct.pack("<QQIIBB", 1, 5, 2, 1, 0x83, 0x40)
    assert body == want
    # a preload: coverage is added and clamped, edges are OR-ed in, a key of its own stays
    pre = (np.array([[1, 5], [0, 1]], dtype=np.uint64), np.array([[U32 - 1, 0], [7, 0]]), np.array([[0x04, 0], [0x20, 0]], dtype=np.uint8))
    body = T.ref_body(keys, edges, [0, 1, 0, 1], 2, preload=pre)
    want = struct.pack("<QQIIBB", 0, 1, 7, 0, 0x20, 0) + struct.pack("<QQIIBB", 0, 9, 0, 1, 0x00, 0x10) + \
        struct.pack("<QQIIBB", 1, 5, U32, 1, 0x87, 0x40)
    assert body == want
    assert T.sort_body(body[26:] + body[:26], 2, 2) == body


@pytest.mark.parametrize("k", WIDTHS)
def test_key_sets_reach_their_states(k):
    W = T.words(k)
    keys, edges = key_set("uniform", k)
    assert len(keys) == N and 0.3 <= T.repeat_share(keys) <= 0.7
    assert int(keys[:, 0].max()) < (1 << T.top_bits(k)) and int(keys[:, 0].max()) >= (1 << (T.top_bits(k) - 1))
    assert len(np.unique(edges)) == 256
    # hot: coverage 70 000 and every edge bit
    rng = np.random.default_rng(1)
    hk, he, row = T.hot(rng, k)
    uk, cov, edg = T.ref_table(hk, he, 0, 1)
    i = int(np.nonzero((uk == row).all(axis=1))[0][0])
    assert int(cov[i, 0]) == T.HOT == 70_000 and int(edg[i, 0]) == 0xFF and len(hk) == 100_000
    assert int(np.delete(cov[:, 0], i).max()) <= 2
    # corners: all of them are in the set, as given
    groups = T.corner_keys(np.random.default_rng(7000 + 10 * k + 1), k)
    ck, _ = key_set("corners", k)
    have = {r.tobytes() for r in ck}
    for name, rows in groups.items():
        assert all(r.tobytes() in have for r in rows), name
    z = groups["zero, all ones"]
    assert not z[0].any() and T.key_int(z[1]) == (1 << (2 * k)) - 1
    a, b = (T.key_int(r) for r in groups["both strands"])
    assert a != b and T.revcomp(a, k) == b and T.revcomp(b, k) == a
    assert all(T.key_int(groups["bit 0"][i]) ^ T.key_int(groups["bit 0"][i + 1]) == 1 for i in range(0, 8, 2))
    assert all(T.key_int(groups["top bit"][i]) ^ T.key_int(groups["top bit"][i + 1]) == 1 << (2 * k - 1) for i in range(0, 8, 2))
    q = groups["one quotient"]
    assert len(q) == 64 and len({T.key_int(r) >> 6 for r in q}) == 1 and len({T.key_int(r) & 63 for r in q}) == 64
    if W >= 2:
        lo, hi = groups["word W-1 only"], groups["word 0 only"]
        assert (lo[:, :-1] == lo[0, :-1]).all() and len(np.unique(lo[:, -1])) == len(lo)
        assert (hi[:, 1:] == hi[0, 1:]).all() and len(np.unique(hi[:, 0])) == len(hi) >= 2
    # integers across a 32-bit boundary, bits above 2k included at k = 33 and 65
    ik = T.integers(k, (1 << 32) - 1000, 2000)
    assert int(ik[0, 0]) < (1 << 32) <= int(ik[-1, 0]) and not ik[:, 1:].any()


# ---- a. the direct path, every key width ----------------------------------------------------------------
A_CASES = [(k, c, 0) for k in WIDTHS for c in ("one", "col2", "percall")] + \
          [(k, c, None) for k in (65, 95, 97, 127) for c in ("one", "percall")]  # defer left at its default


@pytest.mark.gpu
@pytest.mark.parametrize("k,cmode,defer", A_CASES)
def test_direct_path(mcx, k, cmode, defer):
    for name in ("uniform", "corners", "hot"):
        keys, edges = key_set(name, k)
        ncols, calls = calls_of(len(keys), cmode, seed=k)
        g = new_graph(mcx, k, ncols, defer=defer)
        insert_calls(g, keys, edges, calls)
        check(g, set_ref(name, k, cmode))
        path(g, True)
        g.close()


# ---- b. the deferred path ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", NARROW)
@pytest.mark.parametrize("cmode", ["one", "col2", "percall"])
def test_deferred_path(mcx, k, cmode):
    for name in ("uniform", "corners", "hot"):
        keys, edges = key_set(name, k)
        ncols, calls = calls_of(len(keys), cmode, seed=k)
        g = new_graph(mcx, k, ncols, defer=1)
        insert_calls(g, keys, edges, calls)
        check(g, set_ref(name, k, cmode))
        path(g, False)
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", NARROW)
@pytest.mark.parametrize("sets", [None, "1"])
def test_eight_calls_without_a_sync(mcx, k, sets, monkeypatch):
    """colours cycle 0, 1, 2, 0, ...: with the default bin sets every colour keeps a set until the one flush; with one
    set (MCX_L1_SETS=1, read when the bins are first made) every change of colour flushes"""
    if sets:
        monkeypatch.setenv("MCX_L1_SETS", sets)
    else:
        monkeypatch.delenv("MCX_L1_SETS", raising=False)
    keys, edges = key_set("uniform", k)
    cuts = np.linspace(0, len(keys), 9).astype(int)
    calls = [(int(cuts[i]), int(cuts[i + 1]), i % 3) for i in range(8)]
    g = new_graph(mcx, k, 3, defer=1)
    insert_calls(g, keys, edges, calls)
    check(g, T.ref_table(keys, edges, cols_of(len(keys), calls), 3))
    st = path(g, False, min_flushes=8 if sets else 1)
    if not sets:
        assert st["flushes"] <= 3, st  # (one pass per colour at most: nothing flushed between the calls)
    g.close()


# ---- c. more than one reservation per call -----------------------------------------------------------------
C_N = 2_500_000


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("grid", [0, 1])
def test_one_call_of_many_reservations(mcx, k, grid):
    keys, edges = big_uniform(k)
    g = new_graph(mcx, k, 1, cap=1 << 22, defer=1)
    g.configure("defer_tuples", 1 << 20)
    if grid:
        g.configure("grid", 1)
        g.configure("grid_split", 1)
    insert_calls(g, keys[:C_N], edges[:C_N], [(0, C_N, 0)])
    check(g, big_ref(k, C_N))
    path(g, False, min_flushes=2)
    g.close()


# ---- d. 1024 and 2048 region bins ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("cmode", ["one", "percall"])
@pytest.mark.parametrize("lb1,nsub", [(10, 1100), (11, 2100)])
def test_forced_region_bins(mcx, k, cmode, lb1, nsub, monkeypatch):
    from test_gpu_tileloops import _forced
    monkeypatch.setenv("MCX_LB1", str(lb1))
    cap, slots = _forced(nsub, lb1, T.words(k))
    rng = np.random.default_rng(7300 + k + lb1)
    n = 300_000
    keys, edges = T.uniform(rng, k, n), T.random_edges(rng, n)
    ncols, calls = calls_of(n, cmode, seed=lb1)
    g = new_graph(mcx, k, ncols, cap=cap, defer=1)
    g.configure("defer_tuples", 1 << 22)  # (the default flush window of a table this size would take tens of GB)
    assert g.capacity()[0] == slots
    insert_calls(g, keys, edges, calls)
    check(g, T.ref_table(keys, edges, cols_of(n, calls), ncols))
    path(g, False)
    g.close()


# ---- e. a shard of a split table takes every key ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("cmode", ["one", "col2"])
def test_shard_inserts_foreign_keys_directly(mcx, k, cmode):
    keys, edges = key_set("uniform", k)
    ncols, calls = calls_of(len(keys), cmode)
    g = new_graph(mcx, k, ncols, defer=1, nparts=4, part=1)
    uk, inv = np.unique(keys, axis=0, return_inverse=True)
    owner = np.array([g.key_owner([int(w) for w in row]) for row in uk])[np.asarray(inv).ravel()]
    owned, foreign = int((owner == 1).sum()), int((owner != 1).sum())
    assert owned >= 1000 and foreign >= 1000, (owned, foreign)
    insert_calls(g, keys, edges, calls)
    check(g, set_ref("uniform", k, cmode))
    path(g, False, foreign=foreign)
    g.close()


# ---- f. full sub-tables: the overflow area ------------------------------------------------------------------------
def spill_keys(k):
    nmain, novf = geometry(k, CAP)
    n = nmain + novf // 2
    rng = np.random.default_rng(7400 + k)
    keys = np.unique(T.random_keys(rng, k, n + 4096), axis=0)
    keys = keys[rng.permutation(len(keys))[:n]]
    return nmain, novf, keys, T.random_edges(rng, 2 * n)


@pytest.mark.parametrize("k", [31, 63, 127])
def test_spill_input_exceeds_the_hash_addressed_slots(k):
    nmain, novf, keys, _ = spill_keys(k)
    assert (nmain, novf) == (1 << 18, 1 << 13)
    n = len(np.unique(keys, axis=0))
    assert n == len(keys) == nmain + novf // 2 and nmain + novf // 4 <= n <= nmain + 3 * novf // 4


@pytest.mark.gpu
@pytest.mark.parametrize("k,defer", [(31, 1), (31, 0), (63, 1), (63, 0), (127, 0)])
def test_tuples_into_full_subtables(mcx, k, defer):
    nmain, novf, keys, edges = spill_keys(k)
    n = len(keys)
    g = new_graph(mcx, k, 1, defer=defer)
    assert g.capacity()[0] == nmain + novf
    insert_calls(g, np.concatenate([keys, keys]), edges, [(0, n, 0), (n, 2 * n, 0)])
    assert g.nkmers == n > nmain  # the spill, by arithmetic
    table = T.ref_table(np.concatenate([keys, keys]), edges, 0, 1)
    assert (table[1] == 2).all()
    check(g, table)
    path(g, not defer)
    g.close()
    # the same number of hashtest's integers into a fresh table
    g = new_graph(mcx, k, 1, defer=defer)
    g.hashtest(0, n)
    assert g.nkmers == n > nmain
    check(g, T.ref_table(T.integers(k, 0, n), np.zeros(n, np.uint8), 0, 1))
    path(g, not defer)
    g.close()


# ---- g. on top of other contents ------------------------------------------------------------------------------
def saturation_case(k):
    """1000 records of two colours, 200 of them 3 below the clamp in one colour; 10 tuples on each key, 5 per colour,
    among 5000 tuples of other keys"""
    rng = np.random.default_rng(7500 + k)
    rk = np.unique(T.random_keys(rng, k, 1000), axis=0)
    assert len(rk) == 1000
    rk = rk[rng.permutation(1000)]
    cov = rng.integers(1, 100, (1000, 2)).astype(np.uint32)
    cov[np.arange(200), rng.integers(0, 2, 200)] = U32 - 2
    edg = rng.integers(0, 256, (1000, 2), dtype=np.uint8)
    keys = np.concatenate([np.repeat(rk, 5, axis=0), T.random_keys(rng, k, 2500)])
    keys = np.concatenate([keys[rng.permutation(len(keys))], keys[rng.permutation(len(keys))]])  # first half: colour 0
    edges = T.random_edges(rng, len(keys))
    h = len(keys) // 2
    return (rk, cov, edg), keys, edges, [(0, h, 0), (h, 2 * h, 1)]


@pytest.mark.parametrize("k", [31, 63])
def test_saturation_input_passes_the_clamp(k):
    pre, keys, edges, calls = saturation_case(k)
    uk, cov, _ = T.ref_table(keys, edges, cols_of(len(keys), calls), 2, preload=pre)
    assert int((cov > U32).sum()) == 200 and int(cov.max()) == U32 - 2 + 5
    _, cc, _ = T.parse_body(T.pack_body(uk, cov, np.zeros_like(cov, dtype=np.uint8)), T.words(k), 2)
    assert int((cc == U32).sum()) == 200


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("defer", [1, 0])
def test_tuples_on_loaded_records_saturate(mcx, k, defer):
    pre, keys, edges, calls = saturation_case(k)
    g = new_graph(mcx, k, 2, defer=defer)
    g.add_records(T.pack_body(*pre), 2, [(0, 0), (1, 1)])
    insert_calls(g, keys, edges, calls)
    check(g, T.ref_table(keys, edges, cols_of(len(keys), calls), 2, preload=pre))
    path(g, not defer)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("defer", [1, 0])
def test_tuples_reads_tuples(mcx, orc, k, defer):
    """tuples, then reads that share keys with them, then tuples again: the read graph is the oracle's"""
    import synth
    bases, offs = synth.reads(1500, 120, genome_len=40000, seed=k)
    og = orc.Graph(k, 2, 1 << 18)
    og.add_reads(1, bases, offs)
    pre = T.parse_body(og.body_bytes(True), T.words(k), 2)
    rng = np.random.default_rng(7600 + k)
    rk = pre[0]
    assert len(rk) >= 20000
    keys = np.concatenate([rk[rng.integers(0, len(rk), 30000)], T.random_keys(rng, k, 10000)])
    keys = keys[rng.permutation(len(keys))]
    edges = T.random_edges(rng, len(keys))
    h = len(keys) // 2
    calls = [(0, h, 1), (h, len(keys), 0)]
    g = new_graph(mcx, k, 2, defer=defer)
    hold = []
    insert(g, 1, keys[:h], edges[:h], hold)
    g.add_reads(1, bases, offs)
    insert(g, 0, keys[h:], edges[h:], hold)
    g.sync()
    check(g, T.ref_table(keys, edges, cols_of(len(keys), calls), 2, preload=pre))
    prof = g.profile()
    assert ("k_insert_tuples" in prof) == (not defer) and ("k_tuples_bin" in prof) == bool(defer), prof
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("defer", [1, 0])
def test_tuples_over_tombstones(mcx, orc, k, defer):
    """`clean` leaves tombstones: tuples for the removed keys, for kept keys and for new ones"""
    from test_gpu_table_states import c_case
    ref = c_case(orc, k, "reads")
    W = T.words(k)
    k0 = T.parse_body(ref["body0"], W, 1)[0]
    kept = T.parse_body(ref["body1"], W, 1)
    kept_set = {r.tobytes() for r in kept[0]}
    removed = np.array([r for r in k0 if r.tobytes() not in kept_set], dtype=np.uint64).reshape(-1, W)
    assert len(removed) == ref["removed"] >= 200 and len(kept[0]) >= 500
    rng = np.random.default_rng(7650 + k)
    keys = np.concatenate([removed, removed[:100], kept[0][rng.integers(0, len(kept[0]), 500)], T.random_keys(rng, k, 300)])
    keys = keys[rng.permutation(len(keys))]
    edges = T.random_edges(rng, len(keys))
    g = new_graph(mcx, k, 1, defer=defer)
    g.add_reads(0, ref["bases"], ref["offs"])
    g.sync()
    st, _ = g.clean(2, 2 * k)
    assert st["nkmers_removed"] == ref["removed"]
    assert g.export(True) == ref["body1"]
    insert_calls(g, keys, edges, [(0, len(keys), 0)])
    check(g, T.ref_table(keys, edges, 0, 1, preload=kept))
    prof = g.profile()
    assert ("k_insert_tuples" in prof) == (not defer) and ("k_tuples_bin" in prof) == bool(defer), prof
    g.close()


# ---- h. the segments entry ---------------------------------------------------------------------------------------
def fills_of(nseg, seg_cap):
    """the fills of each call: 0, 1, seg_cap - 1, seg_cap and seg_cap + 5 (read as seg_cap)"""
    f = [0, 1, seg_cap - 1, seg_cap, seg_cap + 5]
    if nseg == 1:
        return [[x] for x in f]
    return [[seg_cap + 5, 0, 1, seg_cap - 1, seg_cap, seg_cap // 3, seg_cap + 5], [1, seg_cap, 0, seg_cap + 5, 0, seg_cap - 1, 0]]


LAYOUTS = [(nseg, seg_cap) for nseg in (1, 7) for seg_cap in (4097, 5000, 1001)]


@pytest.mark.parametrize("nseg,seg_cap", LAYOUTS)
def test_segment_fills_cover_the_edges(nseg, seg_cap):
    flat = [x for call in fills_of(nseg, seg_cap) for x in call]
    assert all(len(call) == nseg for call in fills_of(nseg, seg_cap))
    assert {0, 1, seg_cap - 1, seg_cap} <= set(flat) and max(flat) > seg_cap


def segment_calls(rng, k, nseg, seg_cap, ncols, poison):
    """-> [(colour, keys[nseg, seg_cap, W], edges[nseg, seg_cap], counts[nseg])], (all real tuples: keys, edges, cols):
    every slot beyond a segment's fill holds the poison key with edge byte 0xff"""
    W = T.words(k)
    calls, rk, re, rc = [], [], [], []
    pool = T.random_keys(rng, k, 3000)  # (keys repeat across segments and calls)
    for ci, fills in enumerate(fills_of(nseg, seg_cap)):
        colour = ci % ncols
        keys = np.tile(poison, (nseg, seg_cap, 1)).astype(np.uint64)
        edges = np.full((nseg, seg_cap), 0xFF, dtype=np.uint8)
        for s, f in enumerate(fills):
            m = min(f, seg_cap)
            keys[s, :m] = np.where(rng.random((m, 1)) < 0.5, pool[rng.integers(0, len(pool), m)], T.random_keys(rng, k, m))
            edges[s, :m] = T.random_edges(rng, m)
            rk.append(keys[s, :m].copy()); re.append(edges[s, :m].copy()); rc.append(np.full(m, colour))
        calls.append((colour, keys.reshape(nseg, seg_cap, W), edges, np.array(fills, dtype=np.uint64)))
    return calls, (np.concatenate(rk), np.concatenate(re), np.concatenate(rc))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("nseg,seg_cap", LAYOUTS)
def test_segments_entry(mcx, k, ncols, nseg, seg_cap):
    rng = np.random.default_rng(7800 + k + 7 * nseg + seg_cap)
    poison = T.random_keys(rng, k, 1)[0]
    calls, (rk, re, rc) = segment_calls(rng, k, nseg, seg_cap, ncols, poison)
    assert not (rk == poison).all(axis=1).any()
    g = new_graph(mcx, k, ncols, defer=1)
    hold = []
    for colour, keys, edges, counts in calls:
        bufs = (dev(keys), dev(edges), dev(counts))
        hold.append(bufs)
        g.insert_tuple_segments_dev(colour, *bufs, nseg, seg_cap)
    g.sync()
    table = T.ref_table(rk, re, rc, ncols)
    assert int(table[1].sum()) == sum(min(int(f), seg_cap) for c in calls for f in c[3])  # seg_cap + 5 inserts seg_cap
    check(g, table)
    assert not (g.records(True)[0] == poison).all(axis=1).any()
    path(g, False)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_segments_beyond_one_set_of_bins(mcx, k):
    """3 segments of 2^20 full slots against a window of 2^20 tuples per flush"""
    keys, edges = big_uniform(k)
    n = 3 << 20
    g = new_graph(mcx, k, 1, cap=1 << 22, defer=1)
    g.configure("defer_tuples", 1 << 20)
    bufs = (dev(keys), dev(edges), dev(np.full(3, 1 << 20, dtype=np.uint64)))
    g.insert_tuple_segments_dev(0, *bufs, 3, 1 << 20)
    g.sync()
    check(g, big_ref(k, n))
    path(g, False)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_full_region_bin_falls_back_to_the_direct_insert(mcx, k):
    """one block (grid_split = 1) appends to one replica of the region bins: with 2^20 tuples per flush over 512
    regions x 8 replicas a segment holds 2^20 / 4096 x 1.06 + 8192 = 8463 tuples, so at least 60 000 of the hot
    key's 70 000 occurrences find it full and take the direct insert"""
    keys, edges = key_set("hot", k)
    g = new_graph(mcx, k, 1, cap=1 << 22, defer=1)
    g.configure("defer_tuples", 1 << 20)
    g.configure("grid_split", 1)
    bufs = (dev(keys), dev(edges), dev(np.array([len(keys)], dtype=np.uint64)))
    g.insert_tuple_segments_dev(0, *bufs, 1, len(keys))
    g.sync()
    check(g, set_ref("hot", k, "one"))
    st = path(g, False)
    assert T.HOT - 10_000 <= st["fallback_inserts"] <= len(keys), st
    g.close()


def device_free(mcx):
    free, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
    L = mcx.lib()
    L.mcx_device_memory.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    assert L.mcx_device_memory(0, ctypes.byref(free), ctypes.byref(total)) == 0
    return int(free.value)


@pytest.mark.gpu
def test_segments_entry_refusals(mcx):
    seg_cap = 1001
    rng = np.random.default_rng(7900)
    for k, defer in ((31, 0), (63, 0), (95, None), (127, None)):
        W = T.words(k)
        bufs = (dev(T.random_keys(rng, k, seg_cap)), dev(T.random_edges(rng, seg_cap)), dev(np.array([seg_cap], dtype=np.uint64)))
        g = new_graph(mcx, k, 2, defer=defer)
        g.sync()
        before = device_free(mcx)
        with pytest.raises(mcx.McxError) as ei:
            g.insert_tuple_segments_dev(0, *bufs, 1, seg_cap)
        after = device_free(mcx)
        assert ei.value.code == mcx.graph.MCX_ERR_ARG
        assert "tuple segments need the deferred insert path (table too small or defer=0)" in str(ei.value)
        # a refusal allocates nothing (the deferred workspace of this table takes hundreds of MiB: 64 tuples per slot)
        assert before - after < (8 << 20), (k, before, after)
        assert g.nkmers == 0 and W == g.W
        g.close()
    g = new_graph(mcx, 31, 2, defer=1)
    bufs = (dev(T.random_keys(rng, 31, seg_cap)), dev(T.random_edges(rng, seg_cap)), dev(np.array([seg_cap], dtype=np.uint64)))
    for args in ((None, bufs[1], bufs[2]), (bufs[0], None, bufs[2]), (bufs[0], bufs[1], None)):
        with pytest.raises(mcx.McxError) as ei:
            g.insert_tuple_segments_dev(0, *args, 1, seg_cap)
        assert ei.value.code == mcx.graph.MCX_ERR_ARG and "null tuple buffers" in str(ei.value)
    for colour in (-1, 2):
        with pytest.raises(mcx.McxError) as ei:
            g.insert_tuple_segments_dev(colour, *bufs, 1, seg_cap)
        assert ei.value.code == mcx.graph.MCX_ERR_ARG and "colour %d out of range" % colour in str(ei.value)
    g.insert_tuple_segments_dev(0, *bufs, 0, seg_cap)  # no segments, no slots: fine, and nothing happens
    g.insert_tuple_segments_dev(1, *bufs, 1, 0)
    g.insert_tuple_segments_dev(0, None, None, None, 0, 0)
    g.sync()
    assert g.nkmers == 0 and g.export(True) == b""
    g.insert_tuple_segments_dev(1, *bufs, 1, seg_cap)  # (the handle still works)
    g.sync()
    assert g.nkmers == seg_cap
    g.close()


# ---- i. hashtest: which keys are in the table ------------------------------------------------------------------
H_N = 200_000


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 33, 63, 65, 95, 127])
@pytest.mark.parametrize("first", [0, (1 << 32) - 1000])
def test_hashtest_contents(mcx, k, first):
    W = T.words(k)
    g = new_graph(mcx, k, 1, cap=1 << 20)
    keys = T.integers(k, first, H_N)
    zero = np.zeros(H_N, dtype=np.uint8)
    for rounds in (1, 2):  # the second call finds every key: coverage 2, no new keys
        g.hashtest(first, H_N)
        assert g.nkmers == H_N
        nk, sc = g.kmer_covg()
        assert (nk.tolist(), sc.tolist()) == ([H_N], [rounds * H_N])
        want = T.pack_body(keys, np.full((H_N, 1), rounds, np.uint64), zero.reshape(-1, 1))
        # (at k = 33 and 65 the integers pass the top word's two key bits -- the reference inserts such BinaryKmers as
        # they are: the unsorted export, sorted here by whole words, is what is pinned at every k)
        assert T.sort_body(g.export(False), W, 1) == want
        if k not in (33, 65):
            assert g.export(True) == want
    path(g, k > 63)
    g.close()


@pytest.mark.gpu
def test_hashtest_across_its_key_chunk(mcx):
    """2^26 + 12345 keys: the second chunk of the entry's key buffer starts at first + 2^26"""
    n = (1 << 26) + 12345
    g = new_graph(mcx, 31, 1, cap=1 << 27)
    t0 = time.time()
    g.hashtest(0, n)
    print("hashtest of %d keys: %.2f s" % (n, time.time() - t0))
    assert g.nkmers == n
    nk, sc = g.kmer_covg()
    assert (nk.tolist(), sc.tolist()) == ([n], [n])
    assert g.covg_histogram(4).tolist() == [0, n, 0, 0]
    g.close()
