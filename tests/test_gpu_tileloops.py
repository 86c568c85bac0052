"""The build kernels' grid-stride loops and bin-count instances against the C oracle, byte for byte.

At the default grid (CUs x 8 blocks, 4x that for the split and the LDS insert) every block of a small test
build runs ONE iteration of its kernel's loop, and tables below 2^32 slots never get more than 512 regions.
So what happens between iterations -- the next tile / slice fetched early, the barrier skipped on purpose,
the empty half of the 512-thread k_stream_bin, the split's two work orders, k_lds_insert stepping over
empty bins -- and the 1024 / 2048-bin instances of k_stream_bin, k_tuples_bin and k_superk_bin were only
reached by the slow full-size checksums.  Here mcx_graph_configure("grid", n) caps the launches at a few
blocks, so every block walks many tiles, and MCX_LB1 forces the region count of a small table, so the
large-bin instances run on reads of a few MB.  Every case is compared with orc.Graph: the sorted export,
the unsorted export as a record set, nkmers and the device_stats counters."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096  # stream positions per tile of the stream kernels (kThreads x kPosPerLane)
STATS = ("num_good_reads", "num_bad_reads", "total_bases_loaded", "contigs_parsed", "num_kmers_loaded", "num_kmers_novel")
DEV_STATS = ("contigs_parsed", "num_kmers_loaded", "num_kmers_novel")  # (what a device stream entry counts)


# ---- inputs and the oracle -----------------------------------------------------------------------
def _jobs(ncols, nreads, seed, genome_len=150_000):
    """ragged reads (lengths 0 .. 239) with Ns and lower case, one job per colour and a last one in colour 0
    (a colour switch), sized so that the jobs' streams hold odd as well as even numbers of tiles"""
    g0 = synth.genome(genome_len, seed)
    jobs = []
    parity = lambda b, o: -(-(len(b) + len(o) - 1) // TILE) % 2  # (tiles of the job's stream: bases + separators)
    for i in range(ncols + 1):
        n = nreads // (ncols + 1) + 997 * i
        while True:
            b, o = synth.reads(n, 120, seed=seed + 11 * i, g=g0, n_frac=0.05, lower_frac=0.1, var_len=True)
            if i < ncols or parity(b, o) != parity(*jobs[0][1:]):  # the last job takes the other parity than the first
                break
            n += 17
        jobs.append((i % ncols, b, o))
    return jobs


_ORACLES = {}


def _oracle(orc, k, ncols, nreads, seed):
    """(sorted body, summed stats, nkmers) of the oracle build, once per input"""
    key = (k, ncols, nreads, seed)
    if key not in _ORACLES:
        og = orc.Graph(k, ncols, 1 << 22)
        tot = dict.fromkeys(STATS, 0)
        for col, b, o in _jobs(ncols, nreads, seed):
            st = og.add_reads(col, b, o)
            for f in STATS:
                tot[f] += getattr(st, f)
        _ORACLES[key] = (og.body_bytes(True), tot, og.nkmers)
        assert og.nkmers > 50_000
    return _ORACLES[key]


def _recset(body, rs):
    return np.sort(np.frombuffer(body, np.uint8).reshape(-1, rs).copy().view("V%d" % rs).ravel())


def _check(g, want, stats, nk, what, fields=STATS):
    """the four comparisons of every case in this file"""
    assert g.nkmers == nk, what
    body = g.export(True)
    assert len(body) == len(want), what
    assert body == want, what
    rs = 8 * g.W + 5 * g.ncols
    assert np.array_equal(_recset(g.export(False), rs), _recset(want, rs)), what
    st = g.device_stats()
    for f in fields:
        assert getattr(st, f) == stats[f], (what, f)


def _feed(mcx, g, jobs, entry):
    import torch
    keep = []  # (the launches read the device buffers on the graph's stream until the sync below)
    for col, b, o in jobs:
        if entry == "add_reads":
            g.add_reads(col, b, o)
            continue
        stream = torch.from_numpy(synth.to_stream(b, o)).cuda()
        n = stream.numel()
        keep.append(stream)
        if entry == "add_stream_dev":
            g.add_stream_dev(col, stream, n)
        else:
            code = torch.empty((n + 15) // 16, dtype=torch.int32, device="cuda")
            inv = torch.empty((n + 15) // 16, dtype=torch.int16, device="cuda")
            keep += [code, inv]
            mcx.pack_stream_dev(stream, n, code, inv)
            torch.cuda.synchronize()
            g.add_packed_dev(col, code, inv, n)
    g.sync()


def _build(mcx, k, ncols, jobs, cfg, entry="add_reads", cap=1 << 20, devices=None):
    g = mcx.Graph(k, ncols, cap, devices=devices)
    for key, v in cfg.items():
        g.configure(key, v)
    g.configure("profile", 1)
    _feed(mcx, g, jobs, entry)
    return g


# ---- a. grid sweep of the one-device paths -------------------------------------------------------
GRID_CFGS = (
    [{"grid": n} for n in (1, 2, 3, 8)]
    + [{"defer": 0, "grid": n} for n in (1, 3)]
    # (grid_stream, grid_split, grid_insert): the split's XCD-aware order needs a multiple of 8 blocks
    + [{"grid": 1, "grid_stream": s, "grid_split": p, "grid_insert": i} for s, p, i in ((8, 16, 8), (3, 5, 3), (5, 3, 7), (2, 8, 5))]
    # several flushes: k_lds_insert loops over sub-tables that already hold data, and over empty bins
    + [{"grid": 2, "defer_tuples": 1 << 20}, {"grid": 8, "defer_tuples": 1 << 20, "flush_regions": 3}]
)


@pytest.mark.parametrize("k,ncols", [(31, 1), (31, 3), (63, 1), (63, 3), (21, 1), (21, 3)])
def test_grid_sweep_add_reads(mcx, orc, k, ncols):
    nreads, seed = 40_000, 100 + k + ncols
    want, stats, nk = _oracle(orc, k, ncols, nreads, seed)
    jobs = _jobs(ncols, nreads, seed)
    for cfg in GRID_CFGS:
        g = _build(mcx, k, ncols, jobs, cfg)
        _check(g, want, stats, nk, cfg)
        prof = g.profile()
        if cfg.get("defer", 1):
            assert "k_lds_insert" in prof and "k_tuples_bin" in prof, (cfg, prof)
            if "defer_tuples" in cfg:
                assert g.insert_stats()["flushes"] >= 3, cfg
        else:
            assert "k_stream" in prof and "k_lds_insert" not in prof, (cfg, prof)
        g.close()


@pytest.mark.parametrize("entry", ["add_stream_dev", "add_packed_dev"])
@pytest.mark.parametrize("k,ncols", [(31, 1), (63, 3), (21, 1)])
def test_grid_sweep_device_streams(mcx, orc, k, ncols, entry):
    nreads, seed = 30_000, 200 + k + ncols
    want, stats, nk = _oracle(orc, k, ncols, nreads, seed)
    jobs = _jobs(ncols, nreads, seed)
    for cfg in ({"grid": 1}, {"grid": 3}, {"defer": 0, "grid": 1}, {"grid": 2, "defer_tuples": 1 << 20},
                {"grid": 1, "grid_stream": 5, "grid_split": 8, "grid_insert": 3}):
        g = _build(mcx, k, ncols, jobs, cfg, entry)
        _check(g, want, stats, nk, (entry, cfg), DEV_STATS)
        g.close()


@pytest.mark.parametrize("k,ncols", [(31, 1), (63, 2)])
def test_sparse_flushes_over_many_sub_tables(mcx, orc, k, ncols):
    """small batches into 8 K - 16 K sub-tables, each flushed by a scan: most sub-table bins are empty, so the few
    insert blocks step over them (next_bin), and later flushes apply to sub-tables that already hold data"""
    g0 = synth.genome(100_000, k)
    jobs = [(i % ncols, *synth.reads(300 + 7 * i, 120, seed=40 + i, g=g0, n_frac=0.05, lower_frac=0.1, var_len=True)) for i in range(6)]
    og = orc.Graph(k, ncols, 1 << 20)
    tot = dict.fromkeys(STATS, 0)
    for col, b, o in jobs:
        st = og.add_reads(col, b, o)
        for f in STATS:
            tot[f] += getattr(st, f)
    want = og.body_bytes(True)
    for grid in (1, 3):
        g = mcx.Graph(k, ncols, 1 << 25)
        g.configure("grid", grid)
        for col, b, o in jobs:
            g.add_reads(col, b, o)
            g.checksum()  # (flushes the bins)
        assert g.insert_stats()["flushes"] >= len(jobs)
        _check(g, want, tot, og.nkmers, grid)
        g.close()


CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
import mccortex_amd as mcx
k, ncols, grid, defer, src, dst = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
z = np.load(src)
g = mcx.Graph(k, ncols, 1 << 20)
g.configure("grid", grid)
g.configure("defer", defer)
g.configure("profile", 1)
for i in range(len(z.files) // 3):
    g.add_reads(int(z["c%%d" %% i]), z["b%%d" %% i], z["o%%d" %% i])
g.sync()
st = g.device_stats()
np.savez(dst, sorted=np.frombuffer(g.export(True), np.uint8), unsorted=np.frombuffer(g.export(False), np.uint8),
         nkmers=g.nkmers, stats=np.array([getattr(st, f) for f in %r], np.uint64), copies=g.profile()["k_stream_bin" if defer else "k_stream"][0])
g.close()
'''


@pytest.mark.parametrize("k,ncols", [(31, 1), (63, 3)])
def test_small_staging_chunks(mcx, orc, tmp_path, k, ncols):
    """the host entry with 64 KiB staging chunks: one mcx_graph_add_reads call becomes many launches, each a range
    of positions that starts and ends inside a tile (MCX_STAGE_BYTES is read once per process: a child process)"""
    nreads, seed = 20_000, 300 + k
    want, stats, nk = _oracle(orc, k, ncols, nreads, seed)
    jobs = _jobs(ncols, nreads, seed)
    src = tmp_path / "jobs.npz"
    np.savez(src, **{("%s%d" % (n, i)): v for i, (c, b, o) in enumerate(jobs) for n, v in (("c", np.int64(c)), ("b", b), ("o", o))})
    env = dict(os.environ, MCX_STAGE_BYTES=str(64 << 10))
    for grid, defer in ((1, 1), (3, 1), (2, 0)):
        dst = tmp_path / ("out%d%d.npz" % (grid, defer))
        p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, STATS), str(k), str(ncols), str(grid), str(defer), str(src), str(dst)],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        r = np.load(dst)
        assert int(r["nkmers"]) == nk
        assert r["sorted"].tobytes() == want
        rs = 8 * ((2 * k + 63) // 64) + 5 * ncols
        assert np.array_equal(_recset(r["unsorted"].tobytes(), rs), _recset(want, rs))
        assert [int(x) for x in r["stats"]] == [stats[f] for f in STATS]
        assert int(r["copies"]) > 2 * len(jobs)  # (several launches per call)


# ---- b. wide keys: the loop of k_stream<W = 3, 4> (the only path for k = 65 .. 127) -----------------
@pytest.mark.parametrize("k,ncols", [(65, 1), (95, 3), (127, 1)])
def test_wide_keys_capped_grid(mcx, orc, k, ncols):
    nreads, seed = 20_000, 400 + k
    want, stats, nk = _oracle(orc, k, ncols, nreads, seed)
    jobs = _jobs(ncols, nreads, seed)
    for grid in (1, 3):
        for entry in ("add_reads", "add_stream_dev"):
            g = _build(mcx, k, ncols, jobs, {"grid": grid}, entry)
            _check(g, want, stats, nk, (grid, entry), STATS if entry == "add_reads" else DEV_STATS)
            assert "k_stream" in g.profile()
            g.close()


# ---- c. sharded tables: k_stream_superk, k_superk_bin, the sender and owner sides -------------------
@pytest.mark.parametrize("k,ndev,xch", [(31, 2, "v3"), (31, 4, "v3"), (63, 2, "v3"), (31, 2, "v2"), (31, 4, "v2"), (21, 4, "v2"), (63, 2, "v2")])
def test_sharded_capped_grid(mcx, orc, k, ndev, xch, monkeypatch):
    monkeypatch.setenv("MCX_MULTI_EXCHANGE", xch)
    ncols = 3 if ndev == 2 else 1
    nreads, seed = 30_000, 500 + k + ndev
    want, stats, nk = _oracle(orc, k, ncols, nreads, seed)
    jobs = _jobs(ncols, nreads, seed)
    for grid in (1, 3):
        g = _build(mcx, k, ncols, jobs, {"grid": grid}, devices=[0] * ndev)
        _check(g, want, stats, nk, grid)
        cs, n = g.checksum()
        assert n == nk and cs == mcx.records_checksum(want, k, ncols)
        prof = g.profile()
        assert any(name.startswith("k_superk_bin" if xch == "v3" else "k_stream_bin") for name in prof), prof
        g.close()


# ---- d. geometry: 1024 and 2048 bins in k_stream_bin, the split and k_superk_bin ----------------------
SUB_SLOTS = {1: 4096, 2: 2048}


def _region_bits(nsub, lbo=0):
    """mcx_api.hip region_bits: up to 512 regions (2048 / shards for a hash-prefix shard), more for huge tables"""
    lb1, lb1_max = 0, (min(9, 11 - lbo) if lbo else 9)
    while lb1 < lb1_max and (2 << lb1) <= nsub:
        lb1 += 1
    while lb1 < 11 and -(-nsub // (1 << lb1)) > 2048:
        lb1 += 1
    return lb1


def _slots(nsub, lb1, W):
    """slots of a table of nsub sub-tables in 2^lb1 regions: nsub rounded up to spb << lb1, plus the overflow area"""
    ss = SUB_SLOTS[W]
    n = -(-nsub // (1 << lb1)) << lb1
    return n * ss + max(ss, -(-n // 32) * ss)


def _forced(nsub, lb1, W):
    """capacity and slot count of a table forced to 2^lb1 regions, checked to differ from the default geometry's
    (a knob that is silently ignored must fail the test)"""
    want = _slots(nsub, lb1, W)
    assert want != _slots(nsub, _region_bits(nsub), W)
    return nsub * SUB_SLOTS[W], want


# (k, colours, MCX_LB1, sub-tables, grid): region bins 2^lb1; sub-table bins spb = ceil(nsub / 2^lb1)
GEOMETRY = [
    (31, 1, 10, 1100, 0), (31, 3, 10, 1100, 2), (63, 1, 10, 1100, 0), (45, 3, 10, 1100, 0),    # 1024 region bins
    (31, 1, 11, 2100, 3), (31, 3, 11, 2100, 0), (63, 1, 11, 2100, 0), (63, 3, 11, 2100, 3),    # 2048 region bins
    (31, 1, 6, 64 * 600 + 1, 1), (31, 3, 6, 64 * 600 + 1, 0), (63, 1, 6, 64 * 600 + 1, 2), (45, 3, 6, 64 * 600 + 1, 0),  # 601
    (31, 1, 6, 64 * 1200 + 1, 2), (31, 3, 6, 64 * 1200 + 1, 0), (63, 1, 6, 64 * 1200 + 1, 0), (63, 3, 6, 64 * 1200 + 1, 0),  # 1201
]


@pytest.mark.parametrize("k,ncols,lb1,nsub,grid", GEOMETRY)
def test_forced_geometry(mcx, orc, k, ncols, lb1, nsub, grid, monkeypatch):
    monkeypatch.setenv("MCX_LB1", str(lb1))
    W = (2 * k + 63) // 64
    cap, slots = _forced(nsub, lb1, W)
    nreads, seed = 30_000, 600 + k + ncols
    want, stats, nk = _oracle(orc, k, ncols, nreads, seed)
    jobs = _jobs(ncols, nreads, seed)
    cfg = {"defer_tuples": 1 << 22}  # (the default flush window of a table this size would take tens of GB)
    if grid:
        cfg["grid"] = grid
    g = _build(mcx, k, ncols, jobs, cfg, cap=cap)
    assert g.capacity()[0] == slots
    _check(g, want, stats, nk, cfg)
    prof = g.profile()
    assert "k_stream_bin" in prof and "k_tuples_bin" in prof and "k_lds_insert" in prof, prof
    g.close()


@pytest.mark.parametrize("k,lb1,nsub,grid", [(31, 10, 1100, 1), (31, 11, 2100, 0), (63, 11, 2100, 3)])
def test_forced_geometry_superk_exchange(mcx, orc, k, lb1, nsub, grid, monkeypatch):
    """exchange format v3 builds ordinary per-device tables: MCX_LB1 gives their k_superk_bin 1024 / 2048 region bins"""
    monkeypatch.setenv("MCX_LB1", str(lb1))
    monkeypatch.setenv("MCX_MULTI_EXCHANGE", "v3")
    W = (2 * k + 63) // 64
    cap, slots = _forced(nsub, lb1, W)
    nreads, seed = 30_000, 700 + k
    want, stats, nk = _oracle(orc, k, 1, nreads, seed)
    jobs = _jobs(1, nreads, seed)
    cfg = {"defer_tuples": 1 << 22}
    if grid:
        cfg["grid"] = grid
    g = _build(mcx, k, 1, jobs, cfg, cap=2 * cap, devices=[0, 0])
    assert g.capacity()[0] == 2 * slots
    _check(g, want, stats, nk, cfg)
    assert any(name.startswith("k_superk_bin") for name in g.profile())
    g.close()


@pytest.mark.parametrize("k,grid", [(31, 0), (31, 3), (63, 1)])
def test_hash_prefix_shards_with_2048_owner_region_bins(mcx, orc, k, grid, monkeypatch):
    """exchange format v2 sends by (owner, region): 4 shards of >= 1024 sub-tables each have 512 regions, so the
    sender's k_stream_bin runs with 4 x 512 = 2048 bins (MCX_LB1 does not apply to hash-prefix shards)"""
    monkeypatch.setenv("MCX_MULTI_EXCHANGE", "v2")
    W = (2 * k + 63) // 64
    nsub = 1100
    lb1 = _region_bits(nsub, lbo=2)
    assert lb1 == 9
    nreads, seed = 30_000, 800 + k
    want, stats, nk = _oracle(orc, k, 1, nreads, seed)
    jobs = _jobs(1, nreads, seed)
    cfg = {"grid": grid} if grid else {}
    g = _build(mcx, k, 1, jobs, cfg, cap=4 * nsub * SUB_SLOTS[W], devices=[0, 0, 0, 0])
    assert g.capacity()[0] == 4 * _slots(nsub, lb1, W)
    _check(g, want, stats, nk, cfg)
    g.close()


# ---- e. inferedges and the table scans under a capped grid ---------------------------------------------
@pytest.mark.parametrize("k,ncols", [(31, 3), (63, 1), (95, 2)])
def test_infer_edges_capped_grid(mcx, k, ncols):
    import torch
    from test_gpu_inferedges import expect_file, pack, random_graph
    recs = random_graph(random.Random(k + ncols), k, ncols, 3000)
    body = pack(recs, k, ncols)
    for grid in (1, 3):
        g = mcx.Graph(k, ncols, 1 << 14)
        g.configure("grid", grid)
        g.add_records(body, ncols, [(c, c) for c in range(ncols)])
        for pop in (False, True):
            exp, nmod, _ = expect_file(recs, k, ncols, pop)
            got, n = g.infer_edges(body, pop=pop)
            assert got == pack(exp, k, ncols) and n == nmod, (grid, pop)
        exp, nmod, _ = expect_file(recs, k, ncols, False)
        d = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to("cuda:0")
        assert g.infer_edges_dev(d, len(recs)) == nmod
        assert d.cpu().numpy().tobytes() == pack(exp, k, ncols)
        g.close()


@pytest.mark.parametrize("k,ncols", [(31, 1), (63, 3)])
def test_scans_after_grid_one_build(mcx, orc, k, ncols):
    """checksum, kmer_covg and covg_histogram walk the table in grid-stride loops too: with one block"""
    nreads, seed = 30_000, 900 + k
    want, stats, nk = _oracle(orc, k, ncols, nreads, seed)
    jobs = _jobs(ncols, nreads, seed)
    g = _build(mcx, k, ncols, jobs, {"grid": 1})
    _check(g, want, stats, nk, "grid 1")
    W = g.W
    rec = np.frombuffer(want, np.uint8).reshape(-1, 8 * W + 5 * ncols)
    cov = rec[:, 8 * W:8 * W + 4 * ncols].copy().view(np.uint32).astype(np.uint64)
    cs, n = g.checksum()
    assert n == nk and cs == mcx.records_checksum(want, k, ncols)
    nkc, sc = g.kmer_covg()
    assert list(nkc) == list((cov > 0).sum(axis=0)) and list(sc) == list(cov.sum(axis=0))
    for nbins in (8, 5000):  # (bins beyond the 4096 kept in LDS go straight to HBM)
        tot = np.minimum(cov.sum(axis=1), 0xFFFFFFFF)
        assert list(g.covg_histogram(nbins)) == list(np.bincount(np.minimum(tot, nbins - 1).astype(np.int64), minlength=nbins))
    g.close()
