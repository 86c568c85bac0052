"""The tile tail of the 512-thread k_stream_bin (one-word keys, region bins of an unsharded table; csrc/mcx_defer.h).

The block sorts two neighbouring 4096-position tiles as one tile of 8192 positions and stages the sorted tuples in
LDS in rounds of 6656 (StreamLdsWide): ceil(n / 6656) rounds for a tile of n tuples, at least one.  The cases put
n on both sides of that threshold, at the sizes where nothing is staged, and past a region segment's capacity (the
tuples beyond it take the direct insert: in round 0, in round 1).

Every input is built once through the deferred path -- as an ASCII stream (mcx_graph_add_stream_dev) and in its
packed form (mcx_graph_add_packed_dev: the kernel variant the benchmark runs) -- and once with configure("defer", 0),
the fused kernel that bins nothing.  Sorted records, nkmers, device_stats and checksum must agree.  The same streams
go through the untouched 256-thread geometry (MCX_STREAM_T=256, read once per process: a child process, this file run
as a script).

The tuple counts per 8192-position tile are stated in CASES and checked with numpy, without a device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TILE = 8192    # positions per block iteration: two tiles of 4096
STAGE = 6656   # tuples per staging round
SLOTS = 1 << 20
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- streams --------------------------------------------------------------------------------------
def rand_read(rng, n):
    return bytes(rng.choice(ACGT, n))


def filler(rng, n):
    """n positions without a k-mer start for k >= 21: reads of 20 bases, runs of N, each ended by a newline"""
    out = bytearray()
    while len(out) < n:
        out += (rand_read(rng, 20) if rng.integers(2) else b"N" * 20) + b"\n"
    out = out[:n]
    out[n - 1:n] = b"\n"
    return bytes(out)


def tile_with(rng, n, k, positions=TILE):
    """`positions` stream positions that hold exactly n k-mer starts: one read of n + k - 1 bases, then filler"""
    read = rand_read(rng, n + k - 1) + b"\n" if n else b""
    assert len(read) < positions
    return read + filler(rng, positions - len(read))


def tuples_per_tile(stream, k):
    """k-mer starts in each 8192-position tile: position p starts one when bytes p .. p + k - 1 are all ACGT"""
    a = np.frombuffer(stream, np.uint8)
    run = np.concatenate([[0], np.cumsum(np.isin(a, ACGT))])
    starts = np.zeros(len(a), bool)
    if len(a) >= k:
        starts[:len(a) - k + 1] = run[k:] - run[:len(a) - k + 1] == k
    return np.bincount(np.nonzero(starts)[0] // TILE, minlength=-(-len(a) // TILE)).tolist()


def make(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "full_tile":  # one newline-free read: every position of the first tile starts a k-mer
        return rand_read(rng, TILE + 30)
    if name in ("n6655", "n6656", "n6657"):
        return tile_with(rng, int(name[1:]), 31) + tile_with(rng, 3000, 31)
    if name == "records151":  # the benchmark's shape: 150 bases and a newline
        return b"".join(rand_read(rng, 150) + b"\n" for _ in range(163))
    if name == "records151_n":  # ... and every seventh read holds an N
        reads = [bytearray(rand_read(rng, 150)) for _ in range(163)]
        for r in reads[::7]:
            r[int(rng.integers(150))] = ord("N")
        return b"".join(bytes(r) + b"\n" for r in reads)
    if name == "odd_tiles":  # three tiles of 4096: the second block iteration has an empty half
        return tile_with(rng, 5000, 31) + tile_with(rng, 2000, 31, positions=4096)
    if name == "short_stream":
        return rand_read(rng, 1000) + b"\n"
    if name == "no_tuples":  # reads shorter than k, runs of N
        return filler(rng, TILE + 2000)
    if name == "k21":  # lbq and the shifts differ; a one-round tile, a two-round tile, a rest
        return tile_with(rng, 6657, 21) + rand_read(rng, TILE + 20) + b"\n" + rand_read(rng, 500) + b"\n"
    # One k-mer past the capacity of its region's segment (10362 tuples, see CAP1): with one block (grid_stream = 1)
    # everything goes to one replica.  The hot tuples of a tile are sorted positions [o, o + c) of the tile, o = 0
    # when the tile holds nothing else.
    if name == "overflow_both_rounds":  # tile 0: 8192 hot, all fit; tile 1: 8192 hot, 2170 fit: 2170 .. 8191 overflow
        return b"C" * (2 * TILE + 30) + b"\n"
    if name == "overflow_round1":  # tile 0: 4799 others + 3362 hot; tile 1: 8192 hot, 7000 fit: 7000 .. 8191 overflow
        return rand_read(rng, 4829) + b"\n" + b"C" * (3362 + TILE + 30) + b"\n"
    raise KeyError(name)


# name: (k, tuples per 8192-position tile, configure() knobs)
ONE_BLOCK = {"grid_stream": 1, "defer_tuples": 1 << 22}
CASES = {
    "full_tile": (31, [8192, 0], {}),
    "n6655": (31, [6655, 3000], {}),
    "n6656": (31, [6656, 3000], {}),
    "n6657": (31, [6657, 3000], {}),
    "records151": (31, [6518, 6518, 6518, 6], {}),
    "records151_n": (31, [6304, 6329, 6278, 6], {}),
    "odd_tiles": (31, [5000, 2000], {}),
    "short_stream": (31, [970], {}),
    "no_tuples": (31, [0, 0], {}),
    "k21": (21, [6657, 8192, 480], {}),
    "overflow_both_rounds": (31, [8192, 8192, 0], ONE_BLOCK),
    "overflow_round1": (31, [4799 + 3362, 8192, 0], ONE_BLOCK),
}
# capacity of a region segment (mcx_api.hip, ensure_defer): 2^22 tuples per flush over 256 regions x 8 replicas,
# x 1.06, + 8192, rounded up to even; and of a sub-table bin of the split that follows: over 256 sub-tables, x 1.25,
# + 1024 -- more than the hot k-mer's occurrences, so every fallback insert counted is k_stream_bin's
CAP1 = (int((1 << 22) / 256 / 8 * 1.06) + 8192 + 1) & ~1
CAP2 = (int((1 << 22) / 256 * 1.25) + 1024 + 1) & ~1
# (lowest, highest) count of fallback inserts.  The bin is the region, not the k-mer: each of the r other tuples of
# overflow_round1's tile 0 that share the hot k-mer's region (1 in 256 of 4799) takes a place in the segment as well,
# the overflow then starts at sorted position 7000 - r of tile 1 -- in round 1 as long as r < 7000 - 6656
FALLBACK = {"overflow_both_rounds": (2 * 8192 - CAP1, 2 * 8192 - CAP1),
            "overflow_round1": (3362 + 8192 - CAP1, 3362 + 8192 - CAP1 + 7000 - STAGE - 1)}

_STREAMS = {}


def stream_of(name):
    if name not in _STREAMS:
        _STREAMS[name] = make(name)
    return _STREAMS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_hold_the_stated_tuples_per_tile(name):
    k, want, _ = CASES[name]
    s = stream_of(name)
    assert tuples_per_tile(s, k) == want
    if name.startswith("records151"):  # 151-byte records: at most 54 x 120 + 38 starts in 8192 positions -> one round
        assert all(len(r) == 150 for r in s.split(b"\n")[:-1]) and max(want) <= 6518 <= STAGE
    if name == "odd_tiles":
        assert 2 * 4096 < len(s) <= 3 * 4096
    if name == "short_stream":
        assert len(s) < 4096
    if name == "overflow_both_rounds":  # 8192 hot tuples are in the segment: of tile 1, sorted positions 2170 .. fall out
        assert CAP1 == 10362 and 0 < CAP1 - 8192 < STAGE < 8192 and 2 * 8192 <= CAP2
    if name == "overflow_round1":       # 3362 are in the segment: of tile 1, sorted positions 7000 .. fall out
        assert STAGE < CAP1 - 3362 == 7000 < 8192 and 3362 + 8192 <= CAP2
        assert b"C" * 31 not in s[:4829]


def test_rounds_per_tile():
    """what the cases ask of the round count: tiles of 0, < 6656, exactly 6656, 6657 and 8192 tuples"""
    counts = sorted({n for _, per_tile, _ in CASES.values() for n in per_tile})
    assert {0, 6655, 6656, 6657, 8192} <= set(counts)
    assert [max(1, -(-n // STAGE)) for n in (0, 6655, 6656, 6657, 8192)] == [1, 1, 1, 2, 2]


# ---- builds -----------------------------------------------------------------------------------------
def build(mcx, name, how):
    """how: "direct" (defer 0), "ascii" or "packed" (deferred) -> what the builds must agree on"""
    import torch
    k, _, knobs = CASES[name]
    s = stream_of(name)
    g = mcx.Graph(k, 1, SLOTS)
    g.configure("defer", 0 if how == "direct" else 1)
    if how != "direct":
        for key, value in knobs.items():
            g.configure(key, value)
    t = torch.frombuffer(bytearray(s + b"\n" * 64), dtype=torch.uint8).cuda()
    if how == "packed":
        nch = (len(s) + 15) // 16
        code = torch.zeros(nch + 8, dtype=torch.int32, device="cuda")
        inv = torch.zeros(nch + 8, dtype=torch.int16, device="cuda")
        mcx.pack_stream_dev(t, len(s), code, inv)
        torch.cuda.synchronize()
        g.add_packed_dev(0, code, inv, len(s))
    else:
        g.add_stream_dev(0, t, len(s))
    g.sync()
    st = g.device_stats()
    res = {"body": g.export(True).hex(), "nkmers": int(g.nkmers), "loaded": int(st.num_kmers_loaded),
           "contigs": int(st.contigs_parsed), "checksum": [int(x) for x in g.checksum()], "insert": g.insert_stats()}
    g.close()
    return res


SAME = ("body", "nkmers", "loaded", "contigs", "checksum")
_REF = {}


def reference(mcx, name):
    """the fused kernel's graph of a case, built once"""
    if name not in _REF:
        ref = build(mcx, name, "direct")
        k, per_tile, _ = CASES[name]
        assert ref["insert"]["flushes"] == 0  # nothing was binned
        assert ref["loaded"] == sum(per_tile)
        assert ref["checksum"] == [mcx.records_checksum(bytes.fromhex(ref["body"]), k, 1), ref["nkmers"]]
        _REF[name] = ref
    return _REF[name]


def check(name, got, ref):
    for key in SAME:
        assert got[key] == ref[key], (name, key)
    ins = got["insert"]
    assert (ins["flushes"] >= 1 or not ref["loaded"]) and ins["foreign_inserts"] == 0, ins  # the deferred path ran
    lo, hi = FALLBACK.get(name, (0, 0))
    assert lo <= ins["fallback_inserts"] <= hi, ins


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["ascii", "packed"])
@pytest.mark.parametrize("name", list(CASES))
def test_stream_tail_matches_the_direct_build(mcx, name, how):
    check(name, build(mcx, name, how), reference(mcx, name))


def child(out):
    sys.path.insert(0, ROOT)
    import mccortex_amd as mcx
    res = {}
    for name in CASES:
        r = build(mcx, name, "ascii")
        r["body"] = mcx.records_checksum(bytes.fromhex(r["body"]), CASES[name][0], 1)  # (the records, in short)
        res[name] = r
    json.dump(res, open(out, "w"))


@pytest.mark.gpu
def test_same_streams_through_the_256_thread_geometry(mcx, tmp_path):
    """MCX_STREAM_T=256: 4096-position tiles, two fixed rounds of 2048, BinLds as before"""
    out = tmp_path / "t256.json"
    env = dict(os.environ, MCX_STREAM_T="256")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    res = json.load(open(out))
    for name in CASES:
        ref = dict(reference(mcx, name))
        ref["body"] = ref["checksum"][0]
        got = res[name]
        for key in SAME:
            assert got[key] == ref[key], (name, key)
        assert got["insert"]["flushes"] >= 1 or not ref["loaded"]
        if name in FALLBACK:  # tiles of 4096: the same tuples are past the segment's capacity
            assert FALLBACK[name][0] <= got["insert"]["fallback_inserts"] <= FALLBACK[name][1]


if __name__ == "__main__":
    child(sys.argv[1])
