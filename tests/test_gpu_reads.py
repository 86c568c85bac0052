"""`reads` on the MI355X (Graph.reads_touch*, csrc/mcx_reads.h) against the CPU restatement in reads_restate.py: the
byte of every read, and the two k-mer counts.  The cases are built on the CPU (the functions named case_*), where each
first asserts on the restatement alone what it is there to exercise; the shapes are the smallest that reach every
branch: k = 9, 31, 63, 95, 127 (keys of one to four words), batches of a few tiles of 4096 positions."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_restate as R  # noqa: E402
import reads_restate as S  # noqa: E402
import mccortex_amd as mcx  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (9, 31, 63, 95, 127)
TILE = 4096
LONG_STARTS = 4096  # kRtLongStarts of mcx_reads.h: a read with more start positions is ORed by a wave


def rseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def hits(keys, k, seq):
    return [x in keys for x in S.read_kmers(k, seq)]


def junk(rng, keys, k, n):
    """a random sequence of n bases with no k-mer in keys"""
    for _ in range(10000):
        s = rseq(rng, n)
        if not S.touches(keys, k, s):
            return s
    raise AssertionError("no junk found")


def odd(n):
    return n if n % 16 else n + 3


def genome_keys(rng, k, n=2000):
    g = rseq(rng, n + k - 1)
    return g, S.keys_of([g], k)


def load(keys, k, cap=1 << 16):
    g = mcx.Graph(k, 1, cap)
    g.add_records(R.pack({key: ((1,), [0]) for key in keys}, k, 1), 1, [(0, 0)])
    g.sync()
    assert g.nkmers == len(keys)
    return g


def arrays(reads):
    seqs = [s.encode() for s in reads]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) or b"\n", dtype=np.uint8), offs


def expect(keys, k, reads):
    return [int(S.touches(keys, k, s)) for s in reads], S.counts(keys, k, reads)


def check(g, keys, k, reads, exp=None, what=""):
    bytes_, (nk, nf) = exp or expect(keys, k, reads)
    hit, st = g.reads_touch(*arrays(reads))
    print("reads k=%d %s: %s (expected %d hit, %d / %d k-mers)" % (k, what, st.as_dict(), sum(bytes_), nf, nk))
    assert hit.dtype == np.uint8 and hit.tolist() == bytes_
    assert st.as_dict() == {"num_reads": len(reads), "num_reads_hit": sum(bytes_), "num_kmers": nk, "num_kmers_found": nf}
    return hit


# ---- cases (CPU only) ---------------------------------------------------------------------------------------------
def case_classes(k):
    """(keys, reads): every class of read, reads that must not leak into each other, and random reads of which between
    10 % and 90 % hit"""
    rng = random.Random(4100 + k)
    g, keys = genome_keys(rng, k)
    ch, fl = (k + 1) // 2, k // 2
    # a key made of the end of read A and the start of read B, and one made of the two sides of an N: planted first, so
    # that everything drawn afterwards is drawn against the final key set
    a, b = junk(rng, keys, k, odd(k + 21)), junk(rng, keys, k, odd(k + 9))
    n1, n2 = junk(rng, keys, k, odd(k + 5)), junk(rng, keys, k, k + 2)
    planted = {S.read_kmers(k, a[-ch:] + b[:fl])[0], S.read_kmers(k, n1[-ch:] + n2[:fl])[0]}
    assert not planted & keys
    keys = keys | planted
    across_n = n1 + "N" + n2
    for s in (a, b, across_n):
        assert not S.touches(keys, k, s)
    assert S.touches(keys, k, a + b) and S.touches(keys, k, n1 + n2)
    cls = {}
    p = 100
    for _ in range(10000):  # only its first / only its last k-mer
        first = g[p:p + k] + rseq(rng, 25)
        last = rseq(rng, 22) + g[p + 300:p + 300 + k]
        if hits(keys, k, first) == [True] + [False] * 25 and hits(keys, k, last) == [False] * 22 + [True]:
            break
    else:
        raise AssertionError
    cls["first"], cls["last"] = first, last
    for q in range(500, 1500):  # the read's own k-mer is not the key: found only as its reverse complement
        r = rc(g[q:q + k])
        if S.kmer_int(g[q:q + k]) == S.read_kmers(k, r)[0] != S.kmer_int(r):
            break
    else:
        raise AssertionError
    cls["revcomp"] = r
    cls["second_run"] = junk(rng, keys, k, k + 4) + "N" + g[700:700 + k + 3]
    assert hits(keys, k, cls["second_run"]) == [False] * 5 + [True] * 4
    cls["short"], cls["empty"], cls["all_n"], cls["lower"] = g[50:50 + k - 1], "", "N" * (2 * k), g[900:900 + 2 * k].lower()
    want = {"first": 1, "last": 1, "revcomp": 1, "second_run": 1, "short": 0, "empty": 0, "all_n": 0, "lower": 1}
    for name, w in want.items():
        assert cls[name] is not None and int(S.touches(keys, k, cls[name])) == w, name
    # a hitting read between two that do not hit, none a multiple of 16 long
    left, mid, right = junk(rng, keys, k, odd(k + 30)), g[1200:1200 + odd(k + 17)], junk(rng, keys, k, odd(k + 2))
    assert all(len(s) % 16 for s in (left, mid, right, a, b, n1))
    reads = [a, b, across_n] + list(cls.values()) + [left, mid, right]
    for i in range(120):
        if i % 2:
            reads.append(rseq(rng, rng.randrange(k, k + 60)))
        else:
            q = rng.randrange(0, len(g) - k - 60)
            s = list(g[q:q + rng.randrange(k, k + 60)])
            if i % 4 == 0:
                s = [c if rng.random() > 0.02 else "N" for c in s]
            s = "".join(s)
            reads.append(rc(s) if i % 8 < 4 else s)
    frac = sum(S.touches(keys, k, s) for s in reads) / len(reads)
    assert 0.1 <= frac <= 0.9, frac
    return keys, reads


def case_tiles(k):
    """(keys, reads) of four tiles and a bit: junk reads, with one planted key that starts on the last position of tile
    0, one whose window crosses from tile 1 into tile 2, and a read whose last base is the last position of tile 2"""
    rng = random.Random(5200 + k)
    reads, pos = [], 0  # pos = stream position of the next read (every read is followed by one separator)

    def add(n):
        nonlocal pos
        reads.append(rseq(rng, n))
        pos += n + 1
        return len(reads) - 1, pos - n - 1

    def fill_to(target):  # junk reads until the next read starts at `target`
        while pos < target:
            left = target - pos
            add(left - 1 if left <= 2 * k + 80 else rng.randrange(k, k + 60))
        assert pos == target

    fill_to(TILE - 1 - 37)
    x, x0 = add(2 * k + 60)            # its k-mer at read offset 37 starts on position 4095
    fill_to(2 * TILE - k + 3 - 11)
    y, y0 = add(2 * k + 41)            # its k-mer at offset 11 starts k - 3 positions before tile 2: the window crosses
    fill_to(3 * TILE - (k + 29))
    z, z0 = add(k + 29)                # ends on 3 * 4096 - 1; its last k-mer is the key
    assert z0 + len(reads[z]) == 3 * TILE
    zn, _ = add(odd(k + 8))
    fill_to(4 * TILE + 300)
    planted = {x: 37, y: 11, z: 29}
    starts = {x: x0 + 37, y: y0 + 11, z: z0 + 29}
    assert starts[x] == TILE - 1 and starts[y] + k > 2 * TILE > starts[y] and starts[z] + k == 3 * TILE
    keys = {S.read_kmers(k, reads[i][o:o + k])[0] for i, o in planted.items()}
    # a third of the other reads hit as well (one k-mer each), so that 10 % .. 90 % do
    for i in range(0, len(reads), 3):
        if i not in planted and i != zn and len(reads[i]) >= k:
            keys.add(S.read_kmers(k, reads[i])[-1])
    for i, o in planted.items():
        h = hits(keys, k, reads[i])
        assert h[o] and sum(h) == 1, (i, o)
    assert not S.touches(keys, k, reads[zn])
    frac = sum(S.touches(keys, k, s) for s in reads) / len(reads)
    assert 0.1 <= frac <= 0.9 and pos >= 3 * TILE, frac
    return keys, reads


def case_long(k):
    """(keys, reads): one read of more start positions than a lane takes, its only hit near its end, between short reads"""
    rng = random.Random(6300 + k)
    long_read = rseq(rng, LONG_STARTS + 1500 + k)
    at = len(long_read) - k - 5
    keys = {S.read_kmers(k, long_read[at:at + k])[0]}
    h = hits(keys, k, long_read)
    assert len(h) > LONG_STARTS and sum(h) == 1 and h[at]
    # a second long read that does not hit, and one that hits in its first word only
    quiet = junk(rng, keys, k, LONG_STARTS + 200 + k)
    early = long_read[at:at + k] + quiet[:LONG_STARTS + 77]
    assert hits(keys, k, early)[0]
    shorts = [junk(rng, keys, k, odd(k + 20)) for _ in range(5)]
    for i in (1, 3):
        keys.add(S.read_kmers(k, shorts[i])[3])
    reads = [shorts[0], long_read, shorts[1], shorts[2], quiet, shorts[3], early, shorts[4]]
    exp = [int(S.touches(keys, k, s)) for s in reads]
    assert exp == [0, 1, 1, 0, 0, 1, 1, 0]
    return keys, reads


# ---- on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_classes_and_leaks(k):
    keys, reads = case_classes(k)
    g = load(keys, k)
    exp = expect(keys, k, reads)
    hit = check(g, keys, k, reads, exp, "classes")
    assert hit[:3].tolist() == [0, 0, 0]
    # the same reads in another order, so that other reads share a mask word
    order = list(range(len(reads)))
    random.Random(k).shuffle(order)
    check(g, keys, k, [reads[i] for i in order], what="shuffled")
    g.close()


@pytest.mark.parametrize("k", KS)
def test_tiles_one_block_and_default_grid(k):
    keys, reads = case_tiles(k)
    exp = expect(keys, k, reads)
    g = load(keys, k)
    first = check(g, keys, k, reads, exp, "default grid")
    g.configure("grid", 1)
    one = check(g, keys, k, reads, exp, "grid 1")
    assert one.tolist() == first.tolist()
    g.close()


@pytest.mark.parametrize("k", KS)
def test_long_read_branch(k):
    keys, reads = case_long(k)
    g = load(keys, k)
    check(g, keys, k, reads, what="long")
    g.configure("grid", 1)
    check(g, keys, k, reads[::-1], what="long, reversed, grid 1")
    g.close()


@pytest.mark.parametrize("k", KS)
def test_calls_chunks_and_stream(k):
    import torch
    keys, reads = case_classes(k)
    lkeys, lreads = case_long(k)
    keys = keys | lkeys
    reads = reads[:40] + lreads + reads[40:]
    exp = expect(keys, k, reads)
    g = load(keys, k)
    whole = check(g, keys, k, reads, exp, "one call")
    # three calls
    parts, third = [], (len(reads) + 2) // 3
    for i in range(0, len(reads), third):
        parts.append(check(g, keys, k, reads[i:i + third], what="call %d of three" % (i // third)))
    assert np.concatenate(parts).tolist() == whole.tolist()
    # through the device entry
    text = ("\n".join(reads) + "\n").encode()
    soff = np.zeros(len(reads) + 1, dtype=np.int64)
    soff[1:] = np.cumsum([len(s) + 1 for s in reads])
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(soff).cuda()
    d_hit = torch.full((len(reads),), 7, dtype=torch.uint8).cuda()
    g.reads_touch_stream_dev(d_text, len(text), d_off, len(reads), d_hit)
    g.sync()
    assert d_hit.cpu().tolist() == whole.tolist()
    # chunks of 256 and 1024 stream bytes: many chunks in flight, and the long reads go in pieces that overlap by k - 1
    for chunk in (256, 1024):
        g.configure("reads_chunk", chunk)
        assert check(g, keys, k, reads, exp, "chunks of %d" % chunk).tolist() == whole.tolist()
    g.configure("reads_chunk", 0)
    # no reads
    hit, st = g.reads_touch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert hit.tolist() == [] and st.as_dict() == {"num_reads": 0, "num_reads_hit": 0, "num_kmers": 0, "num_kmers_found": 0}
    g.reads_touch_stream_dev(d_text, len(text), d_off, 0, d_hit)
    # a second call does not see the first call's masks: reads of the same lengths that do not hit
    rng = random.Random(k)
    quiet = [junk(rng, keys, k, len(s)) if len(s) < 400 else "T" * len(s) for s in reads]
    assert not any(expect(keys, k, quiet)[0])
    check(g, keys, k, reads, exp, "again")
    assert not check(g, keys, k, quiet, what="quiet").any()
    # the stats are added to the structure that is passed in
    st = mcx.graph.TouchStats()
    g.reads_touch(*arrays(reads), stats=st)
    g.reads_touch(*arrays(reads), stats=st)
    assert st.num_reads == 2 * len(reads) and st.num_kmers == 2 * exp[1][0] and st.num_kmers_found == 2 * exp[1][1]
    g.close()


def test_a_piece_seam_inside_a_k_mer():
    """a read in pieces of 255 bases: its only k-mer in the graph lies across the end of the first piece"""
    k = 31
    rng = random.Random(77)
    read = rseq(rng, 700)
    for at in (255 - k, 255 - k + 1, 240, 254, 255, 2 * 255 - 30 - 5):
        keys = {S.read_kmers(k, read[at:at + k])[0]}
        assert sum(hits(keys, k, read)) == 1
        g = load(keys, k, 1 << 12)
        g.configure("reads_chunk", 256)
        check(g, keys, k, [read[:100], read, read[300:420]], what="seam at %d" % at)
        g.close()


def test_refusals():
    k = 31
    keys, reads = case_classes(k)
    recs = R.pack({key: ((1, 1), [0, 0]) for key in keys}, k, 2)
    g = mcx.Graph(k, 2, 1 << 16)
    g.add_records(recs, 2, [(0, 0), (1, 1)])
    g.configure("intersect", 1)
    before = g.checksum()
    with pytest.raises(mcx.graph.McxError, match="reads does not take a graph in intersect mode") as e:
        g.reads_touch(*arrays(reads))
    assert e.value.code == mcx.graph.MCX_ERR_ARG and g.checksum() == before
    g.close()
    g = mcx.Graph(k, 1, 1 << 16, devices=[0, 0])
    g.add_records(R.pack({key: ((1,), [0]) for key in keys}, k, 1), 1, [(0, 0)])
    before = g.checksum()
    assert before[1] == len(keys)
    with pytest.raises(mcx.graph.McxError, match="reads needs the whole table on one device, not a graph split over devices") as e:
        g.reads_touch(*arrays(reads))
    assert e.value.code == mcx.graph.MCX_ERR_ARG and g.checksum() == before
    g.close()
    g = mcx.Graph(k, 1, 1 << 16, nparts=2, part=0)
    with pytest.raises(mcx.graph.McxError, match="split over devices"):
        g.reads_touch(*arrays(reads))
    g.close()
