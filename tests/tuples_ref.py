"""The exact reference of the tuple insert entries (mcx_graph_insert_tuples_dev, mcx_graph_insert_tuple_segments_dev,
mcx_graph_hashtest) in plain numpy, and the key sets their tests use.  No device, no oracle build:

    for every tuple (key, edge byte e) of colour c:   coverage[key][c] += 1;   edges[key][c] |= e

Keys are rows of W 64-bit words, word 0 most significant, taken exactly as given: nothing here canonicalises."""
import numpy as np

U32 = 0xFFFFFFFF


def words(k):
    return (2 * k + 63) // 64


def top_bits(k):
    """key bits held by word 0"""
    return 2 * k - 64 * (words(k) - 1)


# ---- the reference -----------------------------------------------------------------------------------
def ref_table(keys, edges, cols, ncols, preload=None):
    """-> (distinct keys in key order [m, W] u64, coverage [m, ncols] u64 BEFORE the clamp, edges [m, ncols] u8).
    cols: one colour for all tuples or one per tuple; preload: (keys, coverage [p, ncols], edges [p, ncols]) of
    records already in the table (a key may repeat): coverage is added, edges are OR-ed in."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    keys = keys.reshape(len(keys), -1)
    n, W = keys.shape
    edges = np.ascontiguousarray(edges, dtype=np.uint8).reshape(n)
    cols = np.broadcast_to(np.asarray(cols, dtype=np.int64), (n,))
    assert n == 0 or (0 <= cols.min() and cols.max() < ncols)
    allk = keys
    if preload is not None:
        pk = np.ascontiguousarray(preload[0], dtype=np.uint64).reshape(-1, W)
        allk = np.concatenate([keys, pk])
    if len(allk) == 0:
        return np.zeros((0, W), np.uint64), np.zeros((0, ncols), np.uint64), np.zeros((0, ncols), np.uint8)
    order = np.lexsort(allk.T[::-1])  # (the last key of lexsort is the primary one: word 0)
    sk = allk[order]
    first = np.ones(len(sk), dtype=bool)
    first[1:] = (sk[1:] != sk[:-1]).any(axis=1)
    gid = np.empty(len(sk), dtype=np.int64)
    gid[order] = np.cumsum(first) - 1
    uk = sk[first]
    cov = np.zeros((len(uk), ncols), dtype=np.uint64)
    edg = np.zeros((len(uk), ncols), dtype=np.uint8)
    np.add.at(cov, (gid[:n], cols), np.uint64(1))
    np.bitwise_or.at(edg, (gid[:n], cols), edges)
    if preload is not None:
        np.add.at(cov, gid[n:], np.asarray(preload[1]).astype(np.uint64).reshape(-1, ncols))
        np.bitwise_or.at(edg, gid[n:], np.asarray(preload[2], dtype=np.uint8).reshape(-1, ncols))
    return uk, cov, edg


def pack_body(keys, cov, edg):
    """records -> .ctx body bytes: W key words, ncols u32 coverages (clamped to 2^32 - 1), ncols u8 edges"""
    n = len(keys)
    cov = np.minimum(np.asarray(cov, dtype=np.uint64), U32)
    return np.concatenate([np.ascontiguousarray(keys, "<u8").view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(cov, "<u4").view(np.uint8).reshape(n, -1),
                           np.ascontiguousarray(edg, np.uint8).reshape(n, -1)], axis=1).tobytes()


def parse_body(body, W, ncols):
    rec = np.frombuffer(body, np.uint8).reshape(-1, 8 * W + 5 * ncols)
    keys = rec[:, :8 * W].copy().view("<u8").reshape(-1, W)
    cov = rec[:, 8 * W:8 * W + 4 * ncols].copy().view("<u4").reshape(-1, ncols)
    return keys, cov, rec[:, 8 * W + 4 * ncols:].copy()


def ref_body(keys, edges, cols, ncols, preload=None):
    """the sorted .ctx body of a table that took the tuples (on top of `preload`)"""
    return pack_body(*ref_table(keys, edges, cols, ncols, preload))


def sort_body(body, W, ncols):
    """an unsorted export, sorted on the host by all 64 W key bits"""
    keys, cov, edg = parse_body(body, W, ncols)
    o = np.lexsort(keys.T[::-1])
    return pack_body(keys[o], cov[o], edg[o])


def covg_expect(cov):
    """kmer_covg() of a table with these (unclamped) coverages: per colour (k-mers with coverage, summed coverage)"""
    c = np.minimum(cov, U32)
    return (c > 0).sum(axis=0).tolist(), c.sum(axis=0).tolist()


# ---- keys ------------------------------------------------------------------------------------------
def random_keys(rng, k, n):
    """n uniform keys below 2^(2k)"""
    W = words(k)
    keys = rng.integers(0, 1 << 64, (n, W), dtype=np.uint64)
    keys[:, 0] >>= np.uint64(64 - top_bits(k))
    return keys


def random_edges(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def key_int(row):
    v = 0
    for w in row:
        v = (v << 64) | int(w)
    return v


def key_row(v, W):
    return [(v >> (64 * (W - 1 - w))) & ((1 << 64) - 1) for w in range(W)]


def revcomp(v, k):
    """the reverse complement of the k-mer held in the low 2k bits of the int v"""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (v & 3))
        v >>= 2
    return r


def uniform(rng, k, n):
    """random 2k-bit keys; the second half of the tuples repeats keys of the first half; shuffled"""
    keys = random_keys(rng, k, n)
    h = n // 2
    keys[h:] = keys[rng.integers(0, h, n - h)]
    return keys[rng.permutation(n)]


def repeat_share(keys):
    return 1.0 - len(np.unique(keys, axis=0)) / len(keys)


def corner_keys(rng, k):
    """the keys no read stream produces, as a list of named groups of rows"""
    W = words(k)
    full = (1 << (2 * k)) - 1
    groups = {}

    def rnd():
        return key_int(random_keys(rng, k, 1)[0])

    groups["zero, all ones"] = [0, full]
    a = rnd()
    assert revcomp(a, k) != a
    groups["both strands"] = [a, revcomp(a, k)]
    groups["bit 0"] = [x ^ d for x in (rnd(), rnd(), 0, full) for d in (0, 1)]
    groups["top bit"] = [x ^ d for x in (rnd(), rnd(), 0, full) for d in (0, 1 << (2 * k - 1))]
    if W >= 2:
        lowmask, topshift = (1 << 64) - 1, 64 * (W - 1)
        x = rnd()
        groups["word W-1 only"] = [(x & ~lowmask) | int(v) for v in rng.integers(0, 1 << 64, 8, dtype=np.uint64)] + [x & ~lowmask, x | lowmask]
        y = rnd()
        low = y & ((1 << topshift) - 1)
        tops = [int(v) >> (64 - top_bits(k)) for v in rng.integers(0, 1 << 64, 8, dtype=np.uint64)] + [0, (1 << top_bits(k)) - 1]
        groups["word 0 only"] = [(t << topshift) | low for t in sorted(set(tops))]  # (k = 33, 65: two bits, four values)
    q = rnd() & ~63
    groups["one quotient"] = [q | j for j in range(64)]
    return {name: np.array([key_row(v, W) for v in vals], dtype=np.uint64) for name, vals in groups.items()}


def corners(rng, k, n):
    """every corner key three times among uniform tuples, n tuples in all, shuffled"""
    c = np.concatenate(list(corner_keys(rng, k).values()))
    c = np.concatenate([c, c, c])
    keys = np.concatenate([c, uniform(rng, k, n - len(c))])
    return keys[rng.permutation(n)]


HOT, HOT_OTHERS = 70_000, 30_000


def hot(rng, k):
    """-> (keys, edges, the hot key's row): one key HOT times among HOT_OTHERS other keys, shuffled; each of the
    8 edge bits is alone on one occurrence of the hot key, the rest of the edge bytes are random"""
    hk = random_keys(rng, k, 1)
    others = random_keys(rng, k, HOT_OTHERS)
    assert not (others == hk).all(axis=1).any()
    keys = np.concatenate([np.repeat(hk, HOT, axis=0), others])
    edges = random_edges(rng, len(keys))
    edges[:HOT] &= np.uint8(0x0F)            # (so that the high bits of the hot key come from the planted bytes alone)
    edges[:8] = 1 << np.arange(8)
    p = rng.permutation(len(keys))
    return keys[p], edges[p], hk[0]


def integers(k, first, n):
    """hashtest's keys: the top word is first + i, the other words are 0 (bits above 2k included, as they come)"""
    keys = np.zeros((n, words(k)), dtype=np.uint64)
    keys[:, 0] = np.uint64(first) + np.arange(n, dtype=np.uint64)
    return keys
