"""A CPU restatement of `clean` (src/commands/ctx_clean.c, src/tools/clean_graph.c, src/graph/db_unitig.c,
src/graph/prune_nodes.c), written from the reference's semantics as the expectation of the device tests.

A graph is {key int: (covgs tuple, edges list)} with one entry per colour.  Edge bit nuc + 4 * orient:
orient 0 appends nuc to the key (the k-mer read forwards), orient 1 appends nuc to its reverse complement.

Assumption: carrays' gca_median_uint32 is not available to read.  The median of an even-length list is
taken as the mean of the two middle values rounded down; `median` below is the one place that says so.
"""
import struct

NBINS = 1000
U32 = 2**32 - 1


def revcomp(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canon(x, k):
    return min(x, revcomp(x, k))


def kmer_int(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def median(vals):
    s = sorted(vals)
    n = len(s)
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) // 2  # even length: assumed, see the module text


def outdeg(e, o):
    return bin((e >> (4 * o)) & 15).count("1")


def step(key, o, x, k):
    """the node reached from (key, o) over nucleotide x: (key', orient')"""
    s = key if o == 0 else revcomp(key, k)
    s2 = ((s << 2) | x) & ((1 << (2 * k)) - 1)
    c = canon(s2, k)
    return c, (0 if c == s2 else 1)


def union_edges(graph, key):
    e = 0
    for x in graph[key][1]:
        e |= x
    return e


def sum_covg(graph, key):
    return min(sum(min(c, U32) for c in graph[key][0]), U32)


def _extend(graph, buf, k):
    """db_unitig_extend: walk on from buf[-1] while the current node has one edge out and the next one edge in;
    stop before the first node's key (a closed cycle) or the last node's key (a hairpin or self-loop)"""
    first = buf[0][0]
    key, o = buf[-1]
    while True:
        e = union_edges(graph, key)
        if outdeg(e, o) != 1:
            return
        x = ((e >> (4 * o)) & 15).bit_length() - 1
        nk, no = step(key, o, x, k)
        if nk not in graph:  # the reference asserts; an absent neighbour ends the walk here
            return
        if outdeg(union_edges(graph, nk), 1 - no) != 1:
            return
        if nk == first or nk == buf[-1][0]:
            return
        buf.append((nk, no))
        key, o = nk, no


def unitig(graph, key, k):
    """db_unitig_fetch: [(key, orient)] of the unitig through `key`"""
    buf = [(key, 1)]
    _extend(graph, buf, k)
    buf = [(kk, 1 - o) for kk, o in reversed(buf)]
    _extend(graph, buf, k)
    return buf


def unitigs(graph, k):
    seen = set()
    out = []
    for key in sorted(graph):
        if key in seen:
            continue
        u = unitig(graph, key, k)
        for kk, _ in u:
            assert kk not in seen, "k-mer in two unitigs"
            seen.add(kk)
        out.append(u)
    return out


def hists(graph, us):
    kc, uc, ul = [0] * NBINS, [0] * NBINS, [0] * NBINS
    for u in us:
        cv = [sum_covg(graph, kk) for kk, _ in u]
        for c in cv:
            kc[min(c, NBINS - 1)] += 1
        uc[min(median(cv), NBINS - 1)] += 1
        ul[min(len(u), NBINS - 1)] += 1
    return {"kmer_covg": kc, "unitig_covg": uc, "unitig_len": ul}


def is_tip(graph, u):
    (k0, o0), (k1, o1) = u[0], u[-1]
    return outdeg(union_edges(graph, k0), 1 - o0) + outdeg(union_edges(graph, k1), o1) <= 1


def clean(graph, k, threshold, min_keep_tip):
    """clean_graph + prune_nodes_lacking_flag: (cleaned graph, stats, before hists, after hists)"""
    us = unitigs(graph, k)
    before = hists(graph, us)
    st = dict(num_tips=0, num_tip_kmers=0, num_low_covg_unitigs=0, num_low_covg_unitig_kmers=0,
              num_tip_and_low_unitigs=0, num_tip_and_low_unitig_kmers=0)
    kept_us = []
    for u in us:
        med = median([sum_covg(graph, kk) for kk, _ in u])
        low = med < threshold
        tip = len(u) < min_keep_tip and is_tip(graph, u)
        name = "tip_and_low_unitig" if low and tip else "low_covg_unitig" if low else "tip" if tip else None
        if name:
            st["num_%ss" % name] += 1
            st["num_%s_kmers" % name] += len(u)
        else:
            kept_us.append(u)
    kept = {kk for u in kept_us for kk, _ in u}
    out = {}
    for key in kept:
        e = union_edges(graph, key)
        mask = e
        for b in range(8):
            if (e >> b) & 1:
                nk, _ = step(key, b >> 2, b & 3, k)
                if nk not in kept:  # not kept, or not in the graph at all
                    mask &= ~(1 << b)
        cv, ed = graph[key]
        out[key] = (cv, [x & mask for x in ed])
    return out, st, before, hists(graph, kept_us)


# ---- .ctx body records -------------------------------------------------------------------------
def parse(body, k, ncols):
    W = (2 * k + 63) // 64
    rs = 8 * W + 5 * ncols
    g = {}
    for i in range(0, len(body), rs):
        words = struct.unpack_from("<%dQ" % W, body, i)
        key = 0
        for w in words:
            key = (key << 64) | w
        cv = struct.unpack_from("<%dI" % ncols, body, i + 8 * W)
        g[key] = (tuple(cv), list(body[i + 8 * W + 4 * ncols:i + rs]))
    return g


def pack(graph, k, ncols):
    """sorted records (the order of `--sort`)"""
    W = (2 * k + 63) // 64
    parts = []
    for key in sorted(graph):
        cv, ed = graph[key]
        words = [(key >> (64 * (W - 1 - i))) & (2**64 - 1) for i in range(W)]
        parts.append(struct.pack("<%dQ%dI" % (W, ncols), *words, *cv) + bytes(ed))
    return b"".join(parts)


def build(seqs_by_colour, k):
    """the graph `build` makes of the given sequences (one list per colour): coverage per occurrence and the
    edges between consecutive k-mers of a sequence, each in its own orientation"""
    ncols = len(seqs_by_colour)
    g = {}
    for c, seqs in enumerate(seqs_by_colour):
        for s in seqs:
            prev = None
            for i in range(len(s) - k + 1):
                w = s[i:i + k]
                if any(ch not in "ACGT" for ch in w):
                    prev = None
                    continue
                x = kmer_int(w)
                key = canon(x, k)
                o = 0 if key == x else 1
                cv, ed = g.setdefault(key, ([0] * ncols, [0] * ncols))
                cv[c] = min(cv[c] + 1, U32)
                if prev is not None:
                    pk, po = prev
                    g[pk][1][c] |= 1 << ("ACGT".index(w[-1]) + 4 * po)  # prev -> this, in prev's orientation
                    ed[c] |= 1 << (3 - "ACGT".index(s[i - 1]) + 4 * (1 - o))  # this -> prev, reversed
                prev = (key, o)
    return {key: (tuple(cv), ed) for key, (cv, ed) in g.items()}


# ---- the threshold (cleaning_pick_kmer_threshold, clean_graph.c): double precision through libm -------------
def _libm():
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in ("tgamma", "lgamma", "pow", "exp", "log"):
        getattr(m, f).restype = ctypes.c_double
        getattr(m, f).argtypes = [ctypes.c_double] * (2 if f == "pow" else 1)
    return m


def _div(a, b):
    """C double division: inf or nan where Python raises"""
    if b == 0:
        return float("nan") if a == 0 or a != a else (float("inf") if a > 0 else float("-inf"))
    return a / b


def pick_threshold(kmer_covg):
    m = _libm()
    n = len(kmer_covg)
    r1 = _div(float(kmer_covg[2]), float(kmer_covg[1]))
    r2 = _div(float(kmer_covg[3]), float(kmer_covg[2]))
    rr = _div(r2, r1)
    best, best_i = float("inf"), 0
    for i in range(1, 201):
        aa = i * 0.01
        faa = m.tgamma(aa) * m.tgamma(aa + 2) / (2 * m.pow(m.tgamma(aa + 1), 2))
        t = abs(faa - rr)
        if t < best:
            best, best_i = t, i
    a = best_i * 0.01
    b = _div(m.tgamma(a + 1.0), r1 * m.tgamma(a)) - 1.0
    b = b if b >= 1 else 1  # MAX2(b, 1): a nan becomes 1
    c0 = kmer_covg[1] * m.pow(b / (1 + b), -a)
    e = [0.0] * n
    e_total, d_total = 0.0, 0
    lb, l1b, lga = m.log(b), m.log(1 + b), m.lgamma(a)
    for i in range(1, n):
        e[i] = m.exp(a * lb - lga - m.lgamma(i) + m.lgamma(a + i - 1) - (a + i - 1) * l1b) * c0
        e_total += e[i]
        d_total += kmer_covg[i]
    cut = next((i for i in range(1, n) if _div(e[i], float(kmer_covg[i])) <= 0.001), -1)
    if cut < 0:  # false positives < false negatives
        er, dr, es, ds = e_total, float(d_total), 0.0, 0.0
        for i in range(1, n):
            es += e[i]; ds += kmer_covg[i]; er -= e[i]; dr -= kmer_covg[i]
            if 1 - _div(es, ds) > _div(er, dr):
                cut = i
                break
    if cut < 0:  # sequence lost > errors left
        er, es, ds = e_total, 0.0, 0.0
        for i in range(1, n):
            es += e[i]; ds += kmer_covg[i]; er -= e[i]
            if ds - es > er:
                cut = i
                break
    if cut < 0:
        return -1
    below = sum(kmer_covg[i] * i for i in range(cut)) % 2**64
    above = sum(kmer_covg[i] * i for i in range(cut, n)) % 2**64
    return cut if _div(float(above), float((below + above) % 2**64)) >= 0.2 else -1


# ---- CSV files (cleaning_write_covg_histogram / cleaning_write_len_histogram) ---------------------------------
def covg_csv(kc, uc):
    end = len(kc) - 1
    while end > 2 and kc[end] == 0:
        end -= 1
    return "Covg,NumKmers,NumUnitigs\n" + "".join("%d,%d,%d\n" % (i, kc[i], uc[i]) for i in range(1, end + 1) if kc[i] > 0)


def len_csv(ul, k):
    end = len(ul) - 1
    while end > 1 and ul[end] == 0:
        end -= 1
    return "UnitigKmerLength,bp,Count\n1,%d,%d\n" % (k, ul[1]) + "".join(
        "%d,%d,%d\n" % (i, k + i - 1, ul[i]) for i in range(2, end + 1) if ul[i] > 0)
