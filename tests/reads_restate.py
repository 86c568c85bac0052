"""Pure-Python restatement of `mccortex<K> reads` (src/commands/ctx_reads.c), with no device involved.

touches: a read touches the graph iff one of its k-mers is a key.  The k-mers of a read are those of every maximal run
of ACGTacgt that is at least k long; lower case counts as upper case, any other byte ends a run; the lookup is by
canonical key.  There is no quality or homopolymer cutoff.

Pairing: --seq2 pairs read i of one file with read i of the other and stops at the shorter file; --seqi pairs two
consecutive reads iff their names match (names_match: equal up to the first whitespace, or equal there except for a
final 1 against 2 directly after a '/'; two empty names do not match), otherwise the first is a single read and the
second is tried against the next.  If either mate touches the graph both are printed; --invert prints exactly what
the default does not.

Output (src/basic/seqout.h): FASTA ">name\\nseq\\n", FASTQ "@name\\nseq\\n+\\nqual\\n" with the qualities cut or
padded with '.' to the sequence's length, plain "seq\\n"; singles go to <O>.*, pairs to <O>.1.* and <O>.2.*, in input
order."""

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
WHITE = " \t\n\r\v\f"


def kmer_int(s):
    v = 0
    for ch in s:
        v = (v << 2) | CODE[ch]
    return v


def revcomp_int(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canon(x, k):
    return min(x, revcomp_int(x, k))


def read_kmers(k, seq):
    """canonical k-mers of a read, one per occurrence, in order (forward and reverse strand rolled along)"""
    out, run, fw, rc = [], 0, 0, 0
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    for ch in seq.upper():
        c = CODE.get(ch)
        if c is None:
            run = 0
            continue
        run += 1
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        if run >= k:
            out.append(min(fw, rc))
    return out


def keys_of(seqs, k):
    """the key set of the graph `build -k k` makes of the sequences"""
    return {x for s in seqs for x in read_kmers(k, s)}


def touches(keys, k, seq):
    return any(x in keys for x in read_kmers(k, seq))


def counts(keys, k, seqs):
    """(k-mer occurrences in the reads, occurrences whose k-mer is a key)"""
    n = f = 0
    for s in seqs:
        for x in read_kmers(k, s):
            n += 1
            f += x in keys
    return n, f


def names_match(a, b):
    def head(s):
        for i, ch in enumerate(s):
            if ch in WHITE:
                return s[:i]
        return s
    a, b = head(a), head(b)
    if len(a) != len(b) or not a:
        return False
    if a == b:
        return True
    return len(a) >= 2 and a[:-1] == b[:-1] and a[-2] == "/" and {a[-1], b[-1]} == {"1", "2"}


# a read is (name, seq, qual); qual may be ""
def pair_seq2(reads1, reads2):
    """units of a --seq2 task: (r1, r2) per pair; a mate 2 without sequence leaves mate 1 a single read"""
    return [(a, b) if b[1] else (a,) for a, b in zip(reads1, reads2)]


def pair_seqi(reads):
    units, i = [], 0
    while i < len(reads):
        if i + 1 < len(reads) and names_match(reads[i][0], reads[i + 1][0]):
            units.append((reads[i], reads[i + 1]) if reads[i + 1][1] else (reads[i],))
            i += 2
        else:
            units.append((reads[i],))
            i += 1
    return units


def fmt_read(read, fmt):
    name, seq, qual = read
    if fmt == "fa":
        return ">%s\n%s\n" % (name, seq)
    if fmt == "fq":
        return "@%s\n%s\n+\n%s\n" % (name, seq, (qual + "." * len(seq))[:len(seq)])
    return seq + "\n"


def filter_units(keys, k, units, fmt="fq", invert=False):
    """({"": text of <O>.*, "1": of <O>.1.*, "2": of <O>.2.*}, reads printed, reads seen)"""
    out = {"": [], "1": [], "2": []}
    printed = total = 0
    for u in units:
        total += len(u)
        if any(touches(keys, k, r[1]) for r in u) != invert:
            printed += len(u)
            if len(u) == 1:
                out[""].append(fmt_read(u[0], fmt))
            else:
                out["1"].append(fmt_read(u[0], fmt))
                out["2"].append(fmt_read(u[1], fmt))
    return {w: "".join(t) for w, t in out.items()}, printed, total
