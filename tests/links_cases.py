"""Inputs for the `links` tests: .ctp bodies made without a graph, from random tries per (k-mer, orientation).

Every distinct junction prefix of a (k-mer, orientation) owns its gap (the bases between the junction before and its
own) and its filler bases, so links that share a prefix agree on the seq and juncpos of that prefix.

shared_high_words makes the file whose k-mers agree in their high key words (k = 63, 95, 127), for `links`, for
Graph.links_load_text / links_text and for the seeds of `contigs`; stored() says what a graph keeps of a body."""
import random

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


class Trie:
    """the shared part of the links of one (k-mer, orientation)"""

    def __init__(self, rng, first, max_gap=2):
        self.rng, self.first, self.max_gap, self.own = rng, first, max_gap, {}

    def line(self, orient, juncs, count):
        seq, pos, at = [self.first], [], 0
        for i in range(len(juncs)):
            p = juncs[:i]
            if p not in self.own:
                g = self.rng.randint(0, self.max_gap)
                self.own[p] = "".join(self.rng.choice("ACGT") for _ in range(g))
            fill = self.own[p]
            at += len(fill)
            pos.append(at)
            at += 1
            seq.append(fill + juncs[i])
        return "%s %d %d %s seq=%s juncpos=%s" % (orient, len(juncs), count, juncs, "".join(seq), ",".join(map(str, pos)))


def random_strings(rng, n, max_len):
    out = []
    for _ in range(n):
        if out and rng.random() < 0.7:
            base = rng.choice(out)
            base = base[:rng.randint(0, len(base))]
        else:
            base = ""
        ext = "".join(rng.choice("ACGT") for _ in range(rng.randint(0 if base else 1, max(1, max_len - len(base)))))
        s = (base + ext)[:max_len]
        out.append(s if s else rng.choice("ACGT"))
    return out


def generated(k, nkmers, seed, max_len=12, noise=True):
    """-> bytes: nkmers blocks, counts 1..300, identical links repeated, links shuffled inside a block, k-mers in random
    order, comment and empty lines in between, the second k-mer with only R links"""
    rng = random.Random(seed)
    seen, blocks = set(), []
    while len(blocks) < nkmers:
        kmer = "".join(rng.choice("ACGT") for _ in range(k))
        if kmer in seen:
            continue
        seen.add(kmer)
        orients = ["R"] if len(blocks) == 1 else rng.choice((["F"], ["R"], ["F", "R"]))
        blocks.append(block(rng, kmer, orients, max_len, noise))
    head = "# the body begins\n\n" if noise else ""
    return (head + "".join(blocks)).encode()


def block(rng, kmer, orients, max_len=12, noise=True):
    """the block of one k-mer line as written: up to 7 random links per orientation, some twice, some with a prefix"""
    lines = []
    for o in orients:
        t = Trie(rng, kmer if o == "F" else revcomp(kmer))
        strs = random_strings(rng, rng.randint(1, 7), max_len)
        for s in strs:
            lines.append(t.line(o, s, rng.randint(1, 300)))
            if rng.random() < 0.25:  # the same link again
                lines.append(t.line(o, s, rng.randint(1, 300)))
            if len(s) > 1 and rng.random() < 0.3:  # one of its prefixes as a link of its own
                lines.append(t.line(o, s[:rng.randint(1, len(s) - 1)], rng.randint(1, 300)))
    rng.shuffle(lines)
    out = ["%s %d" % (kmer, len(lines))]
    for ln in lines:
        if noise and rng.random() < 0.05:
            out.append(rng.choice(("# a comment", "", "#")))
        out.append(ln)
    if noise and rng.random() < 0.1:
        out.append("")
    return "\n".join(out) + "\n"


SHARED_KS = (63, 95, 127)  # keys of two, three and four words, the top word full


def key_words(kmer):
    """the key words of a k-mer string, the highest first: the last holds the last 32 bases, the first the rest of k"""
    k = len(kmer)
    W = (2 * k + 63) // 64
    x = 0
    for c in kmer:
        x = x << 2 | "ACGT".index(c)
    return [(x >> (64 * (W - 1 - i))) & (2**64 - 1) for i in range(W)]


def shared_high_words(k, seed=None):
    """-> (body bytes, groups) for a k of SHARED_KS: link blocks whose k-mers come in groups that agree in their high key
    words, which random k-mers never do.  groups: [(j, k-mers, turned)], the canonical k-mers of a group agree in the key
    words before word j and differ in word j; where the words below j lie in a group, they sort the other way round than
    word j.  Every k-mer begins with A and does not end with T, so it is its own canonical form.
      j = W - 1   three groups of six k-mers that differ in their last two bases only, and a fourth (`turned`) of which
                  the file holds the reverse complements: the reader has to turn these k-mers and their links round;
      j < W - 1   from three words on, a group of four per word j >= 1 that share the words above it and 3 to 28 bases
                  of it, then hold A C G T, and begin word j + 1 with T G C A.
    The blocks are those of `generated` (links twice, prefixes, comment and empty lines), in shuffled order."""
    rng = random.Random(k if seed is None else seed)
    rs = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    W = (2 * k + 63) // 64
    first = k - 32 * (W - 1)  # the bases of word 0
    groups = []
    for g in range(4):
        stem = "A" + rs(k - 3)
        ends = rng.sample([a + b for a in "ACGT" for b in "ACG"], 6)
        groups.append((W - 1, [stem + e for e in ends], g == 3))
    for j in range(1, W - 1):
        at = first + 32 * (j - 1) + rng.randint(3, 28)  # inside word j
        stem, nxt = "A" + rs(at - 1), first + 32 * j
        kmers = []
        for i in range(4):
            s = stem + "ACGT"[i] + rs(k - at - 1)
            kmers.append(s[:nxt] + "TGCA"[i] + s[nxt + 1:k - 1] + rng.choice("ACG"))
        groups.append((j, kmers, False))
    written = [(revcomp(s) if turned else s) for _, kmers, turned in groups for s in kmers]
    assert len(set(written)) == len(written)
    rng.shuffle(written)
    body = "".join(block(rng, s, ["R"] if i == 1 else rng.choice((["F"], ["R"], ["F", "R"]))) for i, s in enumerate(written))
    return ("# the body begins\n\n" + body).encode(), groups


def stored(body, k):
    """what a graph keeps of a .ctp body (Graph.links_load_text): [(key, orient, junction bases, nseen)] with every k-mer
    turned to its canonical form (its links change orientation with it), equal links added up, 255 at the most"""
    import clean_restate as R
    per, key, turn = {}, None, 0
    for ln in body.decode().split("\n"):
        if ln[:1] in ("A", "C", "G", "T"):
            x = R.kmer_int(ln.split(" ")[0])
            key = R.canon(x, k)
            turn = 0 if key == x else 1
        elif ln[:2] in ("F ", "R "):
            cols = ln.split(" ")
            link = (key, (0 if cols[0] == "F" else 1) ^ turn, tuple("ACGT".index(c) for c in cols[3]))
            per[link] = min(255, per.get(link, 0) + min(255, int(cols[2])))
    return [(key, o, b, n) for (key, o, b), n in per.items()]


def blocks_of(text):
    """the k-mer blocks of a body (what precedes the first k-mer line goes with the first block)"""
    out, cur = [], []
    for ln in text.decode().split("\n")[:-1]:
        if ln[:1] in ("A", "C", "G", "T") and any(x[:1] in ("A", "C", "G", "T") for x in cur):
            out.append("\n".join(cur) + "\n")
            cur = []
        cur.append(ln)
    if cur:
        out.append("\n".join(cur) + "\n")
    return [b.encode() for b in out]


def seams(k=31):
    """links of 1, 31, 32, 33, 64, 65 and 1000 junctions that differ only in their last junction, and pairs of which
    one is the other's prefix across a 32-junction boundary"""
    rng = random.Random(5)
    blocks = []
    for n in (1, 31, 32, 33, 64, 65, 1000):
        kmer = "".join(rng.choice("ACGT") for _ in range(k))
        t = Trie(rng, kmer, max_gap=1)
        stem = "".join(rng.choice("ACGT") for _ in range(n - 1))
        lines = [t.line("F", stem + b, 3 + i) for i, b in enumerate("TGCA")]
        blocks.append("%s %d\n%s\n" % (kmer, len(lines), "\n".join(lines)))
    for a, b in ((31, 33), (32, 33), (32, 64), (33, 65), (64, 65), (1, 64)):
        kmer = "".join(rng.choice("ACGT") for _ in range(k))
        t = Trie(rng, revcomp(kmer), max_gap=1)
        s = "".join(rng.choice("ACGT") for _ in range(b))
        lines = [t.line("R", s, 7), t.line("R", s[:a], 11), t.line("R", s[:a - 1] + COMP[s[a - 1]], 2)]
        blocks.append("%s %d\n%s\n" % (kmer, len(lines), "\n".join(lines)))
    return "".join(blocks).encode()


def comb(n, k=5):
    """one k-mer, n links, link i has i junctions and is the prefix of the next; the count of link i is 1 + i % 3"""
    rng = random.Random(11)
    kmer = "ACGTA"[:k]
    s = "".join(rng.choice("ACGT") for _ in range(n))
    pos = list(map(str, range(n)))
    lines = ["F %d %d %s seq=%s%s juncpos=%s" % (i, 1 + i % 3, s[:i], kmer, s[:i], ",".join(pos[:i])) for i in range(1, n + 1)]
    return ("%s %d\n%s\n" % (kmer, n, "\n".join(lines))).encode()


def bush(depth=6, k=5):
    """one k-mer, all 4^depth links of `depth` junctions, the count of link i is 1 + i % 5"""
    kmer = "CCGTA"[:k]
    lines = []
    for i in range(4 ** depth):
        s = "".join("ACGT"[(i >> (2 * (depth - 1 - j))) & 3] for j in range(depth))
        lines.append("R %d %d %s seq=%s%s juncpos=%s" % (depth, 1 + i % 5, s, kmer, s, ",".join(map(str, range(depth)))))
    random.Random(3).shuffle(lines)
    return ("%s %d\n%s\n" % (kmer, len(lines), "\n".join(lines))).encode()


def header(k, ncols=1, version=4, totals=(0, 0, 0), commands=None):
    """the JSON header of a .ctp file, as text"""
    import json
    hdr = {"file_format": "ctp", "format_version": version, "file_key": "0123456789abcdef",
           "graph": {"num_colours": ncols, "kmer_size": k, "num_kmers_in_graph": 1000,
                     "colours": [{"colour": c, "sample": "s%d {\"}" % c, "total_sequence": 5, "cleaned_tips": False, "cleaned_unitigs": False}
                                 for c in range(ncols)]},
           "commands": commands if commands is not None else [{"key": "aabbccdd", "cmd": ["mccortex31", "thread"], "prev": []}],
           "paths": {"num_kmers_with_paths": totals[0], "num_paths": totals[1], "path_bytes": totals[2],
                     "contig_hists": [{"lengths": [31], "counts": [4]}]}}
    return json.dumps(hdr, indent=2)


def ctp_file(path, k, body, **kw):
    import gzip
    with gzip.open(path, "wb") as f:
        f.write(header(k, **kw).encode() + b"\n\n# a comment block\n\n" + body)


def split_ctp(raw):
    """(header as a dict, body bytes with comment and empty lines as they are) of an uncompressed .ctp"""
    import json
    hdr, end = json.JSONDecoder().raw_decode(raw.decode())
    return hdr, raw[len(raw.decode()[:end].encode()):]
