"""`pjoin` restated (src/commands/ctx_pjoin.c, src/graph_paths/gpath_reader.c, src/paths/gpath_subset.c, gpath.c:gpath_cmp,
src/graph_paths/gpath_save.c, src/graph/json_hdr.c:json_hdr_make_std), in plain Python with no device involved.

The store is a dict: k-mer text -> {(orient, juncs): [count per output colour]}.  Nothing here sorts all links at once or
reduces runs, as the device engine does: the two check each other.

1. Link lines (link_line_parse, version 4): `<F|R> <njuncs> <c0,c1,..> <juncs> [tags]`; the count column holds exactly the
   file's colours; tags are not read.  Through the filter [(from, into)]: into[into] += count[from]; a line whose into
   counts are all zero is dropped.  The k-mer of a `<kmer> <n>` line is taken as written.
2. Two links are the same link iff k-mer, orientation and junction string are equal; a prefix and its extension are
   different links.  Per colour the count of a merged link is min(255, sum over its lines); every step saturates, so the
   order of addition does not matter.
3. Body: K-MERS IN ASCENDING ORDER OF THEIR TEXT (the device's key order), `<kmer> <nlinks>`, then the links in gpath_cmp
   order: F before R, junction strings in text order with A<C<G<T, a prefix before its extensions; each
   `<F|R> <njuncs> <c0,..,cN-1> <juncs>`.  A k-mer with no kept link is not written.
4. Header (merged_header): see there.
5. Refusals, under the names of graph.LINKS_REFUSALS, with the byte offset of the line; the first bad line of a piece
   wins and nothing of that piece is stored."""
import collections
import copy

MAX_JUNCS, MAX_SEEN = 32767, 255
ACGT = "ACGT"


class BadLine(Exception):
    def __init__(self, code, offset):
        super().__init__("%s at byte %d" % (code, offset))
        self.code, self.offset = code, offset


class SampleClash(Exception):
    """Graph/path sample names do not match"""


def _number(s):
    return s.isascii() and s.isdigit()


def parse_link(line, src_ncols):
    """-> (orient, juncs, counts) or the refusal's name"""
    if len(line) < 2 or line[0] not in "FR" or line[1] != " ":
        return "bad_orient"
    cols = line[2:].split(" ")
    if not _number(cols[0]) or len(cols) < 2:
        return "bad_number"
    nj = int(cols[0])
    counts = cols[1].split(",")
    if not all(_number(c) for c in counts) or len(cols) < 3:
        return "bad_number"
    if len(counts) != src_ncols:
        return "count_columns"
    juncs = cols[2]
    if any(c not in ACGT for c in juncs):
        return "bad_junction"
    if nj == 0 or nj > MAX_JUNCS:
        return "njuncs_range"
    if nj != len(juncs):
        return "njuncs_length"
    return line[0], juncs, [int(c) for c in counts]


class Pjoin:
    def __init__(self, k, out_ncols):
        self.k, self.ncols = k, out_ncols
        self.store = {}
        self.totals = dict.fromkeys(("kmer_lines", "link_lines", "links_kept", "kmers_n_mismatch"), 0)

    def add(self, text, src_ncols=1, filter=None):
        """the lines of a piece; -> the piece's counts.  BadLine: nothing of the piece is stored."""
        flt = [(c, c) for c in range(src_ncols)] if filter is None else list(filter)
        for f, t in flt:
            if not (0 <= f < src_ncols and 0 <= t < self.ncols):
                raise ValueError("filter entry out of range")
        ps = dict.fromkeys(self.totals, 0)
        kept, kmer, off, block = [], None, 0, None  # block: [n of the k-mer line, link lines seen]
        blocks = []
        for line in text.decode().split("\n")[:-1]:
            here, off = off, off + len(line.encode()) + 1
            if not line or line[0] == "#":
                continue
            if line[0] in ACGT:
                k = self.k
                if not (len(line) >= k + 2 and line[k] == " " and all(c in ACGT for c in line[:k]) and _number(line[k + 1:])):
                    raise BadLine("bad_kmer_line", here)
                kmer, block = line[:k], [int(line[k + 1:]), 0]
                blocks.append(block)
                ps["kmer_lines"] += 1
                continue
            if kmer is None:
                raise BadLine("link_before_kmer", here)
            got = parse_link(line, src_ncols)
            if isinstance(got, str):
                raise BadLine(got, here)
            o, juncs, counts = got
            ps["link_lines"] += 1
            block[1] += 1
            into = [0] * self.ncols
            for f, t in flt:
                into[t] += counts[f]
            if any(into):
                kept.append((kmer, o, juncs, into))
        ps["links_kept"] = len(kept)
        ps["kmers_n_mismatch"] = sum(n != seen for n, seen in blocks)
        for kmer, o, juncs, into in kept:
            cur = self.store.setdefault(kmer, {}).setdefault((o, juncs), [0] * self.ncols)
            for c in range(self.ncols):
                cur[c] = min(MAX_SEEN, cur[c] + into[c])
        for n in ps:
            self.totals[n] += ps[n]
        return ps

    def by_kmer(self):
        """[(kmer, [((orient, juncs), counts)] in gpath_cmp order)] in k-mer order"""
        return [(kmer, sorted(self.store[kmer].items())) for kmer in sorted(self.store)]

    def text(self):
        out = []
        for kmer, links in self.by_kmer():
            out.append("%s %d\n" % (kmer, len(links)))
            for (o, juncs), counts in links:
                out.append("%s %d %s %s\n" % (o, len(juncs), ",".join(map(str, counts)), juncs))
        return "".join(out).encode()

    def info(self):
        links = [j for d in self.store.values() for _, j in d]
        return {"num_kmers_with_paths": len(self.store), "num_paths": len(links), "path_bytes": sum((len(j) + 3) // 4 for j in links)}


def default_filters(ncols_of_files):
    """the filters of inputs given without offsets: each file loads into the colours from the running maximum on"""
    out, at = [], 0
    for n in ncols_of_files:
        out.append([(c, at + c) for c in range(n)])
        at += n
    return out


def merged_header(k, out_ncols, inputs, info, command=None):
    """The header `pjoin` writes, as a dict.  inputs: [(header dict of the file, filter [(from, into)])] in input order.
       file_format "ctp", format_version 4, file_key (fresh: None here)
       graph: num_colours, kmer_size, num_kmers_in_graph = the k-mers written; per colour the sample of the inputs
           ("undefined" where no file fills it; two names for one colour: SampleClash), total_sequence 0, cleaned_* false
       commands: this command first (None here, or `command` with its "prev" filled), its prev = the first command key of
           every input in input order; then the inputs' commands in input order, each key once
       paths: the totals, contig_hists: per output colour the input histograms of the colours that load into it added
           length by length, zero counts and length 0 left out"""
    names = ["undefined"] * out_ncols
    hists = [collections.Counter() for _ in range(out_ncols)]
    prev, cmds, seen = [], [], set()
    for hdr, flt in inputs:
        for f, t in flt:
            name = hdr["graph"]["colours"][f]["sample"]
            if names[t] == "undefined":  # gpath_reader_load_sample_names
                names[t] = name
            elif names[t] != name:
                raise SampleClash("Graph/path sample names do not match [%d->%d] '%s' vs '%s'" % (f, t, names[t], name))
            h = hdr["paths"]["contig_hists"]
            if f >= len(h):
                raise ValueError("No hist for colour %d" % f)  # gpath_reader_load_contig_hist dies
            for ln, n in zip(h[f]["lengths"], h[f]["counts"]):
                hists[t][ln] += n
        c = hdr.get("commands") or []
        if c and isinstance(c[0].get("key"), str):
            prev.append(c[0]["key"])
        for x in c:
            if isinstance(x.get("key"), str) and x["key"] not in seen:
                seen.add(x["key"])
                cmds.append(copy.deepcopy(x))
    first = dict(command) if command is not None else {"key": None, "cmd": None}
    first["prev"] = prev
    return {"file_format": "ctp", "format_version": 4, "file_key": None,
            "graph": {"num_colours": out_ncols, "kmer_size": k, "num_kmers_in_graph": info["num_kmers_with_paths"],
                      "colours": [{"colour": c, "sample": names[c], "total_sequence": 0,
                                   "cleaned_tips": False, "cleaned_unitigs": False} for c in range(out_ncols)]},
            "commands": [first] + cmds,
            "paths": dict(info, contig_hists=[{"lengths": [ln for ln in sorted(h) if ln and h[ln]], "counts": [h[ln] for ln in sorted(h) if ln and h[ln]]}
                                              for h in hists])}
