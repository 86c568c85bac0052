"""`links` restated: src/paths/link_tree.c and the loop of src/commands/ctx_links.c, transcribed literally.

A tree of nodes with children[4], counts[4], dist and seq per orientation, built by ltree_add and walked by the two
visitors.  Nothing here uses the sorted-list formulation of the device engine (longest common prefixes, range sums):
the two check each other.  The line parser refuses what link_line_parse and gpath_reader_read_kmer refuse, under the
names of graph.LINKS_REFUSALS."""

NUC = {"A": 0, "C": 1, "G": 2, "T": 3}
MAX_JUNCS = 32767


class BadLine(Exception):
    def __init__(self, code, offset):
        super().__init__("%s at byte %d" % (code, offset))
        self.code, self.offset = code, offset


class Node:
    __slots__ = ("id", "parent", "children", "counts", "dist", "seq", "base")

    def __init__(self, id_, parent, dist, seq, base):
        self.id, self.parent, self.children, self.counts = id_, parent, [None] * 4, [0] * 4
        self.dist, self.seq, self.base = dist, seq, base


class LinkTree:
    def __init__(self, k):
        self.k = k
        self.reset()

    def reset(self):
        self.nodes, self.fw, self.rv, self.ntree = [], None, None, 0

    def _init_node(self, parent, dist, seq, base):
        n = Node(len(self.nodes), parent, dist, seq, base)
        self.nodes.append(n)
        return n

    def add(self, fw, covg, dists, juncs, seq):
        """ltree_add"""
        k = self.k
        assert len(seq) == k + dists[len(juncs) - 1] + 1
        root = self.fw if fw else self.rv
        parent, node, prev_nuc = None, None, 0
        for i in range(len(juncs)):
            nuc = NUC[seq[k + dists[i]]]
            node = parent.children[prev_nuc] if i > 0 else root
            if node is None:
                seq_offset = k + dists[i - 1] + 1 if i > 0 else 0
                dist = dists[i] - dists[i - 1] - 1 if i > 0 else k + dists[0]
                node = self._init_node(parent, dists[i], seq[seq_offset:seq_offset + dist], prev_nuc if i > 0 else -1)
                if i > 0:
                    parent.children[prev_nuc] = node
                elif fw:
                    self.fw = node
                else:
                    self.rv = node
            self.ntree += node.counts[nuc] == 0  # (a count of the suite, not of the reference: distinct prefixes seen)
            node.counts[nuc] += covg
            parent, prev_nuc = node, nuc

    def _visit_links_sub(self, root, func):
        """ltree_visit_links_sub: func(node, base, depth) -> keep going"""
        if root is None:
            return
        wbuf = [[root, 0]]
        while wbuf:
            walk = wbuf[-1]
            while walk[1] < 4 and walk[0].counts[walk[1]] == 0:
                walk[1] += 1
            base = walk[1]
            walk[1] += 1
            if base == 4:
                wbuf.pop()
            elif func(walk[0], base, len(wbuf) - 1) and walk[0].children[base] is not None:
                wbuf.append([walk[0].children[base], 0])

    def visit_links(self, func):
        self._visit_links_sub(self.fw, func)
        self._visit_links_sub(self.rv, func)

    def get_stats(self, stats):
        """ltree_get_stats"""
        init = stats["num_links"]

        def f(l, base, depth):
            if l.children[base] is None:
                stats["num_links"] += 1
                stats["num_link_bytes"] += (depth + 1 + 3) // 4
            return True
        self.visit_links(f)
        stats["num_trees_with_links"] += stats["num_links"] > init

    def clean(self, cutoff):
        """ltree_clean"""
        def f(l, base, depth):
            if l.counts[base] < cutoff:
                l.counts[base] = 0
                l.children[base] = None
                return False
            return True
        self.visit_links(f)

    def write_list(self, out):
        def f(l, base, depth):
            out.append("%d,%d\n" % (self.k + l.dist + 1, l.counts[base]))
            return True
        self.visit_links(f)

    def write_ctp(self, kmer, num_links, out):
        out.append("%s %d\n" % (kmer, num_links))

        def f(l, base, depth):
            if l.children[base] is not None:
                return True
            njuncs = depth + 1
            nodes, lj = [None] * njuncs, l
            i = njuncs - 1
            while lj is not None:
                nodes[i] = lj
                lj = lj.parent
                i -= 1
            juncs = ["ACGT"[nodes[i + 1].base] for i in range(njuncs - 1)] + ["ACGT"[base]]
            fw = nodes[0] is self.fw
            seq = "".join(nodes[i].seq + juncs[i] for i in range(njuncs))
            out.append("%s %d %d %s seq=%s juncpos=%s\n" % ("F" if fw else "R", njuncs, l.counts[base], "".join(juncs), seq,
                                                          ",".join(str(n.dist) for n in nodes)))
            return True
        self.visit_links(f)

    def update_covg_hists(self, hists, distsize, covgsize):
        def f(l, base, depth):
            if l.dist >= distsize:
                return False
            hists[l.dist][min(l.counts[base], covgsize - 1)] += 1
            return True
        self.visit_links(f)


def _is_num(s):
    return len(s) > 0 and all("0" <= c <= "9" for c in s)


def parse_link_line(line, k, off=0):
    """link_line_parse (version 4), the refusals in the order the engine documents -> (fw, count, juncs, seq, juncpos)"""
    if len(line) < 2 or line[0] not in "FR" or line[1] != " ":
        raise BadLine("bad_orient", off)
    cols = line.split(" ")
    if len(cols) < 2 or not _is_num(cols[1]) or len(cols) < 3:
        raise BadLine("bad_number", off)
    if not _is_num(cols[2]):
        head = cols[2].split(",")[0]
        if "," in cols[2] and _is_num(head):
            raise BadLine("multi_colour", off)
        raise BadLine("bad_number", off)
    if len(cols) < 4:
        raise BadLine("bad_number", off)
    juncs = cols[3]
    if any(c not in "ACGT" for c in juncs):
        raise BadLine("bad_junction", off)
    njuncs = int(cols[1])
    if njuncs == 0 or njuncs > MAX_JUNCS:
        raise BadLine("njuncs_range", off)
    if njuncs != len(juncs):
        raise BadLine("njuncs_length", off)
    seq = next((c[4:] for c in cols[4:] if c.startswith("seq=")), None)
    jp = next((c[8:] for c in cols[4:] if c.startswith("juncpos=")), None)
    if seq is None:
        raise BadLine("no_seq", off)
    if jp is None:
        raise BadLine("no_juncpos", off)
    items = jp.split(",")
    if not all(_is_num(x) for x in items) or len(items) != njuncs:
        raise BadLine("juncpos_count", off)
    pos = [int(x) for x in items]
    if len(seq) != k + pos[-1] + 1:
        raise BadLine("seq_length", off)
    if any(k + p >= len(seq) or seq[k + p] != juncs[i] for i, p in enumerate(pos)):
        raise BadLine("seq_base", off)
    return line[0] == "F", int(cols[2]), juncs, seq, pos


def parse_kmer_line(line, k, off=0):
    if len(line) < k + 2 or any(c not in "ACGT" for c in line[:k]) or line[k] != " " or not _is_num(line[k + 1:]):
        raise BadLine("bad_kmer_line", off)
    return line[:k]


def new_stats():
    return {"num_trees_with_links": 0, "num_links": 0, "num_link_bytes": 0, "tree_links": 0, "kmers_read": 0, "links_in": 0}


def links(text, k, clean=None, hist=None, limit=0, stats=None, hists=None):
    """the loop of ctx_links.c over a .ctp body -> (ctp text, list text, stats, hists).  `text` is bytes; the list text
    has no header line.  stats / hists: accumulate into these."""
    stats = stats if stats is not None else new_stats()
    if hist is not None and hists is None:
        hists = [[0] * hist[1] for _ in range(hist[0])]
    ctp, lst = [], []
    tree = LinkTree(k)
    lines, off = [], 0
    for ln in text.decode().split("\n")[:-1] if text.endswith(b"\n") else text.decode().split("\n"):
        lines.append((off, ln))
        off += len(ln) + 1
    i, knum = 0, 0
    while not limit or knum < limit:
        tree.reset()
        while i < len(lines) and (lines[i][1] == "" or lines[i][1][0] == "#"):
            i += 1
        if i == len(lines):
            break
        if lines[i][1][0] not in "ACGT":
            raise BadLine("link_before_kmer" if knum == 0 else "bad_orient", lines[i][0])
        kmer = parse_kmer_line(lines[i][1], k, lines[i][0])
        i += 1
        stats["kmers_read"] += 1
        while i < len(lines):
            off, ln = lines[i]
            if ln == "" or ln[0] == "#":
                i += 1
                continue
            if ln[0] in "ACGT":
                break
            fw, covg, juncs, seq, pos = parse_link_line(ln, k, off)
            tree.add(fw, covg, pos, juncs, seq)
            stats["links_in"] += 1
            i += 1
        if hist is not None:
            tree.update_covg_hists(hists, hist[0], hist[1])
        if clean is not None:
            tree.clean(clean)
        init = stats["num_links"]
        stats["tree_links"] += tree.ntree
        tree.get_stats(stats)
        num_links = stats["num_links"] - init
        tree.write_list(lst)
        if num_links:
            tree.write_ctp(kmer, num_links, ctp)
        knum += 1
    return "".join(ctp).encode(), "".join(lst).encode(), stats, hists


def hist_csv(hists, distsize, covgsize):
    """ctx_links.c:398-411"""
    out = ["  " + "".join(",covg.%02d" % j for j in range(1, covgsize)) + "\n"]
    for i in range(1, distsize):
        out.append("dist.%02d" % i + "".join(",%d" % hists[i][j] for j in range(1, covgsize)) + "\n")
    return "".join(out)


def threshold_text(hists, covgsize, pick):
    """print_suggest_cutoff (ctx_links.c:82-115) as ctx_links.c:416 calls it: six distances whatever -D says.
    pick: cleaning_pick_kmer_threshold over one row (clean_restate.pick_threshold)"""
    cutoffs, sums = [], []
    for dist in range(1, 6):
        t = pick(hists[dist][:covgsize])
        cutoffs.append(max(t, 0))
        sums.append(sum(hists[dist][:covgsize]))
    return "sumcovgs=%s\ncutoffs=%s\nsuggested_cutoff=%d\n" % (",".join(map(str, sums)), ",".join(map(str, cutoffs)), sorted(cutoffs)[2])
