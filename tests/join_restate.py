"""Dictionary restatement of `join` (src/commands/ctx_join.c, graph_writer_merge_mkhdr, graph_load), built on
oracle/ctxio.py.  Two levels:

  join_records   what the device engine computes: bodies + colour filters in, the sorted body and the counts out
  join_command   what `mccortex<K> join` writes: argument strings ("3:in.ctx:0,1") and -i arguments in, header bytes and
                 sorted body out -- colour offsets, the swap of the smallest intersection graph to the front, the
                 intersection name in the header, when the k-mers nobody supplies are written

Semantics restated (include/mcx_gpu.h, the `join` section):
  - a record is dropped when its coverage is zero in every colour its file's filter selects (keep_kmer);
  - covg[into] is the sum saturating at 2^32 - 1, edges[into] the OR, over every (record, filter pair);
  - with intersection graphs a key is kept iff every one of them has it (after the drop rule); every output colour's
    edges are ANDed with the OR, over the selected colours, of the edges intersection source 0 has for the key;
    keep_empty writes the keys of the intersection that no input supplies as all-zero records.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ctxio  # noqa: E402

U32 = 0xFFFFFFFF
STATS = ("recs_read", "recs_kept", "isec_recs_read", "isec_recs_kept", "kmers_written", "kmers_intersection",
         "kmers_written_no_covg")


def pack(recs, k, ncols):
    """[(key int, [covg], [edges])] -> .ctx body bytes in the order given (key words most significant first)"""
    W = ctxio.words_for_k(k)
    rs = 8 * W + 5 * ncols
    out = np.zeros((len(recs), rs), dtype=np.uint8)
    for i, (key, cv, ed) in enumerate(recs):
        words = [(key >> (64 * (W - 1 - w))) & 0xFFFFFFFFFFFFFFFF for w in range(W)]
        out[i, :8 * W] = np.array(words, dtype="<u8").view(np.uint8)
        out[i, 8 * W:8 * W + 4 * ncols] = np.array(cv, dtype="<u4").view(np.uint8)
        out[i, 8 * W + 4 * ncols:] = np.array(ed, dtype=np.uint8)
    return out.tobytes()


def parse(body, k, ncols):
    """.ctx body bytes -> [(key int, [covg], [edges])] in file order"""
    W = ctxio.words_for_k(k)
    hdr = dict(num_words=W, num_cols=ncols)
    keys, cv, ed = ctxio.records(body, hdr, 0)
    assert len(body) == len(keys) * (8 * W + 5 * ncols)
    kl, cl, el = keys.tolist(), cv.tolist(), ed.tolist()
    out = []
    for i in range(len(kl)):
        key = 0
        for w in kl[i]:
            key = (key << 64) | w
        out.append((key, cl[i], el[i]))
    return out


def join_records(k, out_ncols, inputs, isecs=(), keep_empty=False):
    """inputs, isecs: [(body bytes, file_ncols, [(from, into)])], isecs in rank order (their `into` is not read)
    -> (sorted body bytes, stats dict, {key: (covg, edges)})"""
    st = dict.fromkeys(STATS, 0)
    present, mask = [], {}
    for rank, (body, nc, filt) in enumerate(isecs):
        sel = [f for f, _ in filt]
        have = set()
        for key, cv, ed in parse(body, k, nc):
            st["isec_recs_read"] += 1
            if not any(cv[f] for f in sel):
                continue
            st["isec_recs_kept"] += 1
            have.add(key)
            if rank == 0:
                m = mask.get(key, 0)
                for f in sel:
                    m |= ed[f]
                mask[key] = m
        present.append(have)
    isec = set.intersection(*present) if present else None
    out = {}
    for body, nc, filt in inputs:
        for key, cv, ed in parse(body, k, nc):
            st["recs_read"] += 1
            if not any(cv[f] for f, _ in filt):
                continue
            st["recs_kept"] += 1
            if isec is not None and key not in isec:
                continue
            c, e = out.setdefault(key, ([0] * out_ncols, [0] * out_ncols))
            m = mask[key] if isec is not None else 0xFF
            for f, t in filt:
                c[t] = min(U32, c[t] + cv[f])
                e[t] |= ed[f] & m
    if isec is not None:
        st["kmers_intersection"] = len(isec)
        if keep_empty:
            for key in isec:
                if key not in out:
                    out[key] = ([0] * out_ncols, [0] * out_ncols)
                    st["kmers_written_no_covg"] += 1
    st["kmers_written"] = len(out)
    body = pack([(key, out[key][0], out[key][1]) for key in sorted(out)], k, out_ncols)
    return body, st, out


def _open(arg, files, into_offset):
    path = ctxio.parse_filter(arg, 1 << 20, 0)[0]
    buf = files[path]
    hdr, hs = ctxio.read_header(buf)
    _, filt = ctxio.parse_filter(arg, hdr["num_cols"], into_offset)
    return hdr, buf[hs:], filt


def join_command(args, files, isec_args=(), sort=False):
    """args / isec_args: the command's graph and -i arguments, files: {path: file bytes}
    -> (header bytes, sorted body bytes, stats, out_ncols)"""
    opened, ncols = [], 0
    for a in args:  # graph_files_open: each file starts at the running maximum of into_ncols
        hdr, body, filt = _open(a, files, ncols)
        ncols = max(ncols, max(t for _, t in filt) + 1)
        opened.append((hdr, body, filt))
    k = opened[0][0]["kmer_size"]
    W = ctxio.words_for_k(k)
    iopened, smallest = [], 0
    for i, a in enumerate(isec_args):
        hdr, body, filt = _open(a, files, 0)
        n = len(body) // (8 * W + 5 * hdr["num_cols"])
        iopened.append((hdr, body, filt))
        if i == 0:
            smallest = n
        elif n < smallest:  # ctx_join.c:150-158
            iopened[i], iopened[0] = iopened[0], iopened[i]
            smallest = n
    ginfos = [ctxio.GraphInfo() for _ in range(ncols)]
    loaded = set()
    for hdr, _, filt in opened:
        for f, t in filt:
            ginfos[t].merge(hdr["ginfo"][f])
            loaded.add(t)
    if iopened:
        name = ""
        for hdr, _, _ in iopened:  # graph_info_make_intersect on header colour 0
            g = hdr["ginfo"][0]
            name += ("," if name else "") + g.sample_name
            if g.cleaning.is_graph_intersection:
                name += "," + g.cleaning.intersection_name
        for t in sorted(loaded):  # graph_info_append_intersect
            c = ginfos[t].cleaning
            c.intersection_name = name if not c.is_graph_intersection else c.intersection_name + "," + name
            c.is_graph_intersection = 1
    keep_empty = bool(iopened) and (len(opened) > 1 or sort)
    body, st, _ = join_records(k, ncols, [(b, h["num_cols"], f) for h, b, f in opened],
                               [(b, h["num_cols"], f) for h, b, f in iopened], keep_empty)
    return ctxio.header_bytes(k, ginfos), body, st, ncols
