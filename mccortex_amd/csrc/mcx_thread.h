// mcx_thread.h -- `thread` on the device (included by mcx_api.hip).
//
// ctx_thread.c without -p and without -u: reads are laid over the graph as `correct` lays them (passes A-C of
// mcx_correct.h, k_cr_tasks without the two end extensions) and the links of every contig are generated
// (src/tools/generate_paths.c), counted and written as .ctp text (gpath_save_sbuf).  The walkers hold no paths
// (gpath_store_split_read_write, ctx_thread.c:233-234), so the links depend on the graph and the reads alone.
// The graph has one colour; a degree counts the edges whose k-mer is a key (AN EDGE THAT NAMES AN ABSENT K-MER COUNTS AS
// NO EDGE).  The passes behind A-C ("thread's device passes"):
//   D. k_th_nodes   a wave per read: its contigs (correct_alignment_nxt:361-510) as one run of node references, aligned
//                   nodes from node[], walked nodes from the ranges of the filled gap tasks; per node the start of its
//                   contig, per contig start its end; the contig histogram.  Counted first, then, behind a scan, written.
//   E. k_th_junc    a thread per node: forward and reverse junction (worker_contig_to_junctions:351-378) with its base;
//                   two scans rank the junctions of the batch
//      k_th_pack    the bases by rank, 2 bits each, most significant first: the forward ones ascending, the reverse ones
//                   descending and complemented, so every link of a contig is a run of one of the two arrays
//   F. k_th_links   a thread per node: the link a reverse junction adds forward and the one a forward junction adds
//                   backward (_juncs_to_paths:204-231 with the step back of :217) as records that VIEW the packed
//                   arrays at a 2-bit offset; no link's bases are copied before equal links are counted
//   G. sort and reduce (sort_perm_by_words): the key is the k-mer's words shifted up by the orientation bit, as many
//      junction words as the longest link needs, zero padded (k_th_word reads them through the view), then the length:
//      gpath_cmp inside a k-mer, key order across k-mers, exact for links of any length.  k_th_heads, a scan, k_th_runs,
//      k_th_reduce (counts added, saturating at 255) and k_th_copy (the unique links' bases into a pool of their own).
//      The store on the handle is a list of such sorted segments; they are merged by the same sort and reduce once the
//      pending links outgrow the merged ones, and before anything is read.
//   H. k_th_text    four lanes per stored link, one successor candidate each, walk gpath_fetch (gpath_checks.c:199-234):
//                   first the line's length, then, behind a 64-bit scan, the line itself
// All are grid-stride loops (the "grid" knob caps the launches); the table is only read.
#pragma once
#include "mcx_correct.h"

namespace mcx {

constexpr uint32_t kThMaxJuncs = 32767;  // GPATH_MAX_JUNCS
constexpr uint32_t kThMaxSeen = 255;     // GPATH_MAX_SEEN
enum : uint32_t { kThContigs = 0, kThContigKmers, kThJuncsFw, kThJuncsRv, kThLinks, kThNumCounters, kThMaxNodes = kThNumCounters, kThMaxLen, kThAllCounters };

// A link: kw = (key << 1 | orientation) as a number of W words (kw[0] most significant, the words behind W are 0), its
// bases a view of `len` 2-bit codes from code `start` of `base` on.  len = 0: no link (kw[0] = all ones sorts it last).
struct ThLink {
  uint64_t kw[4];
  const uint64_t *base;
  uint64_t start;
  uint32_t len, cnt;
};

// junction word j (32 bases, the first in the top bits) of a link, zero behind its end
__device__ __forceinline__ uint64_t th_word(const ThLink &L, uint32_t j)
{
  if ((uint64_t)j * 32u >= L.len) return 0;
  const uint64_t s = L.start + (uint64_t)j * 32u, q = s >> 5;
  const uint32_t sh = 2u * (uint32_t)(s & 31u), rem = L.len - j * 32u;
  uint64_t w = L.base[q] << sh;
  if (sh) w |= L.base[q + 1] >> (64u - sh);  // (the arrays are padded by a word)
  if (rem < 32u) w &= ~0ull << (64u - 2u * rem);
  return w;
}
__device__ __forceinline__ uint32_t th_base(const ThLink &L, uint32_t i)
{
  const uint64_t s = L.start + i;
  return (uint32_t)(L.base[s >> 5] >> (62u - 2u * (uint32_t)(s & 31u))) & 3u;
}

// D. A wave per read.  WRITE = false: nnode[r]; WRITE = true: the nodes from noff[r] on.  ctr[kThMaxNodes] = the most
// nodes of a read (the histogram's bound).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_th_nodes(CrView x, TableView t, const CrTask *tasks, const CrRes *res, const uint64_t *refs, const uint64_t *toff,
                                                  const uint64_t *noff, uint64_t *nnode, uint64_t *cn, uint64_t *cs, uint64_t *cend,
                                                  unsigned long long *hist, unsigned long long *ctr)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  unsigned long long c_contigs = 0, c_nodes = 0, c_max = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < x.nreads; r += nwaves) {
    const uint64_t len = cr_len(x, r), p0 = x.boff[r] - x.boff[0], k = (uint64_t)x.k;
    const uint64_t nk = len >= k ? len - k + 1 : 0, base = WRITE ? noff[r] : 0;
    uint64_t tk = toff[r], n = 0, start = 0, prev = 0, prevref = 0, first = kCrNone;
    auto close = [&]() {  // the contig [start, n) ends
      if (WRITE && lane == 0) {
        cend[base + start] = base + n;
        atomicAdd(&hist[n - start], 1ull);
        c_contigs++;
      }
      start = n;
    };
    cr_for_aligned(x, p0, nk, lane, [&](uint64_t i, uint64_t ref) {
      if (first == kCrNone) first = i;
      else if (i != prev + 1) {
        const CrTask T = tasks[tk];
        const CrRes R = res[tk];
        tk++;
        if (R.ok) {
          const uint64_t fill = (uint64_t)R.nfront + R.nback;
          if (WRITE)
            for (uint64_t j = lane; j < fill; j += 64) {  // (walker 1 kept its nodes turned round)
              const bool back = j >= R.nfront;
              const uint64_t at = back ? (uint64_t)T.cap - R.nback + (j - R.nfront) : j;
              cn[base + n + j] = refs[T.off + at] ^ (back ? 1ull : 0ull);
              cs[base + n + j] = base + start;
            }
          n += fill;
        } else close();
      } else {  // db_alignment_next_gap:166-173
        const uint32_t e = (uint32_t)*val_ptr(t, prevref >> 1, 0) & 0xffu;
        const uint32_t nuc = base_code(x.seq[p0 + i + k - 1]);
        if (!((e >> (4u * (uint32_t)(prevref & 1u) + nuc)) & 1u)) close();
      }
      if (WRITE && lane == 0) { cn[base + n] = ref; cs[base + n] = base + start; }
      n++;
      prev = i;
      prevref = ref;
    });
    if (first != kCrNone) close();
    if (lane == 0) {
      if (!WRITE) { nnode[r] = n; c_max = n > c_max ? n : c_max; }
      else c_nodes += n;
    }
  }
  if (WRITE) {
    block_add(&ctr[kThContigs], c_contigs);
    block_add(&ctr[kThContigKmers], c_nodes);
  } else if (c_max) atomicMax(&ctr[kThMaxNodes], c_max);
}

// edges of (key, o) whose k-mer is a key
template <int W> __device__ __forceinline__ uint32_t th_degree(const TableView &t, const Kmer<W> &key, uint32_t e8, uint32_t o, int k)
{
  const uint32_t nib = (e8 >> (4u * o)) & 15u;
  if (!(nib & (nib - 1u))) return nib ? 1u : 0u;  // (what a single edge names is not looked up: one is no junction either way)
  uint32_t d = 0;
  for (uint32_t b = 0; b < 4; b++)
    if ((nib >> b) & 1u) {
      uint32_t p;
      d += cl_next<W>(t, key, o, b, k, p) != kNoSlot;
    }
  return d;
}

// E. per node: is it a forward / a reverse junction of its contig, and the base
template <int W>
__global__ __launch_bounds__(256) void k_th_junc(TableView t, int k, const uint64_t *cn, const uint64_t *cs, const uint64_t *cend, uint64_t nn, uint8_t *fwf,
                                                 uint8_t *rvf, uint8_t *fwb, uint8_t *rvb, unsigned long long *ctr)
{
  unsigned long long c_fw = 0, c_rv = 0;
  for (uint64_t i = cl_first(); i < nn; i += cl_stride()) {
    const uint64_t s = cs[i], e = cend[s], ref = cn[i];
    const uint32_t o = (uint32_t)(ref & 1u);
    const uint32_t e8 = (uint32_t)*val_ptr(t, ref >> 1, 0) & 0xffu;
    const Kmer<W> key = cl_key<W>(t, ref >> 1);
    uint8_t f = 0, r = 0, fb = 0, rb = 0;
    if (i + 1 < e && th_degree<W>(t, key, e8, o, k) > 1) {
      const uint64_t nx = cn[i + 1];
      f = 1;
      fb = (uint8_t)cr_last_nuc<W>(cl_key<W>(t, nx >> 1), (uint32_t)(nx & 1u), k);
    }
    if (i > s && th_degree<W>(t, key, e8, o ^ 1u, k) > 1) {
      const uint64_t pv = cn[i - 1];
      r = 1;
      rb = (uint8_t)cr_first_nuc<W>(cl_key<W>(t, pv >> 1), (uint32_t)(pv & 1u), k);
    }
    fwf[i] = f; rvf[i] = r; fwb[i] = fb; rvb[i] = rb;
    c_fw += f;
    c_rv += r;
  }
  block_add(&ctr[kThJuncsFw], c_fw);
  block_add(&ctr[kThJuncsRv], c_rv);
}

// the bases by rank into the zeroed arrays pf (ascending) and pr (descending, complemented)
__global__ __launch_bounds__(256) void k_th_pack(const uint8_t *fwf, const uint8_t *rvf, const uint8_t *fwb, const uint8_t *rvb, const uint64_t *fwx,
                                                 const uint64_t *rvx, uint64_t nn, unsigned long long *pf, unsigned long long *pr)
{
  const uint64_t nrv = rvx[nn];
  for (uint64_t i = cl_first(); i < nn; i += cl_stride()) {
    if (fwf[i]) {
      const uint64_t q = fwx[i];
      atomicOr(&pf[q >> 5], (unsigned long long)fwb[i] << (62u - 2u * (uint32_t)(q & 31u)));
    }
    if (rvf[i]) {
      const uint64_t q = nrv - 1 - rvx[i];
      atomicOr(&pr[q >> 5], (unsigned long long)(3u - rvb[i]) << (62u - 2u * (uint32_t)(q & 31u)));
    }
  }
}

template <int W> __device__ __forceinline__ void th_set_kw(const TableView &t, ThLink &L, uint64_t ref)
{
  const Kmer<W> key = cl_key<W>(t, ref >> 1);
  for (int j = 0; j < 4; j++) L.kw[j] = 0;
  for (int j = 0; j < W; j++) L.kw[j] = (key.w[j] << 1) | (j + 1 < W ? key.w[j + 1] >> 63 : (ref & 1ull));
}

// F. links[rvx[i]] = the forward link of the reverse junction at i, links[nrv + fwx[i]] = the reverse link of the
// forward junction at i.  fwx and rvx are the exclusive sums of the flags over the nn + 1 positions.
template <int W>
__global__ __launch_bounds__(256) void k_th_links(TableView t, const uint64_t *cn, const uint64_t *cs, const uint64_t *cend, const uint8_t *fwf,
                                                  const uint8_t *rvf, const uint64_t *fwx, const uint64_t *rvx, uint64_t nn, uint32_t max_juncs,
                                                  const uint64_t *pf, const uint64_t *pr, ThLink *links, unsigned long long *ctr)
{
  const uint64_t nrv = rvx[nn];
  unsigned long long c_links = 0, c_len = 0;
  for (uint64_t i = cl_first(); i < nn; i += cl_stride()) {
    if (!fwf[i] && !rvf[i]) continue;
    const uint64_t s = cs[i], e = cend[s];
    const bool both = fwx[e] > fwx[s] && rvx[e] > rvx[s];  // worker_contig_to_junctions:383
    if (rvf[i]) {
      ThLink L;
      L.kw[0] = ~0ull; L.kw[1] = L.kw[2] = L.kw[3] = 0; L.base = pf; L.start = 0; L.len = 0; L.cnt = 0;
      if (both && fwx[e] > fwx[i]) {  // a forward junction at i or behind it (:207-211); the one at i - 1 comes with it (:217)
        th_set_kw<W>(t, L, cn[i - 1]);
        L.start = fwx[i - 1];
        L.len = (uint32_t)min(fwx[e] - fwx[i - 1], (uint64_t)max_juncs);
        L.cnt = 1;
        c_links++;
        c_len = max(c_len, (unsigned long long)L.len);
      }
      links[rvx[i]] = L;
    }
    if (fwf[i]) {
      ThLink L;
      L.kw[0] = ~0ull; L.kw[1] = L.kw[2] = L.kw[3] = 0; L.base = pr; L.start = 0; L.len = 0; L.cnt = 0;
      if (both && rvx[i + 1] > rvx[s]) {  // a reverse junction at i or before it; the one at i + 1 comes with it
        th_set_kw<W>(t, L, cn[i + 1] ^ 1ull);
        L.start = nrv - rvx[i + 2];
        L.len = (uint32_t)min(rvx[i + 2] - rvx[s], (uint64_t)max_juncs);
        L.cnt = 1;
        c_links++;
        c_len = max(c_len, (unsigned long long)L.len);
      }
      links[nrv + fwx[i]] = L;
    }
  }
  block_add(&ctr[kThLinks], c_links);
  if (c_len) atomicMax(&ctr[kThMaxLen], c_len);
}

// G. word w of the sort key of links[through[i]]: W words of kw, nj junction words, the length
__global__ __launch_bounds__(256) void k_th_word(const ThLink *links, const uint64_t *through, uint32_t w, uint32_t W, uint32_t nj, uint64_t *dst, uint64_t n)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const ThLink &L = links[through[i]];
    dst[i] = w < W ? L.kw[w] : w < W + nj ? th_word(L, w - W) : (uint64_t)L.len;
  }
}

__device__ __forceinline__ bool th_same(const ThLink &a, const ThLink &b)
{
  if (a.kw[0] != b.kw[0] || a.kw[1] != b.kw[1] || a.kw[2] != b.kw[2] || a.kw[3] != b.kw[3] || a.len != b.len) return false;
  for (uint32_t j = 0; j * 32u < a.len; j++)
    if (th_word(a, j) != th_word(b, j)) return false;
  return true;
}
// head[i] = 1 where sorted item i is another link than item i - 1; head[n] = 0 for the scan
__global__ __launch_bounds__(256) void k_th_heads(const ThLink *links, const uint64_t *perm, uint64_t n, uint8_t *head)
{
  for (uint64_t i = cl_first(); i <= n; i += cl_stride()) head[i] = i == n ? 0 : i == 0 ? 1 : th_same(links[perm[i]], links[perm[i - 1]]) ? 0 : 1;
}
// ex = exclusive sum of head: runstart[run] = its first item, runstart[nruns] = n
__global__ __launch_bounds__(256) void k_th_runs(const uint8_t *head, const uint64_t *ex, uint64_t n, uint64_t *runstart)
{
  for (uint64_t i = cl_first(); i <= n; i += cl_stride())
    if (i == n || head[i]) runstart[ex[i]] = i;
}
// per run the unique link with its count (a view still) and the words its bases take
__global__ __launch_bounds__(256) void k_th_reduce(const ThLink *links, const uint64_t *perm, const uint64_t *runstart, uint64_t nruns, ThLink *out,
                                                   uint64_t *nwords)
{
  for (uint64_t u = cl_first(); u <= nruns; u += cl_stride()) {
    if (u == nruns) { nwords[u] = 0; continue; }
    ThLink L = links[perm[runstart[u]]];
    uint32_t c = 0;
    for (uint64_t i = runstart[u]; i < runstart[u + 1]; i++) c = min(kThMaxSeen, c + links[perm[i]].cnt);
    L.cnt = c;
    out[u] = L;
    nwords[u] = (L.len + 31u) / 32u;
  }
}
// the bases of every unique link into the pool, each from a word boundary on
__global__ __launch_bounds__(256) void k_th_copy(ThLink *out, const uint64_t *woff, uint64_t nruns, uint64_t *pool)
{
  for (uint64_t u = cl_first(); u < nruns; u += cl_stride()) {
    ThLink L = out[u];
    for (uint32_t j = 0; j * 32u < L.len; j++) pool[woff[u] + j] = th_word(L, j);
    out[u].base = pool;
    out[u].start = woff[u] * 32u;
  }
}

// same k-mer: kw without the orientation bit
__device__ __forceinline__ bool th_same_kmer(const ThLink &a, const ThLink &b, uint32_t W)
{
  for (uint32_t j = 0; j < W; j++)
    if ((a.kw[j] ^ b.kw[j]) & (j + 1 == W ? ~1ull : ~0ull)) return false;
  return true;
}
// out[0] += k-mers with links, out[1] += bytes of the packed bases ((njuncs + 3) / 4 each)
__global__ __launch_bounds__(256) void k_th_info(const ThLink *links, uint64_t n, uint32_t W, unsigned long long *out)
{
  unsigned long long c_k = 0, c_b = 0;
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    c_k += i == 0 || !th_same_kmer(links[i], links[i - 1], W);
    c_b += (links[i].len + 3u) / 4u;
  }
  block_add(&out[0], c_k);
  block_add(&out[1], c_b);
}

__device__ __forceinline__ uint32_t th_digits(uint64_t v)
{
  uint32_t d = 1;
  while (v >= 10) { v /= 10; d++; }
  return d;
}
__device__ __forceinline__ void th_put_num(uint8_t *p, uint64_t v, uint32_t d)
{
  for (uint32_t i = d; i-- > 0; v /= 10) p[i] = (uint8_t)('0' + v % 10);
}
// base i (0 = the first) of a k-mer
template <int W> __device__ __forceinline__ uint32_t th_kmer_base(const Kmer<W> &x, int k, int i)
{
  const int bit = 2 * (k - 1 - i);
  return (uint32_t)(x.w[W - 1 - (bit >> 6)] >> (bit & 63)) & 3u;
}

// H. Four lanes per link (the links are sorted and unique).  EMIT = false: len[i] = the bytes of link i's line, with
// the `<kmer> <nlinks>` line before it when it is its k-mer's first.  EMIT = true: the lines at out + off[i].
template <int W, bool EMIT>
__global__ __launch_bounds__(256) void k_th_text(TableView t, int k, const ThLink *links, uint64_t n, uint32_t flags, uint64_t *len, const uint64_t *off,
                                                 uint8_t *out)
{
  const uint32_t lane = threadIdx.x & 63u, sub = lane & 3u, g0 = lane & ~3u;
  const uint64_t per_block = blockDim.x >> 2;
  const bool seq = flags & 1u;
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < n; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t i = base + (threadIdx.x >> 2);
    const bool have = i < n;
    ThLink L;
    L.kw[0] = L.kw[1] = L.kw[2] = L.kw[3] = 0; L.base = nullptr; L.start = 0; L.len = 0; L.cnt = 0;
    if (have) L = links[i];
    Kmer<W> key;
    for (int j = 0; j < W; j++) key.w[j] = (L.kw[j] >> 1) | (j ? L.kw[j - 1] << 63 : 0ull);
    uint32_t o = (uint32_t)(L.kw[W - 1] & 1ull);
    uint64_t o_at = 0;  // bytes written (or counted) so far
    uint8_t *dst = EMIT && have ? out + off[i] : nullptr;
    if (have && (i == 0 || !th_same_kmer(L, links[i - 1], (uint32_t)W))) {
      uint64_t nl = 1;
      while (i + nl < n && th_same_kmer(L, links[i + nl], (uint32_t)W)) nl++;
      const uint32_t d = th_digits(nl);
      if (EMIT) {
        for (int j = (int)sub; j < k; j += 4) dst[j] = (uint8_t)"ACGT"[th_kmer_base<W>(key, k, j)];
        if (sub == 0) { dst[k] = ' '; th_put_num(dst + k + 1, nl, d); dst[k + 1 + d] = '\n'; }
      }
      o_at += (uint64_t)k + 2 + d;
    }
    if (have) {  // <F|R> <njuncs> <nseen> <juncs>
      const uint32_t d1 = th_digits(L.len), d2 = th_digits(L.cnt);
      if (EMIT) {
        uint8_t *p = dst + o_at;
        if (sub == 0) {
          p[0] = o ? 'R' : 'F'; p[1] = ' ';
          th_put_num(p + 2, L.len, d1); p[2 + d1] = ' ';
          th_put_num(p + 3 + d1, L.cnt, d2); p[3 + d1 + d2] = ' ';
        }
        for (uint32_t j = sub; j < L.len; j += 4) p[4 + d1 + d2 + j] = (uint8_t)"ACGT"[th_base(L, j)];
      }
      o_at += 4ull + d1 + d2 + L.len;
    }
    // gpath_fetch: the nodes from the oriented k-mer on, a junction base taken where there are several successors
    bool live = have && seq;
    uint64_t slot = kNoSlot;
    if (live) {
      uint32_t novel = 0, full = 0;
      slot = find_or_insert_rec<W>(t, key, true, novel, full);  // must_exist: read-only
      if (EMIT) {
        if (sub == 0) memcpy(dst + o_at, " seq=", 5);
        const Kmer<W> first = o ? revcomp<W>(key, k) : key;
        for (int j = (int)sub; j < k; j += 4) dst[o_at + 5 + j] = (uint8_t)"ACGT"[th_kmer_base<W>(first, k, j)];
      }
      o_at += 5ull + (uint64_t)k;
    }
    // the positions are written behind the sequence, whose length the first pass has left in len[i]'s place: the emit
    // pass walks twice, once for the bases and once for the positions
    for (int pass = 0; pass < (EMIT ? 2 : 1); pass++) {
      Kmer<W> wk = key;
      uint64_t ws = slot;
      uint32_t wo = o, nj = 0;
      uint64_t nn = 1, jp = 0;  // nodes so far; bytes of the positions
      bool go = live && ws != kNoSlot;
      while (__builtin_amdgcn_ballot_w64(go && nj < L.len)) {  // (the same for the whole wave: the votes cross lanes)
        const bool act = go && nj < L.len;
        uint64_t nslot = kNoSlot;
        if (act) {
          const uint32_t e = (uint32_t)*val_ptr(t, ws, 0) & 0xffu;
          if ((e >> (4u * wo + sub)) & 1u) { uint32_t p; nslot = cl_next<W>(t, wk, wo, sub, k, p); }
        }
        const uint32_t F = (uint32_t)(__builtin_amdgcn_ballot_w64(nslot != kNoSlot) >> g0) & 15u;
        int choice = -1;
        bool junc = false;
        if (act && F) {
          if (F & (F - 1u)) {
            const uint32_t b = th_base(L, nj);
            if ((F >> b) & 1u) { choice = (int)b; junc = true; }
          } else choice = __builtin_ctz(F);
        }
        const uint64_t cslot = (uint64_t)__shfl((unsigned long long)nslot, (int)g0 + (choice < 0 ? 0 : choice));
        if (act && choice >= 0) {
          if (junc) {
            const uint32_t d = th_digits(nn - 1);
            if (EMIT && pass == 1 && sub == 0) {
              uint8_t *p = dst + o_at + jp;
              if (nj) *p++ = ',';
              th_put_num(p, nn - 1, d);
            }
            jp += d + (nj ? 1u : 0u);
            nj++;
          }
          uint32_t p;
          wk = cr_neighbour<W>(wk, wo, (uint32_t)choice, k, p);
          wo = p;
          ws = cslot;
          if (EMIT && pass == 0 && sub == 0) dst[o_at + nn - 1] = (uint8_t)"ACGT"[cr_last_nuc<W>(wk, wo, k)];
          nn++;
        } else if (act) go = false;  // a dead end, or a base that no successor has: the reference asserts there is none
      }
      if (live && (pass == 0)) {
        o_at += nn - 1;
        if (EMIT && sub == 0) memcpy(dst + o_at, " juncpos=", 9);
        o_at += 9;
        if (!EMIT) o_at += jp;
      } else if (live) o_at += jp;
    }
    if (have) {
      if (EMIT) { if (sub == 0) dst[o_at] = '\n'; }
      else if (sub == 0) len[i] = o_at + 1;
    }
  }
}

}  // namespace mcx
