// mcx_links.h -- `links` on the device (included by mcx_api.hip, behind the sort and scan helpers it uses).
//
// ctx_links.c over the body of a version-4 .ctp file: per k-mer and orientation the links form a trie of junction
// strings with summed counts (src/paths/link_tree.c).  Over the links sorted by junction string the trie is a list of
// longest-common-prefix values: a TREE LINK (a distinct prefix) is a pair (i, d) with lcp[i] < d <= len[i], its count
// is S[e] - S[i] (S the exclusive sum of the counts, e the first j > i whose lcp is below d or that leaves the group)
// and its distance is juncpos[d - 1] of link i.  No table and no binary k-mers: a k-mer is its ordinal in the piece.
// The passes ("links' device passes"), all grid-stride loops:
//   1. k_lk_mark, k_lk_starts, k_lk_class   line starts; every line a k-mer, a link, a comment or empty; two scans
//                    give a link line its k-mer ordinal and its rank among the link lines
//   2. k_lk_parse    a thread per line: the columns of a link line, every refusal of link_line_parse and
//                    gpath_reader_read_kmer (the smallest offset wins through an atomic min); behind a scan of the
//                    lengths k_lk_store packs the junctions 2 bits each from a word boundary on and puts juncpos as
//                    u32 into a pool
//   3. sort_perm_by_words by (ordinal << 1 | orientation, junction words zero padded to the longest link, length):
//      a prefix sorts before its extensions, which follow it without a gap
//   4. k_lk_heads, a scan, k_th_runs, k_lk_reduce: equal links are one link, the counts added in 64 bits;
//      k_lk_lcp (word compare and count-leading-zeros), the maximal flag, S[] by a scan
//   5. k_lk_ns       ns[j] = the first j' > j with lcp[j'] < lcp[j], by rounds of pointer jumping;
//      k_lk_tree     a thread per link walks d downward with one forward cursor that skips subtrees through ns[]:
//                    count, distance, histogram (privatised in LDS where it fits) and the length of the list row
//   6. k_lk_written, k_lk_groups, k_lk_stats   which links are written (maximal in the input, count >= cut-off), per
//                    k-mer how many, the totals
//   7. k_lk_text, k_lk_list   length pass, 64-bit scan, emit pass: the .ctp lines (juncs, seq= and juncpos= copied
//                    from the link's own input line) and the list rows
// Links of a group that share a junction prefix but disagree on the seq or juncpos of that prefix are outside the
// contract: the reference keeps whichever came first, here a tree link takes the juncpos of the first link in sorted
// order that has it.  A written link is always a whole input link with its own seq= and juncpos=.  seq= is checked
// at the junction positions only.
#pragma once
#include "mcx_thread.h"

namespace mcx {

enum : uint32_t { kLkKmersWithLinks = 0, kLkLinks, kLkBytes, kLkMaxLen, kLkChanged, kLkNumCounters };
constexpr uint64_t kLkNoErr = ~0ull;

// a parsed link line; the offsets are bytes from the start of the piece
struct LkLink {
  uint64_t line, cnt, woff /* junction words in the pool */, poff /* juncpos in the pool */, key /* ordinal << 1 | orientation */;
  uint32_t len, junc_at, seq_at, seq_len, jp_at, jp_len;  // (relative to `line`)
};

__device__ __forceinline__ bool lk_acgt(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
__device__ __forceinline__ bool lk_digit(uint8_t c) { return c >= '0' && c <= '9'; }
__device__ __forceinline__ void lk_fail(unsigned long long *err, uint64_t off, uint32_t code) { atomicMin(err, (unsigned long long)((off << 8) | code)); }

// 1. flag[i] = a line starts at byte i; flag[n] = 0 for the scan
__global__ __launch_bounds__(256) void k_lk_mark(const uint8_t *text, uint64_t n, uint8_t *flag)
{
  for (uint64_t i = cl_first(); i <= n; i += cl_stride()) flag[i] = i < n && (i == 0 || text[i - 1] == '\n');
}
__global__ __launch_bounds__(256) void k_lk_starts(const uint8_t *flag, const uint64_t *lidx, uint64_t n, uint64_t *lstart)
{
  for (uint64_t i = cl_first(); i <= n; i += cl_stride())
    if (i == n || flag[i]) lstart[lidx[i]] = i;
}
// per line: is it a k-mer line, is it a link line (anything that is no k-mer line, no comment and not empty)
__global__ __launch_bounds__(256) void k_lk_class(const uint8_t *text, const uint64_t *lstart, uint64_t nlines, uint8_t *kflag, uint8_t *lflag)
{
  for (uint64_t l = cl_first(); l <= nlines; l += cl_stride()) {
    uint8_t kf = 0, lf = 0;
    if (l < nlines && lstart[l + 1] - lstart[l] > 1) {
      const uint8_t c = text[lstart[l]];
      if (lk_acgt(c)) kf = 1;
      else if (c != '#') lf = 1;
    }
    kflag[l] = kf;
    lflag[l] = lf;
  }
}
// kline[ordinal] = the line of that k-mer
__global__ __launch_bounds__(256) void k_lk_klines(const uint8_t *kflag, const uint64_t *kx, uint64_t nlines, uint64_t *kline)
{
  for (uint64_t l = cl_first(); l < nlines; l += cl_stride())
    if (kflag[l]) kline[kx[l]] = l;
}

// one comma list of numbers in [p, e): calls f(i, v) per item (v saturates at 2^32 - 1); false when an item is no number
template <class F> __device__ __forceinline__ bool lk_numbers(const uint8_t *t, uint64_t p, uint64_t e, uint32_t &count, F f)
{
  count = 0;
  while (true) {
    uint64_t v = 0;
    uint32_t nd = 0;
    while (p < e && lk_digit(t[p])) { v = min(v * 10 + (uint64_t)(t[p] - '0'), 0xffffffffull); p++; nd++; }
    if (!nd) return false;
    f(count, (uint32_t)v);
    count++;
    if (p == e) return true;
    if (t[p] != ',') return false;
    p++;
  }
}

// The columns of the link line [p, e) (link_line_parse, version 4).  Returns 0 or the refusal.
__device__ __forceinline__ uint32_t lk_parse_link(const uint8_t *t, uint64_t p, uint64_t e, uint32_t k, LkLink &L)
{
  L.line = p;
  if (e - p < 2 || (t[p] != 'F' && t[p] != 'R') || t[p + 1] != ' ') return MCX_LINKS_BAD_ORIENT;
  uint64_t q = p + 2, nj = 0, cnt = 0;
  uint32_t nd = 0;
  for (; q < e && lk_digit(t[q]); q++, nd++) nj = min(nj * 10 + (uint64_t)(t[q] - '0'), 1ull << 40);
  if (!nd || q >= e || t[q] != ' ') return MCX_LINKS_BAD_NUMBER;
  q++;
  nd = 0;
  for (; q < e && lk_digit(t[q]); q++, nd++) cnt = cnt * 10 + (uint64_t)(t[q] - '0');
  if (q < e && t[q] == ',' && nd) return MCX_LINKS_MULTI_COLOUR;
  if (!nd || q >= e || t[q] != ' ') return MCX_LINKS_BAD_NUMBER;
  q++;
  const uint64_t j0 = q;
  for (; q < e && t[q] != ' '; q++)
    if (!lk_acgt(t[q])) return MCX_LINKS_BAD_JUNCTION;
  const uint64_t jl = q - j0;
  if (nj == 0 || nj > kThMaxJuncs) return MCX_LINKS_NJUNCS_RANGE;
  if (nj != jl) return MCX_LINKS_NJUNCS_LENGTH;
  bool have_seq = false, have_jp = false;
  uint64_t s0 = 0, s1 = 0, p0 = 0, p1 = 0;
  while (q < e) {  // the tags: tokens behind single spaces, the first of a name counts
    q++;
    const uint64_t ts = q;
    while (q < e && t[q] != ' ') q++;
    if (!have_seq && q - ts >= 4 && t[ts] == 's' && t[ts + 1] == 'e' && t[ts + 2] == 'q' && t[ts + 3] == '=') { have_seq = true; s0 = ts + 4; s1 = q; }
    else if (!have_jp && q - ts >= 8 && t[ts] == 'j' && t[ts + 1] == 'u' && t[ts + 2] == 'n' && t[ts + 3] == 'c' && t[ts + 4] == 'p' && t[ts + 5] == 'o' &&
             t[ts + 6] == 's' && t[ts + 7] == '=') { have_jp = true; p0 = ts + 8; p1 = q; }
  }
  if (!have_seq) return MCX_LINKS_NO_SEQ;
  if (!have_jp) return MCX_LINKS_NO_JUNCPOS;
  const uint64_t sl = s1 - s0;
  uint32_t njp = 0, last = 0;
  bool bad_base = false;
  const bool ok = lk_numbers(t, p0, p1, njp, [&](uint32_t i, uint32_t v) {
    last = v;
    if (i < jl && ((uint64_t)k + v >= sl || t[s0 + k + v] != t[j0 + i])) bad_base = true;
  });
  if (!ok || njp != nj) return MCX_LINKS_JUNCPOS_COUNT;
  if (sl != (uint64_t)k + last + 1) return MCX_LINKS_SEQ_LENGTH;
  if (bad_base) return MCX_LINKS_SEQ_BASE;
  L.cnt = cnt;
  L.len = (uint32_t)nj;
  L.junc_at = (uint32_t)(j0 - p); L.seq_at = (uint32_t)(s0 - p); L.seq_len = (uint32_t)sl; L.jp_at = (uint32_t)(p0 - p); L.jp_len = (uint32_t)(p1 - p0);
  return 0;
}

// 2. A thread per line.  kx / lx: the k-mer and link lines before line l.  Link i of the piece gets links[i], nw[i]
// (junction words) and np[i] (juncpos entries); nw[nl] = np[nl] = 0 for the scans.
__global__ __launch_bounds__(256) void k_lk_parse(const uint8_t *text, const uint64_t *lstart, uint64_t nlines, const uint8_t *kflag, const uint8_t *lflag,
                                                  const uint64_t *kx, const uint64_t *lx, uint32_t k, LkLink *links, uint64_t *nw, uint64_t *np,
                                                  unsigned long long *err, unsigned long long *ctr)
{
  unsigned long long c_max = 0;
  for (uint64_t l = cl_first(); l <= nlines; l += cl_stride()) {
    if (l == nlines) { nw[lx[l]] = 0; np[lx[l]] = 0; continue; }
    const uint64_t p = lstart[l], e = lstart[l + 1] - 1;
    if (kflag[l]) {  // ACGT{k} <int>
      bool ok = e - p >= (uint64_t)k + 2 && text[p + k] == ' ';
      for (uint64_t i = 0; ok && i < k; i++) ok = lk_acgt(text[p + i]);
      for (uint64_t i = p + k + 1; ok && i < e; i++) ok = lk_digit(text[i]);
      if (!ok) lk_fail(err, p, MCX_LINKS_BAD_KMER_LINE);
    } else if (lflag[l]) {
      LkLink L;
      L.line = p; L.cnt = 0; L.woff = L.poff = 0; L.key = 0; L.len = 0; L.junc_at = L.seq_at = L.seq_len = L.jp_at = L.jp_len = 0;
      const uint32_t code = kx[l] == 0 ? (uint32_t)MCX_LINKS_LINK_BEFORE_KMER : lk_parse_link(text, p, e, k, L);
      if (code) { lk_fail(err, p, code); L.len = 0; }
      else L.key = ((kx[l] - 1) << 1) | (text[p] == 'R' ? 1ull : 0ull);
      links[lx[l]] = L;
      nw[lx[l]] = (L.len + 31u) / 32u;
      np[lx[l]] = L.len;
      c_max = max(c_max, (unsigned long long)L.len);
    }
  }
  if (c_max) atomicMax(&ctr[kLkMaxLen], c_max);
}
// the junctions of every link into wpool, 2 bits each, the first in the top bits, from a word boundary on; juncpos into ppool
__global__ __launch_bounds__(256) void k_lk_store(const uint8_t *text, LkLink *links, const uint64_t *woff, const uint64_t *poff, uint64_t nl, uint64_t *wpool,
                                                  uint32_t *ppool)
{
  for (uint64_t i = cl_first(); i < nl; i += cl_stride()) {
    LkLink L = links[i];
    L.woff = woff[i];
    L.poff = poff[i];
    links[i].woff = L.woff;
    links[i].poff = L.poff;
    const uint8_t *j = text + L.line + L.junc_at;
    for (uint32_t w = 0; w * 32u < L.len; w++) {
      uint64_t x = 0;
      const uint32_t m = min(32u, L.len - w * 32u);
      for (uint32_t b = 0; b < m; b++) x |= (uint64_t)base_code(j[w * 32u + b]) << (62u - 2u * b);
      wpool[L.woff + w] = x;
    }
    uint32_t cnt;
    uint32_t *dst = ppool + L.poff;
    (void)lk_numbers(text, L.line + L.jp_at, L.line + L.jp_at + L.jp_len, cnt, [&](uint32_t at, uint32_t v) { dst[at] = v; });
  }
}

__device__ __forceinline__ uint64_t lk_word(const LkLink &L, const uint64_t *wpool, uint32_t j)
{
  ThLink v;
  v.base = wpool; v.start = L.woff * 32u; v.len = L.len;
  return th_word(v, j);
}
// 3. word w of the sort key of links[through[i]]: the key, nj junction words, the length
__global__ __launch_bounds__(256) void k_lk_word(const LkLink *links, const uint64_t *wpool, const uint64_t *through, uint32_t w, uint32_t nj, uint64_t *dst,
                                                 uint64_t n)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const LkLink &L = links[through[i]];
    dst[i] = w == 0 ? L.key : w <= nj ? lk_word(L, wpool, w - 1) : (uint64_t)L.len;
  }
}
// 4. head[i] = 1 where sorted item i is another link than item i - 1; head[n] = 0 for the scan
__global__ __launch_bounds__(256) void k_lk_heads(const LkLink *links, const uint64_t *wpool, const uint64_t *perm, uint64_t n, uint8_t *head)
{
  for (uint64_t i = cl_first(); i <= n; i += cl_stride()) {
    uint8_t h = i == n ? 0 : 1;
    if (i > 0 && i < n) {
      const LkLink &a = links[perm[i]], &b = links[perm[i - 1]];
      bool same = a.key == b.key && a.len == b.len;
      for (uint32_t j = 0; same && j * 32u < a.len; j++) same = lk_word(a, wpool, j) == lk_word(b, wpool, j);
      h = same ? 0 : 1;
    }
    head[i] = h;
  }
}
// per run the unique link (the first of the run in file order: the sort is stable) and its summed count; ucnt[nruns] = 0
__global__ __launch_bounds__(256) void k_lk_reduce(const LkLink *links, const uint64_t *perm, const uint64_t *runstart, uint64_t nruns, uint64_t *rep, uint64_t *ucnt)
{
  for (uint64_t u = cl_first(); u <= nruns; u += cl_stride()) {
    if (u == nruns) { ucnt[u] = 0; continue; }
    uint64_t c = 0;
    for (uint64_t i = runstart[u]; i < runstart[u + 1]; i++) c += links[perm[i]].cnt;
    rep[u] = perm[runstart[u]];
    ucnt[u] = c;
  }
}
// lcp[u] = junctions link u shares with link u - 1 of its group (0 for the first); ntl[u] = its tree links; ns[u] = u + 1
__global__ __launch_bounds__(256) void k_lk_lcp(const LkLink *links, const uint64_t *wpool, const uint64_t *rep, uint64_t U, uint32_t *lcp, uint64_t *ntl, uint32_t *ns)
{
  for (uint64_t u = cl_first(); u <= U; u += cl_stride()) {
    if (u == U) { ntl[u] = 0; lcp[u] = 0; continue; }
    const LkLink &b = links[rep[u]];
    uint32_t c = 0;
    if (u > 0) {
      const LkLink &a = links[rep[u - 1]];
      if (a.key == b.key) {
        const uint32_t m = min(a.len, b.len);
        c = m;
        for (uint32_t j = 0; j * 32u < m; j++) {
          const uint64_t x = lk_word(a, wpool, j) ^ lk_word(b, wpool, j);
          if (x) { c = min(m, j * 32u + (uint32_t)__clzll((long long)x) / 2u); break; }
        }
      }
    }
    lcp[u] = c;
    ntl[u] = b.len - c;
    ns[u] = (uint32_t)u + 1u;
  }
}
// 5. One round of pointer jumping, in place: ns[u] moves over links whose lcp is not below lcp[u].  Every value ns[]
// ever holds is valid (everything between u and ns[u] has an lcp of at least lcp[u]), so a stale read only costs a step.
__global__ __launch_bounds__(256) void k_lk_ns(const uint32_t *lcp, uint64_t U, uint32_t *ns, unsigned long long *ctr)
{
  bool more = false;
  for (uint64_t u = cl_first(); u < U; u += cl_stride()) {
    const uint32_t c = lcp[u];
    if (!c) continue;  // (the first of a group is never jumped from: every depth is above its lcp)
    uint32_t p = ns[u];
    for (int step = 0; step < 8 && p < U && lcp[p] >= c; step++) p = __hip_atomic_load(&ns[p], MCX_RLX, MCX_AGENT);
    __hip_atomic_store(&ns[u], p, MCX_RLX, MCX_AGENT);
    more |= p < U && lcp[p] >= c;
  }
  if (__syncthreads_or(more) && threadIdx.x == 0) atomicOr(&ctr[kLkChanged], 1ull);
}

struct LkTree {
  const LkLink *links;
  const uint64_t *rep, *S, *toff;
  const uint32_t *lcp, *ns, *ppool;
  uint64_t U, cutoff;
  uint32_t k, distsize, covgsize, lds_hist;
  unsigned long long *hist;  // or nullptr
  uint64_t *tcnt, *rowlen;   // per tree link, or nullptr (no list wanted)
  uint32_t *tdist;
};
// A thread per link: its tree links from the deepest up, one forward cursor.
__global__ __launch_bounds__(256) void k_lk_tree(LkTree a)
{
  extern __shared__ unsigned long long lk_sh[];
  const uint32_t hn = a.distsize * a.covgsize;
  if (a.hist && a.lds_hist) {
    for (uint32_t i = threadIdx.x; i < hn; i += blockDim.x) lk_sh[i] = 0;
    __syncthreads();
  }
  for (uint64_t u = cl_first(); u < a.U; u += cl_stride()) {
    const LkLink &L = a.links[a.rep[u]];
    const uint32_t lo = a.lcp[u];
    const uint64_t t0 = a.toff[u], Su = a.S[u];
    uint64_t j = u + 1;
    for (uint32_t d = L.len; d > lo; d--) {
      while (j < a.U && a.lcp[j] >= d) j = a.ns[j];
      const uint64_t C = a.S[j] - Su, t = t0 + (d - lo - 1);
      const uint32_t dist = a.ppool[L.poff + d - 1];
      if (a.hist && C && dist < a.distsize) {
        const uint32_t at = dist * a.covgsize + (uint32_t)min(C, (uint64_t)a.covgsize - 1);
        atomicAdd(a.lds_hist ? &lk_sh[at] : &a.hist[at], 1ull);
      }
      if (a.rowlen) {
        const bool keep = C && C >= a.cutoff;
        a.tcnt[t] = C;
        a.tdist[t] = dist;
        a.rowlen[t] = keep ? 2ull + th_digits((uint64_t)a.k + dist + 1) + th_digits(C) : 0ull;
      }
    }
  }
  if (a.hist && a.lds_hist) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < hn; i += blockDim.x)
      if (lk_sh[i]) atomicAdd(&a.hist[i], lk_sh[i]);
  }
}
// the list rows `<k + dist + 1>,<count>`
__global__ __launch_bounds__(256) void k_lk_list(const uint64_t *tcnt, const uint32_t *tdist, const uint64_t *rowlen, const uint64_t *roff, uint64_t T, uint32_t k,
                                                 uint8_t *out)
{
  for (uint64_t t = cl_first(); t < T; t += cl_stride()) {
    if (!rowlen[t]) continue;
    uint8_t *p = out + roff[t];
    const uint64_t a = (uint64_t)k + tdist[t] + 1, c = tcnt[t];
    const uint32_t d1 = th_digits(a), d2 = th_digits(c);
    th_put_num(p, a, d1);
    p[d1] = ',';
    th_put_num(p + d1 + 1, c, d2);
    p[d1 + 1 + d2] = '\n';
  }
}

// 6. wflag[u] = link u is written: maximal in the input (the next link does not extend it) and its count passes
__global__ __launch_bounds__(256) void k_lk_written(const LkLink *links, const uint64_t *rep, const uint64_t *ucnt, const uint32_t *lcp, uint64_t U, uint64_t cutoff,
                                                    uint8_t *wflag)
{
  for (uint64_t u = cl_first(); u <= U; u += cl_stride()) {
    if (u == U) { wflag[u] = 0; continue; }
    const bool maximal = lcp[u + 1] != links[rep[u]].len;  // (lcp[U] = 0, and no link is empty)
    wflag[u] = maximal && ucnt[u] && ucnt[u] >= cutoff;
  }
}
// kbeg / kend [ordinal] = the unique links of that k-mer (both 0 where it has none: the arrays come zeroed)
__global__ __launch_bounds__(256) void k_lk_groups(const LkLink *links, const uint64_t *rep, uint64_t U, uint64_t *kbeg, uint64_t *kend)
{
  for (uint64_t u = cl_first(); u < U; u += cl_stride()) {
    const uint64_t o = links[rep[u]].key >> 1;
    if (u == 0 || (links[rep[u - 1]].key >> 1) != o) kbeg[o] = u;
    if (u + 1 == U || (links[rep[u + 1]].key >> 1) != o) kend[o] = u + 1;
  }
}
__global__ __launch_bounds__(256) void k_lk_stats(const LkLink *links, const uint64_t *rep, const uint8_t *wflag, const uint64_t *wx, const uint64_t *kbeg, uint64_t U,
                                                  unsigned long long *ctr)
{
  unsigned long long c_k = 0, c_l = 0, c_b = 0;
  for (uint64_t u = cl_first(); u < U; u += cl_stride()) {
    if (!wflag[u]) continue;
    const LkLink &L = links[rep[u]];
    c_l++;
    c_b += (L.len + 3u) / 4u;
    c_k += wx[u] == wx[kbeg[L.key >> 1]];
  }
  block_add(&ctr[kLkKmersWithLinks], c_k);
  block_add(&ctr[kLkLinks], c_l);
  block_add(&ctr[kLkBytes], c_b);
}

struct LkText {
  const uint8_t *text;
  const LkLink *links;
  const uint64_t *rep, *ucnt, *wx, *kbeg, *kend, *kline, *lstart;
  const uint8_t *wflag;
  uint64_t U;
  uint32_t k;
};
// 7. Eight lanes per link.  EMIT = false: len[u] = the bytes of link u's line (0 when it is not written), with the
// `<kmer> <nlinks>` line before it when it is the first written link of its k-mer.  EMIT = true: the lines at out + off[u].
template <bool EMIT> __global__ __launch_bounds__(256) void k_lk_text(LkText a, uint64_t *len, const uint64_t *off, uint8_t *out)
{
  const uint32_t sub = threadIdx.x & 7u;
  const uint64_t per_block = blockDim.x >> 3;
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < a.U; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t u = base + (threadIdx.x >> 3);
    if (u >= a.U) continue;
    if (!a.wflag[u]) { if (!EMIT && sub == 0) len[u] = 0; continue; }
    const LkLink L = a.links[a.rep[u]];
    const uint64_t o = L.key >> 1, cnt = a.ucnt[u];
    uint8_t *dst = EMIT ? out + off[u] : nullptr;
    uint64_t at = 0;
    if (a.wx[u] == a.wx[a.kbeg[o]]) {
      const uint64_t nl = a.wx[a.kend[o]] - a.wx[a.kbeg[o]];
      const uint32_t d = th_digits(nl);
      if (EMIT) {
        const uint8_t *km = a.text + a.lstart[a.kline[o]];
        for (uint32_t j = sub; j < a.k; j += 8) dst[j] = km[j];
        if (sub == 0) { dst[a.k] = ' '; th_put_num(dst + a.k + 1, nl, d); dst[a.k + 1 + d] = '\n'; }
      }
      at += (uint64_t)a.k + 2 + d;
    }
    const uint32_t d1 = th_digits(L.len), d2 = th_digits(cnt);
    if (EMIT) {
      uint8_t *p = dst + at;
      const uint8_t *src = a.text + L.line;
      if (sub == 0) {
        p[0] = (L.key & 1ull) ? 'R' : 'F'; p[1] = ' ';
        th_put_num(p + 2, L.len, d1); p[2 + d1] = ' ';
        th_put_num(p + 3 + d1, cnt, d2); p[3 + d1 + d2] = ' ';
      }
      p += 4 + d1 + d2;
      for (uint32_t j = sub; j < L.len; j += 8) p[j] = src[L.junc_at + j];
      p += L.len;
      if (sub == 0) memcpy(p, " seq=", 5);
      p += 5;
      for (uint32_t j = sub; j < L.seq_len; j += 8) p[j] = src[L.seq_at + j];
      p += L.seq_len;
      if (sub == 1) memcpy(p, " juncpos=", 9);
      p += 9;
      for (uint32_t j = sub; j < L.jp_len; j += 8) p[j] = src[L.jp_at + j];
      if (sub == 0) p[L.jp_len] = '\n';
    }
    at += 4ull + d1 + d2 + L.len + 5ull + L.seq_len + 9ull + L.jp_len + 1ull;
    if (!EMIT && sub == 0) len[u] = at;
  }
}

}  // namespace mcx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mcx_links {
  int k = 0, device = 0, cus = 0;
  uint32_t grid = 0;
  uint64_t out_chunk = 64ull << 20;
  hipStream_t stream = nullptr;
  unsigned long long *d_ctr = nullptr, *d_err = nullptr, *d_hist = nullptr;
  uint32_t distsize = 0, covgsize = 0;
  void *h_buf = nullptr;     // mcx_links_buffer
  uint8_t *h_out = nullptr;  // text delivery
  size_t h_out_cap = 0;
  int err_code = 0;
  uint64_t err_off = 0;
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // mcx_links_phases
  mcx_links_stats st{};
};

static unsigned links_grid(const mcx_links *l, uint64_t items)
{
  const uint64_t cap = l->grid ? l->grid : (uint64_t)l->cus * 8;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, cap));
}

extern "C" void mcx_links_destroy(mcx_links *l)
{
  if (!l) return;
  (void)hipSetDevice(l->device);
  if (l->stream) (void)hipStreamSynchronize(l->stream);
  if (l->d_ctr) (void)hipFree(l->d_ctr);
  if (l->d_err) (void)hipFree(l->d_err);
  if (l->d_hist) (void)hipFree(l->d_hist);
  if (l->h_buf) (void)hipHostFree(l->h_buf);
  if (l->h_out) (void)hipHostFree(l->h_out);
  if (l->stream) (void)hipStreamDestroy(l->stream);
  delete l;
}

extern "C" int mcx_links_create(mcx_links **out, int kmer_size, int device)
{
  if (!out) return fail(MCX_ERR_ARG, "null argument");
  *out = nullptr;
  if (kmer_size < 3 || !(kmer_size & 1)) return fail(MCX_ERR_ARG, "kmer size must be odd and at least 3 (got %d)", kmer_size);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return fail(MCX_ERR_NODEVICE, "no HIP device found"); }
  if (device < 0 || device >= ndev) return fail(MCX_ERR_NODEVICE, "no HIP device %d (%d found)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  mcx_links *l = new mcx_links();
  ScopeExit drop([&] { mcx_links_destroy(l); });
  l->k = kmer_size; l->device = device;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  l->cus = std::max(1, prop.multiProcessorCount);
  HIP_TRY(hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc((void **)&l->d_ctr, kLkNumCounters * sizeof(unsigned long long)));
  HIP_TRY(hipMalloc((void **)&l->d_err, sizeof(unsigned long long)));
  drop.dismiss();
  *out = l;
  return MCX_OK;
}

extern "C" int mcx_links_configure(mcx_links *l, const char *key, uint64_t value)
{
  if (!l || !key) return fail(MCX_ERR_ARG, "null argument");
  if (!strcmp(key, "grid")) { l->grid = (uint32_t)std::min<uint64_t>(value, 1u << 20); return MCX_OK; }
  if (!strcmp(key, "out_chunk")) { l->out_chunk = value ? value : (64ull << 20); return MCX_OK; }
  return fail(MCX_ERR_ARG, "unknown links configuration key: %s", key);
}

extern "C" int mcx_links_get_stats(const mcx_links *l, mcx_links_stats *stats)
{
  if (!l || !stats) return fail(MCX_ERR_ARG, "null argument");
  *stats = l->st;
  return MCX_OK;
}

extern "C" int mcx_links_phases(const mcx_links *l, double *ms)
{
  if (!l || !ms) return fail(MCX_ERR_ARG, "null argument");
  for (int i = 0; i < 8; i++) ms[i] = l->ms[i];
  return MCX_OK;
}

extern "C" int mcx_links_error(const mcx_links *l, int *code, uint64_t *byte_offset)
{
  if (!l) return fail(MCX_ERR_ARG, "null argument");
  if (code) *code = l->err_code;
  if (byte_offset) *byte_offset = l->err_off;
  return MCX_OK;
}

extern "C" int mcx_links_buffer(mcx_links *l, size_t bytes, void **ptr)
{
  if (!l || !ptr || !bytes) return fail(MCX_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(l->device));
  if (l->h_buf) { (void)hipHostFree(l->h_buf); l->h_buf = nullptr; }
  HIP_TRY(hipHostMalloc(&l->h_buf, bytes, hipHostMallocDefault));
  *ptr = l->h_buf;
  return MCX_OK;
}

extern "C" int mcx_links_hist(mcx_links *l, uint64_t *out)
{
  if (!l || !out) return fail(MCX_ERR_ARG, "null argument");
  if (!l->d_hist) return fail(MCX_ERR_ARG, "links: no histogram was asked for");
  HIP_TRY(hipSetDevice(l->device));
  HIP_TRY(hipMemcpy(out, l->d_hist, (size_t)l->distsize * l->covgsize * 8, hipMemcpyDeviceToHost));
  return MCX_OK;
}

// `total` bytes of finished text on the device to a sink, `out_chunk` bytes at a time through the pinned buffer *h_out
// (grown to a chunk when it is smaller); `links` and `pjoin` deliver their texts through this
static int text_deliver(hipStream_t st, uint64_t out_chunk, uint8_t **h_out, size_t *h_out_cap, const uint8_t *d_text, uint64_t total, mcx_sink_fn sink, void *ctx,
                        const char *who, const char *what)
{
  const uint64_t chunk = std::min<uint64_t>(std::max<uint64_t>(out_chunk, 1), std::max<uint64_t>(total, 1));
  if (chunk > *h_out_cap) {
    if (*h_out) (void)hipHostFree(*h_out);
    *h_out = nullptr; *h_out_cap = 0;
    HIP_TRY(hipHostMalloc((void **)h_out, chunk, hipHostMallocDefault));
    *h_out_cap = chunk;
  }
  for (uint64_t c0 = 0; c0 < total; c0 += chunk) {
    const uint64_t nb = std::min(total, c0 + chunk) - c0;
    HIP_TRY(hipMemcpyAsync(*h_out, d_text + c0, nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (sink(ctx, *h_out, (size_t)nb) != 0) return fail(MCX_ERR_SINK, "%s: the sink refused the %s", who, what);
  }
  return MCX_OK;
}
static int links_deliver(mcx_links *l, const uint8_t *d_text, uint64_t total, mcx_sink_fn sink, void *ctx, const char *what)
{
  return text_deliver(l->stream, l->out_chunk, &l->h_out, &l->h_out_cap, d_text, total, sink, ctx, "links", what);
}

#define LK_LAUNCH(NAME, ITEMS, ...)                                                                       \
  do {                                                                                                    \
    hipLaunchKernelGGL(NAME, dim3(links_grid(l, ITEMS)), dim3(256), 0, st, __VA_ARGS__);                  \
    HIP_TRY(hipGetLastError());                                                                           \
  } while (0)

extern "C" int mcx_links_add_text(mcx_links *l, const void *text, uint64_t nbytes, const mcx_links_params *p, mcx_sink_fn ctp_sink, void *ctp_ctx,
                                  mcx_sink_fn list_sink, void *list_ctx)
{
  if (!l || !p) return fail(MCX_ERR_ARG, "null argument");
  if (p->flags & ~(uint32_t)(MCX_LINKS_CLEAN | MCX_LINKS_HIST)) return fail(MCX_ERR_ARG, "unknown links flags: %u", p->flags);
  const bool want_hist = p->flags & MCX_LINKS_HIST;
  if (want_hist && (!p->distsize || !p->covgsize || (uint64_t)p->distsize * p->covgsize > (1u << 26)))
    return fail(MCX_ERR_ARG, "links: bad histogram size %u x %u", p->distsize, p->covgsize);
  if (want_hist && l->d_hist && (l->distsize != p->distsize || l->covgsize != p->covgsize))
    return fail(MCX_ERR_ARG, "links: the histogram of this handle is %u x %u", l->distsize, l->covgsize);
  if (!nbytes) return MCX_OK;
  if (!text) return fail(MCX_ERR_ARG, "null text");
  if (nbytes >= (1ull << 31)) return fail(MCX_ERR_ARG, "links: a piece of %llu bytes (2 GB at the most)", (unsigned long long)nbytes);
  if (((const uint8_t *)text)[nbytes - 1] != '\n') return fail(MCX_ERR_ARG, "links: the text does not end with a newline");
  HIP_TRY(hipSetDevice(l->device));
  hipStream_t st = l->stream;
  double t_ph = now_s();
  auto phase = [&](int i) { (void)hipStreamSynchronize(st); const double t = now_s(); l->ms[i] += (t - t_ph) * 1e3; t_ph = t; };
  const uint64_t cutoff = (p->flags & MCX_LINKS_CLEAN) ? p->cutoff : 0;
  const uint32_t k = (uint32_t)l->k;
  int rc;
  if (want_hist && !l->d_hist) {
    HIP_TRY(hipMalloc((void **)&l->d_hist, (size_t)p->distsize * p->covgsize * 8));
    l->distsize = p->distsize; l->covgsize = p->covgsize;
    HIP_TRY(hipMemsetAsync(l->d_hist, 0, (size_t)p->distsize * p->covgsize * 8, st));
  }
  l->err_code = 0; l->err_off = 0;

  // 1. lines
  uint64_t n = nbytes;
  DevBuf<uint8_t> d_text, d_flag, d_kflag, d_lflag;
  DevBuf<uint64_t> d_lidx, d_lstart, d_kx, d_lx, d_kline;
  HIP_TRY(d_text.alloc(n + 16));
  HIP_TRY(d_flag.alloc(n + 1));
  HIP_TRY(d_lidx.alloc(n + 1));
  HIP_TRY(hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_text.p + n, 0, 16, st));
  HIP_TRY(hipMemsetAsync(l->d_ctr, 0, kLkNumCounters * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(l->d_err, 0xff, sizeof(unsigned long long), st));
  phase(0);
  LK_LAUNCH(k_lk_mark, n + 1, (const uint8_t *)d_text.p, n, d_flag.p);
  uint64_t nlines = 0;
  if ((rc = scan_total(st, (const uint8_t *)d_flag.p, d_lidx.p, n + 1, &nlines)) != MCX_OK) return rc;
  HIP_TRY(d_lstart.alloc(nlines + 1));
  HIP_TRY(d_kflag.alloc(nlines + 1));
  HIP_TRY(d_lflag.alloc(nlines + 1));
  HIP_TRY(d_kx.alloc(nlines + 1));
  HIP_TRY(d_lx.alloc(nlines + 1));
  LK_LAUNCH(k_lk_starts, n + 1, (const uint8_t *)d_flag.p, (const uint64_t *)d_lidx.p, n, d_lstart.p);
  LK_LAUNCH(k_lk_class, nlines + 1, (const uint8_t *)d_text.p, (const uint64_t *)d_lstart.p, nlines, d_kflag.p, d_lflag.p);
  uint64_t nk = 0, nl = 0;
  if ((rc = scan_total(st, (const uint8_t *)d_kflag.p, d_kx.p, nlines + 1, &nk)) != MCX_OK) return rc;
  if ((rc = device_scan(st, (const uint8_t *)d_lflag.p, d_lx.p, nlines + 1)) != MCX_OK) return rc;
  d_flag.release();
  d_lidx.release();
  HIP_TRY(d_kline.alloc(nk + 1));
  LK_LAUNCH(k_lk_klines, nlines, (const uint8_t *)d_kflag.p, (const uint64_t *)d_kx.p, nlines, d_kline.p);
  if (p->max_kmers && nk > p->max_kmers) {  // the piece ends where k-mer number max_kmers begins
    HIP_TRY(hipMemcpyAsync(&nlines, d_kline.p + p->max_kmers, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    nk = p->max_kmers;
  }
  HIP_TRY(hipMemcpyAsync(&nl, d_lx.p + nlines, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  phase(1);

  // 2. parse
  DevBuf<LkLink> d_links;
  DevBuf<uint64_t> d_nw, d_np, d_woff, d_poff, d_wpool;
  DevBuf<uint32_t> d_ppool;
  HIP_TRY(d_links.alloc(nl + 1));
  HIP_TRY(d_nw.alloc(nl + 1));
  HIP_TRY(d_np.alloc(nl + 1));
  HIP_TRY(d_woff.alloc(nl + 1));
  HIP_TRY(d_poff.alloc(nl + 1));
  LK_LAUNCH(k_lk_parse, nlines + 1, (const uint8_t *)d_text.p, (const uint64_t *)d_lstart.p, nlines, (const uint8_t *)d_kflag.p, (const uint8_t *)d_lflag.p,
            (const uint64_t *)d_kx.p, (const uint64_t *)d_lx.p, k, d_links.p, d_nw.p, d_np.p, l->d_err, l->d_ctr);
  unsigned long long h_err = 0, h_ctr[kLkNumCounters];
  HIP_TRY(hipMemcpyAsync(&h_err, l->d_err, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_ctr, l->d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h_err != kLkNoErr) {
    l->err_code = (int)(h_err & 0xffu);
    l->err_off = h_err >> 8;
    return fail(MCX_ERR_INVAL, "links: bad line at byte %llu of the piece (refusal %d)", (unsigned long long)l->err_off, l->err_code);
  }
  l->st.kmers_read += nk;
  l->st.links_in += nl;
  if (!nl) { phase(2); return MCX_OK; }
  uint64_t nwords = 0, npos = 0;
  if ((rc = scan_total(st, (const uint64_t *)d_nw.p, d_woff.p, nl + 1, &nwords)) != MCX_OK) return rc;
  if ((rc = scan_total(st, (const uint64_t *)d_np.p, d_poff.p, nl + 1, &npos)) != MCX_OK) return rc;
  HIP_TRY(d_wpool.alloc(nwords + 2));
  HIP_TRY(d_ppool.alloc(npos + 1));
  HIP_TRY(hipMemsetAsync(d_wpool.p + nwords, 0, 16, st));
  LK_LAUNCH(k_lk_store, nl, (const uint8_t *)d_text.p, d_links.p, (const uint64_t *)d_woff.p, (const uint64_t *)d_poff.p, nl, d_wpool.p, d_ppool.p);
  d_nw.release(); d_np.release(); d_woff.release(); d_poff.release();
  d_kflag.release(); d_lflag.release(); d_kx.release(); d_lx.release();
  phase(2);

  // 3. sort
  const uint32_t nj = ((uint32_t)h_ctr[kLkMaxLen] + 31u) / 32u;
  size_t tmp_bytes = 0;
  if ((rc = sort_perm_scratch(st, nl, &tmp_bytes)) != MCX_OK) return rc;
  DevBuf<uint64_t> d_p0, d_p1, d_k0, d_k1;
  DevBuf<uint8_t> d_tmp, d_head;
  HIP_TRY(d_p0.alloc(nl + 1));
  HIP_TRY(d_p1.alloc(nl + 1));
  HIP_TRY(d_k0.alloc(nl + 1));
  HIP_TRY(d_k1.alloc(nl + 1));
  HIP_TRY(d_tmp.alloc(tmp_bytes ? tmp_bytes : 16));
  HIP_TRY(d_head.alloc(nl + 1));
  HIP_TRY(hipMemsetAsync(d_head.p, 1, nl, st));  // iota: the exclusive sum of ones
  if ((rc = device_scan(st, (const uint8_t *)d_head.p, d_p0.p, nl)) != MCX_OK) return rc;
  auto word = [&](int w, bool, const uint64_t *through, uint64_t *dst, const uint64_t **) -> int {
    LK_LAUNCH(k_lk_word, nl, (const LkLink *)d_links.p, (const uint64_t *)d_wpool.p, through, (uint32_t)w, nj, dst, nl);
    return MCX_OK;
  };
  uint64_t *const keys[2] = {d_k0.p, d_k1.p}, *const perms[2] = {d_p0.p, d_p1.p}, *perm = nullptr;
  if ((rc = sort_perm_by_words(st, nl, (int)nj + 2, 33, keys, perms, d_tmp.p, tmp_bytes, nullptr, word, &perm)) != MCX_OK) return rc;
  phase(3);

  // 4. equal links, lcp
  uint64_t *runstart = perm == d_p0.p ? d_p1.p : d_p0.p, *ex = d_k0.p, U = 0;
  LK_LAUNCH(k_lk_heads, nl + 1, (const LkLink *)d_links.p, (const uint64_t *)d_wpool.p, (const uint64_t *)perm, nl, d_head.p);
  if ((rc = scan_total(st, (const uint8_t *)d_head.p, ex, nl + 1, &U)) != MCX_OK) return rc;
  LK_LAUNCH(k_th_runs, nl + 1, (const uint8_t *)d_head.p, (const uint64_t *)ex, nl, runstart);
  DevBuf<uint64_t> d_rep, d_ucnt, d_S, d_ntl, d_toff;
  DevBuf<uint32_t> d_lcp, d_ns;
  HIP_TRY(d_rep.alloc(U + 1));
  HIP_TRY(d_ucnt.alloc(U + 1));
  HIP_TRY(d_S.alloc(U + 1));
  HIP_TRY(d_ntl.alloc(U + 1));
  HIP_TRY(d_toff.alloc(U + 1));
  HIP_TRY(d_lcp.alloc(U + 1));
  HIP_TRY(d_ns.alloc(U + 1));
  LK_LAUNCH(k_lk_reduce, U + 1, (const LkLink *)d_links.p, (const uint64_t *)perm, (const uint64_t *)runstart, U, d_rep.p, d_ucnt.p);
  LK_LAUNCH(k_lk_lcp, U + 1, (const LkLink *)d_links.p, (const uint64_t *)d_wpool.p, (const uint64_t *)d_rep.p, U, d_lcp.p, d_ntl.p, d_ns.p);
  if ((rc = device_scan(st, (const uint64_t *)d_ucnt.p, d_S.p, U + 1)) != MCX_OK) return rc;
  uint64_t T = 0;
  if ((rc = scan_total(st, (const uint64_t *)d_ntl.p, d_toff.p, U + 1, &T)) != MCX_OK) return rc;
  d_p0.release(); d_p1.release(); d_k0.release(); d_k1.release(); d_tmp.release(); d_head.release();
  l->st.tree_links += T;
  phase(4);

  // 5. tree links: histogram and list
  if (want_hist || list_sink) {
    for (int round = 0;; round++) {
      if (round > 4096) return fail(MCX_ERR_HIP, "links: the next-smaller pointers did not settle");
      HIP_TRY(hipMemsetAsync(l->d_ctr + kLkChanged, 0, 8, st));
      LK_LAUNCH(k_lk_ns, U, (const uint32_t *)d_lcp.p, U, d_ns.p, l->d_ctr);
      unsigned long long more = 0;
      HIP_TRY(hipMemcpyAsync(&more, l->d_ctr + kLkChanged, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (!more) break;
    }
    DevBuf<uint64_t> d_tcnt, d_rowlen, d_roff;
    DevBuf<uint32_t> d_tdist;
    DevBuf<uint8_t> d_rows;
    if (list_sink) {
      HIP_TRY(d_tcnt.alloc(T + 1));
      HIP_TRY(d_rowlen.alloc(T + 1));
      HIP_TRY(d_roff.alloc(T + 1));
      HIP_TRY(d_tdist.alloc(T + 1));
      HIP_TRY(hipMemsetAsync(d_rowlen.p + T, 0, 8, st));
    }
    LkTree a;
    a.links = d_links.p; a.rep = d_rep.p; a.S = d_S.p; a.toff = d_toff.p; a.lcp = d_lcp.p; a.ns = d_ns.p; a.ppool = d_ppool.p;
    a.U = U; a.cutoff = cutoff; a.k = k;
    a.distsize = want_hist ? p->distsize : 0; a.covgsize = want_hist ? p->covgsize : 0;
    a.hist = want_hist ? l->d_hist : nullptr;
    const size_t hbytes = (size_t)a.distsize * a.covgsize * 8;
    a.lds_hist = want_hist && hbytes <= (32u << 10);
    a.tcnt = d_tcnt.p; a.rowlen = d_rowlen.p; a.tdist = d_tdist.p;
    hipLaunchKernelGGL(k_lk_tree, dim3(links_grid(l, U)), dim3(256), a.lds_hist ? hbytes : 0, st, a);
    HIP_TRY(hipGetLastError());
    if (list_sink) {
      uint64_t rbytes = 0;
      if ((rc = scan_total(st, (const uint64_t *)d_rowlen.p, d_roff.p, T + 1, &rbytes)) != MCX_OK) return rc;
      if (rbytes) {
        HIP_TRY(d_rows.alloc(rbytes));
        LK_LAUNCH(k_lk_list, T, (const uint64_t *)d_tcnt.p, (const uint32_t *)d_tdist.p, (const uint64_t *)d_rowlen.p, (const uint64_t *)d_roff.p, T, k, d_rows.p);
        if ((rc = links_deliver(l, d_rows.p, rbytes, list_sink, list_ctx, "list rows")) != MCX_OK) return rc;
      }
    }
  }
  phase(5);

  // 6. what is written, the totals
  DevBuf<uint8_t> d_wflag;
  DevBuf<uint64_t> d_wx, d_kbeg, d_kend;
  HIP_TRY(d_wflag.alloc(U + 1));
  HIP_TRY(d_wx.alloc(U + 1));
  HIP_TRY(d_kbeg.alloc(nk + 1));
  HIP_TRY(d_kend.alloc(nk + 1));
  HIP_TRY(hipMemsetAsync(d_kbeg.p, 0, (nk + 1) * 8, st));
  HIP_TRY(hipMemsetAsync(d_kend.p, 0, (nk + 1) * 8, st));
  LK_LAUNCH(k_lk_written, U + 1, (const LkLink *)d_links.p, (const uint64_t *)d_rep.p, (const uint64_t *)d_ucnt.p, (const uint32_t *)d_lcp.p, U, cutoff, d_wflag.p);
  if ((rc = device_scan(st, (const uint8_t *)d_wflag.p, d_wx.p, U + 1)) != MCX_OK) return rc;
  LK_LAUNCH(k_lk_groups, U, (const LkLink *)d_links.p, (const uint64_t *)d_rep.p, U, d_kbeg.p, d_kend.p);
  LK_LAUNCH(k_lk_stats, U, (const LkLink *)d_links.p, (const uint64_t *)d_rep.p, (const uint8_t *)d_wflag.p, (const uint64_t *)d_wx.p, (const uint64_t *)d_kbeg.p, U,
            l->d_ctr);
  HIP_TRY(hipMemcpyAsync(h_ctr, l->d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  l->st.kmers_with_links += h_ctr[kLkKmersWithLinks];
  l->st.links += h_ctr[kLkLinks];
  l->st.link_bytes += h_ctr[kLkBytes];
  phase(6);

  // 7. the .ctp text
  if (ctp_sink && h_ctr[kLkLinks]) {
    DevBuf<uint64_t> d_len, d_off;
    DevBuf<uint8_t> d_out;
    HIP_TRY(d_len.alloc(U + 1));
    HIP_TRY(d_off.alloc(U + 1));
    HIP_TRY(hipMemsetAsync(d_len.p + U, 0, 8, st));
    LkText a;
    a.text = d_text.p; a.links = d_links.p; a.rep = d_rep.p; a.ucnt = d_ucnt.p; a.wx = d_wx.p; a.kbeg = d_kbeg.p; a.kend = d_kend.p; a.kline = d_kline.p;
    a.lstart = d_lstart.p; a.wflag = d_wflag.p; a.U = U; a.k = k;
    LK_LAUNCH(k_lk_text<false>, U * 8, a, d_len.p, (const uint64_t *)nullptr, (uint8_t *)nullptr);
    uint64_t total = 0;
    if ((rc = scan_total(st, (const uint64_t *)d_len.p, d_off.p, U + 1, &total)) != MCX_OK) return rc;
    HIP_TRY(d_out.alloc(total + 1));
    LK_LAUNCH(k_lk_text<true>, U * 8, a, (uint64_t *)nullptr, (const uint64_t *)d_off.p, d_out.p);
    if ((rc = links_deliver(l, d_out.p, total, ctp_sink, ctp_ctx, ".ctp text")) != MCX_OK) return rc;
  }
  phase(7);
  return MCX_OK;
}
