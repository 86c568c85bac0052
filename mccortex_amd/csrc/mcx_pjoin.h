// mcx_pjoin.h -- `pjoin` on the device (included by mcx_api.hip behind mcx_links.h: it uses that file's line marking,
// its number lists and its text delivery).
//
// ctx_pjoin.c without its hash table: link files are merged by a sort of (k-mer, orientation, junction string) and a
// segmented reduce of per-colour counts.  No graph handle; the k-mer of a `<kmer> <n>` line is taken as written, packed
// 2 bits a base into W = ceil(2k / 64) words whose order is text order.  One handle holds a STORE across pieces and files:
//   records  PjRec: kw = (k-mer << 1 | orientation) as a number of W words (kw[0] most significant, as ThLink keeps it),
//            the junction length, an offset into the junction word pool (the layout k_lk_store writes: 2 bits a
//            junction, the first in the top bits, every link from a word boundary on) and offset, first colour and extent
//            into the count pool
//   counts   one byte per colour of the into-range [c0, c0 + cn) of the line's file only (sparse: N one-colour files cost
//            one byte a line, not N), already min(255, .) per line and colour
// The passes ("pjoin's device passes"), all grid-stride loops:
//   add      k_lk_mark, k_lk_starts, k_lk_class, k_lk_klines (mcx_links.h), then k_pj_parse, a thread per line: a k-mer
//            line to its key words and its <n> against the link lines that follow; a link line to orientation, njuncs, a
//            count column of exactly src_ncols numbers and the junctions (tags are skipped unparsed); a line whose mapped
//            counts are all zero is flagged.  A scan of the flags compacts those away, k_pj_store writes records, junction
//            words and counts at scanned offsets.  A refused piece (the smallest byte offset wins, lk_fail) stores nothing.
//   finish   sort_perm_by_words over (kw, junction words zero padded to the longest link, length); k_pj_heads, a scan,
//            k_th_runs; k_pj_reduce: per run the saturating per-colour sums into a dense U x out_ncols byte matrix;
//            k_pj_groups: the first link of every k-mer, a scan, k_th_runs again: links per k-mer; k_pj_totals; k_pj_text:
//            length pass, 64-bit scan, emit pass, delivered in "out_chunk" pieces (text_deliver)
//   compact  the same sort and runs; k_pj_extent and k_pj_compact write the unique links in the store's own layout.  Every
//            step is min(255, .), so compaction at any point cannot change the answer.
// A run of equal links is reduced by one thread, and two links are compared word by word by one thread (the limits
// `thread` records for k_th_reduce and k_th_heads).
#pragma once
#include "mcx_links.h"

namespace mcx {

enum : uint32_t { kPjKmerLines = 0, kPjLinkLines, kPjBadN, kPjMaxLen, kPjKmers, kPjBytes, kPjNumCounters };

// a parsed link line of the piece (offsets relative to `line`, a byte offset in the piece)
struct PjLine {
  uint64_t line, ord /* of its k-mer line */;
  uint32_t len, junc_at, cnt_at, cnt_len, orient;
};
struct PjRec {
  uint64_t kw[4], woff, coff;
  uint32_t len, c0, cn, pad;
};
// the filter by source colour: the into colours of source colour f are into[start[f] .. start[f + 1])
struct PjFilter {
  const uint32_t *start, *into;
  uint32_t src_ncols, lo /* the smallest into colour */, cn /* the extent of the into colours */;
};

// A thread per line.  kx / lx: the k-mer and link lines before line l.  k-mer `ord` gets kw[4 * ord ..]; link i of the
// piece gets lines[i], keep[i] (it has a non-zero mapped count) and nw[i] (its junction words when it is kept);
// keep[nl] = nw[nl] = 0 for the scans.
__global__ __launch_bounds__(256) void k_pj_parse(const uint8_t *text, const uint64_t *lstart, uint64_t nlines, const uint8_t *kflag, const uint8_t *lflag,
                                                  const uint64_t *kx, const uint64_t *lx, const uint64_t *kline, uint64_t nk, uint32_t k, uint32_t W, PjFilter f,
                                                  PjLine *lines, uint8_t *keep, uint64_t *nw, uint64_t *kw, unsigned long long *err, unsigned long long *ctr)
{
  unsigned long long c_k = 0, c_l = 0, c_bad = 0, c_max = 0;
  for (uint64_t l = cl_first(); l <= nlines; l += cl_stride()) {
    if (l == nlines) { keep[lx[l]] = 0; nw[lx[l]] = 0; continue; }
    const uint64_t p = lstart[l], e = lstart[l + 1] - 1;
    if (kflag[l]) {  // ACGT{k} <int>
      bool ok = e - p >= (uint64_t)k + 2 && text[p + k] == ' ';
      for (uint64_t i = 0; ok && i < k; i++) ok = lk_acgt(text[p + i]);
      for (uint64_t i = p + k + 1; ok && i < e; i++) ok = lk_digit(text[i]);
      if (!ok) { lk_fail(err, p, MCX_LINKS_BAD_KMER_LINE); continue; }
      uint64_t x[4] = {0, 0, 0, 0}, n = 0;
      for (uint32_t i = 0; i < k; i++) {
        for (uint32_t w = 0; w + 1 < W; w++) x[w] = (x[w] << 2) | (x[w + 1] >> 62);
        x[W - 1] = (x[W - 1] << 2) | base_code(text[p + i]);
      }
      for (uint32_t w = 0; w < W; w++) x[w] = (x[w] << 1) | (w + 1 < W ? x[w + 1] >> 63 : 0ull);
      const uint64_t ord = kx[l];
      for (uint32_t w = 0; w < 4; w++) kw[4 * ord + w] = x[w];
      for (uint64_t i = p + k + 1; i < e; i++) n = min(n * 10 + (uint64_t)(text[i] - '0'), 1ull << 40);
      const uint64_t next = ord + 1 < nk ? kline[ord + 1] : nlines;
      c_k++;
      c_bad += n != lx[next] - lx[l];
    } else if (lflag[l]) {
      PjLine L;
      L.line = p; L.ord = 0; L.len = 0; L.junc_at = L.cnt_at = L.cnt_len = L.orient = 0;
      uint32_t code = 0;
      bool nonzero = false;
      if (kx[l] == 0) code = MCX_LINKS_LINK_BEFORE_KMER;
      else if (e - p < 2 || (text[p] != 'F' && text[p] != 'R') || text[p + 1] != ' ') code = MCX_LINKS_BAD_ORIENT;
      else {
        uint64_t q = p + 2, nj = 0;
        uint32_t nd = 0;
        for (; q < e && lk_digit(text[q]); q++, nd++) nj = min(nj * 10 + (uint64_t)(text[q] - '0'), 1ull << 40);
        if (!nd || q >= e || text[q] != ' ') code = MCX_LINKS_BAD_NUMBER;
        else {
          const uint64_t c0 = ++q;
          while (q < e && text[q] != ' ') q++;
          uint32_t ncnt = 0;
          const bool ok = lk_numbers(text, c0, q, ncnt, [&](uint32_t i, uint32_t v) {
            if (v && i < f.src_ncols && f.start[i + 1] > f.start[i]) nonzero = true;
          });
          if (!ok || q >= e) code = MCX_LINKS_BAD_NUMBER;
          else if (ncnt != f.src_ncols) code = MCX_LINKS_COUNT_COLUMNS;
          else {
            const uint64_t j0 = ++q;
            for (; q < e && text[q] != ' '; q++)
              if (!lk_acgt(text[q])) { code = MCX_LINKS_BAD_JUNCTION; break; }
            if (!code) {
              if (nj == 0 || nj > kThMaxJuncs) code = MCX_LINKS_NJUNCS_RANGE;
              else if (nj != q - j0) code = MCX_LINKS_NJUNCS_LENGTH;
              else {
                L.ord = kx[l] - 1; L.len = (uint32_t)nj; L.junc_at = (uint32_t)(j0 - p); L.cnt_at = (uint32_t)(c0 - p); L.cnt_len = (uint32_t)(j0 - 1 - c0);
                L.orient = text[p] == 'R';
              }
            }
          }
        }
      }
      if (code) { lk_fail(err, p, code); L.len = 0; nonzero = false; }
      lines[lx[l]] = L;
      keep[lx[l]] = nonzero;
      nw[lx[l]] = nonzero ? (L.len + 31u) / 32u : 0u;
      c_l++;
      if (nonzero) c_max = max(c_max, (unsigned long long)L.len);
    }
  }
  block_add(&ctr[kPjKmerLines], c_k);
  block_add(&ctr[kPjLinkLines], c_l);
  block_add(&ctr[kPjBadN], c_bad);
  if (c_max) atomicMax(&ctr[kPjMaxLen], c_max);
}

// the kept links of the piece into the store: record rec0 + keepx[i], its junction words from word0 + woff[i] on, its
// f.cn count bytes from cnt0 + keepx[i] * f.cn on
__global__ __launch_bounds__(256) void k_pj_store(const uint8_t *text, const PjLine *lines, const uint8_t *keep, const uint64_t *keepx, const uint64_t *woff, uint64_t nl,
                                                  const uint64_t *kw, uint32_t W, PjFilter f, uint64_t rec0, uint64_t word0, uint64_t cnt0, PjRec *recs, uint64_t *wpool,
                                                  uint8_t *cpool)
{
  for (uint64_t i = cl_first(); i < nl; i += cl_stride()) {
    if (!keep[i]) continue;
    const PjLine L = lines[i];
    PjRec R;
    for (uint32_t w = 0; w < 4; w++) R.kw[w] = kw[4 * L.ord + w];
    R.kw[W - 1] |= (uint64_t)L.orient;
    R.woff = word0 + woff[i];
    R.coff = cnt0 + keepx[i] * f.cn;
    R.len = L.len; R.c0 = f.lo; R.cn = f.cn; R.pad = 0;
    recs[rec0 + keepx[i]] = R;
    const uint8_t *j = text + L.line + L.junc_at;
    for (uint32_t w = 0; w * 32u < L.len; w++) {
      uint64_t x = 0;
      const uint32_t m = min(32u, L.len - w * 32u);
      for (uint32_t b = 0; b < m; b++) x |= (uint64_t)base_code(j[w * 32u + b]) << (62u - 2u * b);
      wpool[R.woff + w] = x;
    }
    uint8_t *c = cpool + R.coff;
    for (uint32_t a = 0; a < f.cn; a++) c[a] = 0;
    uint32_t cnt;
    (void)lk_numbers(text, L.line + L.cnt_at, L.line + L.cnt_at + L.cnt_len, cnt, [&](uint32_t at, uint32_t v) {
      for (uint32_t s = f.start[at]; s < f.start[at + 1]; s++) {
        uint8_t *d = c + (f.into[s] - f.lo);
        *d = (uint8_t)min(255u, (uint32_t)*d + min(v, 255u));
      }
    });
  }
}

__device__ __forceinline__ uint64_t pj_word(const PjRec &R, const uint64_t *wpool, uint32_t j) { return (uint64_t)j * 32u < R.len ? wpool[R.woff + j] : 0ull; }
// word w of the sort key of recs[through[i]]: W words of kw, nj junction words, the length
__global__ __launch_bounds__(256) void k_pj_word(const PjRec *recs, const uint64_t *wpool, const uint64_t *through, uint32_t w, uint32_t W, uint32_t nj, uint64_t *dst,
                                                 uint64_t n)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const PjRec &R = recs[through[i]];
    dst[i] = w < W ? R.kw[w] : w < W + nj ? pj_word(R, wpool, w - W) : (uint64_t)R.len;
  }
}
// head[i] = 1 where sorted item i is another link than item i - 1; head[n] = 0 for the scan
__global__ __launch_bounds__(256) void k_pj_heads(const PjRec *recs, const uint64_t *wpool, const uint64_t *perm, uint64_t n, uint8_t *head)
{
  for (uint64_t i = cl_first(); i <= n; i += cl_stride()) {
    uint8_t h = i == n ? 0 : 1;
    if (i > 0 && i < n) {
      const PjRec &a = recs[perm[i]], &b = recs[perm[i - 1]];
      bool same = a.kw[0] == b.kw[0] && a.kw[1] == b.kw[1] && a.kw[2] == b.kw[2] && a.kw[3] == b.kw[3] && a.len == b.len;
      for (uint32_t j = 0; same && j * 32u < a.len; j++) same = wpool[a.woff + j] == wpool[b.woff + j];
      h = same ? 0 : 1;
    }
    head[i] = h;
  }
}
// per run of equal links: row u of the dense U x C matrix = the saturating sums of its lines' counts
__global__ __launch_bounds__(256) void k_pj_reduce(const PjRec *recs, const uint8_t *cpool, const uint64_t *perm, const uint64_t *runstart, uint64_t U, uint32_t C,
                                                   uint8_t *mat)
{
  for (uint64_t u = cl_first(); u < U; u += cl_stride()) {
    uint8_t *row = mat + u * C;
    for (uint32_t c = 0; c < C; c++) row[c] = 0;
    for (uint64_t i = runstart[u]; i < runstart[u + 1]; i++) {
      const PjRec &R = recs[perm[i]];
      for (uint32_t c = 0; c < R.cn; c++) row[R.c0 + c] = (uint8_t)min(255u, (uint32_t)row[R.c0 + c] + cpool[R.coff + c]);
    }
  }
}
// ghead[u] = unique link u is the first of its k-mer; ghead[U] = 0 for the scan
__global__ __launch_bounds__(256) void k_pj_groups(const PjRec *recs, const uint64_t *perm, const uint64_t *runstart, uint64_t U, uint32_t W, uint8_t *ghead)
{
  for (uint64_t u = cl_first(); u <= U; u += cl_stride()) {
    uint8_t h = u == U ? 0 : 1;
    if (u > 0 && u < U) {
      const PjRec &a = recs[perm[runstart[u]]], &b = recs[perm[runstart[u - 1]]];
      bool same = true;
      for (uint32_t j = 0; j < W; j++) same = same && !((a.kw[j] ^ b.kw[j]) & (j + 1 == W ? ~1ull : ~0ull));
      h = same ? 0 : 1;
    }
    ghead[u] = h;
  }
}
__global__ __launch_bounds__(256) void k_pj_totals(const PjRec *recs, const uint64_t *perm, const uint64_t *runstart, const uint8_t *ghead, uint64_t U,
                                                   unsigned long long *ctr)
{
  unsigned long long c_k = 0, c_b = 0;
  for (uint64_t u = cl_first(); u < U; u += cl_stride()) {
    c_k += ghead[u];
    c_b += (recs[perm[runstart[u]]].len + 3u) / 4u;
  }
  block_add(&ctr[kPjKmers], c_k);
  block_add(&ctr[kPjBytes], c_b);
}

// base i (0 = the first) of the k-mer in kw
__device__ __forceinline__ uint32_t pj_kmer_base(const uint64_t *kw, uint32_t W, uint32_t k, uint32_t i)
{
  const uint32_t bit = 2u * (k - 1u - i) + 1u, wi = W - 1u - (bit >> 6), sh = bit & 63u;
  uint64_t x = kw[wi] >> sh;
  if (sh == 63u) x |= kw[wi - 1u] << 1;
  return (uint32_t)x & 3u;
}

struct PjText {
  const PjRec *recs;
  const uint64_t *wpool, *perm, *runstart, *gx, *gstart;
  const uint8_t *ghead, *mat;
  uint64_t U;
  uint32_t k, W, C;
};
// Eight lanes per unique link.  EMIT = false: len[u] = the bytes of link u's line, with the `<kmer> <nlinks>` line
// before it when it is the first of its k-mer; len[U] = 0.  EMIT = true: the lines at out + off[u].
template <bool EMIT> __global__ __launch_bounds__(256) void k_pj_text(PjText a, uint64_t *len, const uint64_t *off, uint8_t *out)
{
  const uint32_t sub = threadIdx.x & 7u;
  const uint64_t per_block = blockDim.x >> 3;
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base <= a.U; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t u = base + (threadIdx.x >> 3);
    if (u > a.U) continue;
    if (u == a.U) { if (!EMIT && sub == 0) len[u] = 0; continue; }
    const PjRec R = a.recs[a.perm[a.runstart[u]]];
    uint8_t *dst = EMIT ? out + off[u] : nullptr;
    uint64_t at = 0;
    if (a.ghead[u]) {
      const uint64_t g = a.gx[u], nl = a.gstart[g + 1] - a.gstart[g];
      const uint32_t d = th_digits(nl);
      if (EMIT) {
        for (uint32_t j = sub; j < a.k; j += 8) dst[j] = (uint8_t)"ACGT"[pj_kmer_base(R.kw, a.W, a.k, j)];
        if (sub == 0) { dst[a.k] = ' '; th_put_num(dst + a.k + 1, nl, d); dst[a.k + 1 + d] = '\n'; }
      }
      at += (uint64_t)a.k + 2 + d;
    }
    const uint32_t d1 = th_digits(R.len);
    const uint8_t *row = a.mat + u * a.C;
    uint64_t cl = a.C - 1;  // the commas
    for (uint32_t c = 0; c < a.C; c++) cl += th_digits(row[c]);
    if (EMIT) {
      uint8_t *p = dst + at;
      if (sub == 0) {
        p[0] = (R.kw[a.W - 1] & 1ull) ? 'R' : 'F'; p[1] = ' ';
        th_put_num(p + 2, R.len, d1); p[2 + d1] = ' ';
        uint8_t *q = p + 3 + d1;
        for (uint32_t c = 0; c < a.C; c++) {
          const uint32_t d2 = th_digits(row[c]);
          if (c) *q++ = ',';
          th_put_num(q, row[c], d2);
          q += d2;
        }
        *q = ' ';
      }
      p += 4 + d1 + cl;
      for (uint32_t j = sub; j < R.len; j += 8) p[j] = (uint8_t)"ACGT"[(uint32_t)(a.wpool[R.woff + (j >> 5)] >> (62u - 2u * (j & 31u))) & 3u];
      if (sub == 0) p[R.len] = '\n';
    }
    at += 4ull + d1 + cl + R.len + 1ull;
    if (!EMIT && sub == 0) len[u] = at;
  }
}

// compaction: per run the junction words it keeps and the extent [lo, lo + cn) of the colours its lines cover;
// nw[U] = cn[U] = 0 for the scans
__global__ __launch_bounds__(256) void k_pj_extent(const PjRec *recs, const uint64_t *perm, const uint64_t *runstart, uint64_t U, uint64_t *nw, uint64_t *cn, uint32_t *lo)
{
  for (uint64_t u = cl_first(); u <= U; u += cl_stride()) {
    if (u == U) { nw[u] = 0; cn[u] = 0; continue; }
    uint32_t a = ~0u, b = 0;
    for (uint64_t i = runstart[u]; i < runstart[u + 1]; i++) {
      const PjRec &R = recs[perm[i]];
      a = min(a, R.c0);
      b = max(b, R.c0 + R.cn);
    }
    nw[u] = (recs[perm[runstart[u]]].len + 31u) / 32u;
    cn[u] = b - a;
    lo[u] = a;
  }
}
// ... and the unique links, sorted, in the store's layout
__global__ __launch_bounds__(256) void k_pj_compact(const PjRec *recs, const uint64_t *wpool, const uint8_t *cpool, const uint64_t *perm, const uint64_t *runstart,
                                                    uint64_t U, const uint64_t *woff, const uint64_t *coff, const uint64_t *cn, const uint32_t *lo, PjRec *nrecs,
                                                    uint64_t *nwpool, uint8_t *ncpool)
{
  for (uint64_t u = cl_first(); u < U; u += cl_stride()) {
    PjRec N = recs[perm[runstart[u]]];
    const uint64_t from = N.woff;
    N.woff = woff[u]; N.coff = coff[u]; N.c0 = lo[u]; N.cn = (uint32_t)cn[u];
    for (uint32_t j = 0; j * 32u < N.len; j++) nwpool[N.woff + j] = wpool[from + j];
    uint8_t *c = ncpool + N.coff;
    for (uint32_t x = 0; x < N.cn; x++) c[x] = 0;
    for (uint64_t i = runstart[u]; i < runstart[u + 1]; i++) {
      const PjRec &R = recs[perm[i]];
      for (uint32_t x = 0; x < R.cn; x++) {
        uint8_t *d = c + (R.c0 + x - N.c0);
        *d = (uint8_t)min(255u, (uint32_t)*d + cpool[R.coff + x]);
      }
    }
    nrecs[u] = N;
  }
}

}  // namespace mcx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mcx_pjoin {
  int k = 0, W = 0, ncols = 0, device = 0, cus = 0;
  uint32_t grid = 0, maxlen = 0;
  uint64_t out_chunk = 64ull << 20, max_bytes = 0;
  bool compact_each = false, dirty = false;  // dirty: lines were added since the last compaction
  hipStream_t stream = nullptr;
  unsigned long long *d_ctr = nullptr, *d_err = nullptr;
  // the store
  PjRec *recs = nullptr;
  uint64_t *wpool = nullptr;
  uint8_t *cpool = nullptr;
  uint64_t n_rec = 0, n_words = 0, n_cnt = 0, cap_rec = 0, cap_words = 0, cap_cnt = 0;
  void *h_buf = nullptr;     // mcx_pjoin_buffer
  uint8_t *h_out = nullptr;  // text delivery
  size_t h_out_cap = 0;
  int err_code = 0;
  uint64_t err_off = 0;
  double ms[6] = {0, 0, 0, 0, 0, 0};  // mcx_pjoin_phases
  mcx_pjoin_stats st{};
};

static unsigned pjoin_grid(const mcx_pjoin *h, uint64_t items)
{
  const uint64_t cap = h->grid ? h->grid : (uint64_t)h->cus * 8;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, cap));
}
static uint64_t pjoin_store_bytes(uint64_t n_rec, uint64_t n_words, uint64_t n_cnt) { return n_rec * sizeof(PjRec) + n_words * 8 + n_cnt; }

#define PJ_LAUNCH(NAME, ITEMS, ...)                                                                       \
  do {                                                                                                    \
    hipLaunchKernelGGL(NAME, dim3(pjoin_grid(h, ITEMS)), dim3(256), 0, st, __VA_ARGS__);                  \
    HIP_TRY(hipGetLastError());                                                                           \
  } while (0)

extern "C" void mcx_pjoin_destroy(mcx_pjoin *h)
{
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->d_ctr) (void)hipFree(h->d_ctr);
  if (h->d_err) (void)hipFree(h->d_err);
  if (h->recs) (void)hipFree(h->recs);
  if (h->wpool) (void)hipFree(h->wpool);
  if (h->cpool) (void)hipFree(h->cpool);
  if (h->h_buf) (void)hipHostFree(h->h_buf);
  if (h->h_out) (void)hipHostFree(h->h_out);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

extern "C" int mcx_pjoin_create(mcx_pjoin **out, int kmer_size, int out_ncols, int device)
{
  if (!out) return fail(MCX_ERR_ARG, "null argument");
  *out = nullptr;
  if (kmer_size < 3 || !(kmer_size & 1) || kmer_size > 127) return fail(MCX_ERR_ARG, "kmer size must be odd, at least 3 and at most 127 (got %d)", kmer_size);
  if (out_ncols < 1 || out_ncols > (1 << 20)) return fail(MCX_ERR_ARG, "pjoin: bad number of output colours: %d", out_ncols);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return fail(MCX_ERR_NODEVICE, "no HIP device found"); }
  if (device < 0 || device >= ndev) return fail(MCX_ERR_NODEVICE, "no HIP device %d (%d found)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  mcx_pjoin *h = new mcx_pjoin();
  ScopeExit drop([&] { mcx_pjoin_destroy(h); });
  h->k = kmer_size; h->W = (2 * kmer_size + 63) / 64; h->ncols = out_ncols; h->device = device;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  h->cus = std::max(1, prop.multiProcessorCount);
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc((void **)&h->d_ctr, kPjNumCounters * sizeof(unsigned long long)));
  HIP_TRY(hipMalloc((void **)&h->d_err, sizeof(unsigned long long)));
  drop.dismiss();
  *out = h;
  return MCX_OK;
}

extern "C" int mcx_pjoin_configure(mcx_pjoin *h, const char *key, uint64_t value)
{
  if (!h || !key) return fail(MCX_ERR_ARG, "null argument");
  if (!strcmp(key, "grid")) { h->grid = (uint32_t)std::min<uint64_t>(value, 1u << 20); return MCX_OK; }
  if (!strcmp(key, "out_chunk")) { h->out_chunk = value ? value : (64ull << 20); return MCX_OK; }
  if (!strcmp(key, "compact")) { h->compact_each = value != 0; return MCX_OK; }
  if (!strcmp(key, "max_bytes")) { h->max_bytes = value; return MCX_OK; }
  return fail(MCX_ERR_ARG, "unknown pjoin configuration key: %s", key);
}

extern "C" int mcx_pjoin_get_stats(const mcx_pjoin *h, mcx_pjoin_stats *stats)
{
  if (!h || !stats) return fail(MCX_ERR_ARG, "null argument");
  *stats = h->st;
  return MCX_OK;
}

extern "C" int mcx_pjoin_phases(const mcx_pjoin *h, double *ms)
{
  if (!h || !ms) return fail(MCX_ERR_ARG, "null argument");
  for (int i = 0; i < 6; i++) ms[i] = h->ms[i];
  return MCX_OK;
}

extern "C" int mcx_pjoin_error(const mcx_pjoin *h, int *code, uint64_t *byte_offset)
{
  if (!h) return fail(MCX_ERR_ARG, "null argument");
  if (code) *code = h->err_code;
  if (byte_offset) *byte_offset = h->err_off;
  return MCX_OK;
}

extern "C" int mcx_pjoin_buffer(mcx_pjoin *h, size_t bytes, void **ptr)
{
  if (!h || !ptr || !bytes) return fail(MCX_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  if (h->h_buf) { (void)hipHostFree(h->h_buf); h->h_buf = nullptr; }
  HIP_TRY(hipHostMalloc(&h->h_buf, bytes, hipHostMallocDefault));
  *ptr = h->h_buf;
  return MCX_OK;
}

// the store sorted: *perm orders its records by (kw, junctions, length), runstart[u] = the first item of run u of equal
// links (runstart[U] = n_rec).  The buffers of `s` hold both until it goes.
struct PjSorted {
  DevBuf<uint64_t> p0, p1, k0, k1;
  DevBuf<uint8_t> tmp, head;
  uint64_t *perm = nullptr, *runstart = nullptr, *ex = nullptr, U = 0;
};
static int pjoin_sort(mcx_pjoin *h, PjSorted &s)
{
  hipStream_t st = h->stream;
  const uint64_t n = h->n_rec;
  const uint32_t nj = (h->maxlen + 31u) / 32u, W = (uint32_t)h->W;
  int rc;
  size_t tmp_bytes = 0;
  if ((rc = sort_perm_scratch(st, n, &tmp_bytes)) != MCX_OK) return rc;
  HIP_TRY(s.p0.alloc(n + 1));
  HIP_TRY(s.p1.alloc(n + 1));
  HIP_TRY(s.k0.alloc(n + 1));
  HIP_TRY(s.k1.alloc(n + 1));
  HIP_TRY(s.tmp.alloc(tmp_bytes ? tmp_bytes : 16));
  HIP_TRY(s.head.alloc(n + 1));
  HIP_TRY(hipMemsetAsync(s.head.p, 1, n, st));  // iota: the exclusive sum of ones
  if ((rc = device_scan(st, (const uint8_t *)s.head.p, s.p0.p, n)) != MCX_OK) return rc;
  auto word = [&](int w, bool, const uint64_t *through, uint64_t *dst, const uint64_t **) -> int {
    PJ_LAUNCH(k_pj_word, n, (const PjRec *)h->recs, (const uint64_t *)h->wpool, through, (uint32_t)w, W, nj, dst, n);
    return MCX_OK;
  };
  uint64_t *const keys[2] = {s.k0.p, s.k1.p}, *const perms[2] = {s.p0.p, s.p1.p};
  if ((rc = sort_perm_by_words(st, n, (int)(W + nj) + 1, 2 * h->k + 1 - 64 * (h->W - 1), keys, perms, s.tmp.p, tmp_bytes, nullptr, word, &s.perm)) != MCX_OK) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return MCX_OK;
}
static int pjoin_runs(mcx_pjoin *h, PjSorted &s)
{
  hipStream_t st = h->stream;
  const uint64_t n = h->n_rec;
  int rc;
  s.runstart = s.perm == s.p0.p ? s.p1.p : s.p0.p;
  s.ex = s.k0.p;
  PJ_LAUNCH(k_pj_heads, n + 1, (const PjRec *)h->recs, (const uint64_t *)h->wpool, (const uint64_t *)s.perm, n, s.head.p);
  if ((rc = scan_total(st, (const uint8_t *)s.head.p, s.ex, n + 1, &s.U)) != MCX_OK) return rc;
  PJ_LAUNCH(k_th_runs, n + 1, (const uint8_t *)s.head.p, (const uint64_t *)s.ex, n, s.runstart);
  return MCX_OK;
}

// the store becomes its unique links, sorted (phases 3 and 4)
static int pjoin_compact(mcx_pjoin *h)
{
  if (!h->n_rec || !h->dirty) return MCX_OK;
  hipStream_t st = h->stream;
  double t_ph = now_s();
  auto phase = [&](int i) { (void)hipStreamSynchronize(st); const double t = now_s(); h->ms[i] += (t - t_ph) * 1e3; t_ph = t; };
  int rc;
  PjSorted s;
  if ((rc = pjoin_sort(h, s)) != MCX_OK) return rc;
  phase(3);
  if ((rc = pjoin_runs(h, s)) != MCX_OK) return rc;
  const uint64_t U = s.U;
  DevBuf<uint64_t> d_nw, d_cn, d_woff, d_coff, n_wpool;
  DevBuf<uint32_t> d_lo;
  DevBuf<PjRec> n_recs;
  DevBuf<uint8_t> n_cpool;
  HIP_TRY(d_nw.alloc(U + 1));
  HIP_TRY(d_cn.alloc(U + 1));
  HIP_TRY(d_woff.alloc(U + 1));
  HIP_TRY(d_coff.alloc(U + 1));
  HIP_TRY(d_lo.alloc(U + 1));
  PJ_LAUNCH(k_pj_extent, U + 1, (const PjRec *)h->recs, (const uint64_t *)s.perm, (const uint64_t *)s.runstart, U, d_nw.p, d_cn.p, d_lo.p);
  uint64_t nwords = 0, ncnt = 0;
  if ((rc = scan_total(st, (const uint64_t *)d_nw.p, d_woff.p, U + 1, &nwords)) != MCX_OK) return rc;
  if ((rc = scan_total(st, (const uint64_t *)d_cn.p, d_coff.p, U + 1, &ncnt)) != MCX_OK) return rc;
  HIP_TRY(n_recs.alloc(std::max<uint64_t>(U, 1)));
  HIP_TRY(n_wpool.alloc(std::max<uint64_t>(nwords, 1)));
  HIP_TRY(n_cpool.alloc(std::max<uint64_t>(ncnt, 1)));
  PJ_LAUNCH(k_pj_compact, U, (const PjRec *)h->recs, (const uint64_t *)h->wpool, (const uint8_t *)h->cpool, (const uint64_t *)s.perm, (const uint64_t *)s.runstart, U,
            (const uint64_t *)d_woff.p, (const uint64_t *)d_coff.p, (const uint64_t *)d_cn.p, (const uint32_t *)d_lo.p, n_recs.p, n_wpool.p, n_cpool.p);
  HIP_TRY(hipStreamSynchronize(st));
  (void)hipFree(h->recs); (void)hipFree(h->wpool); (void)hipFree(h->cpool);
  h->recs = n_recs.p; h->wpool = n_wpool.p; h->cpool = n_cpool.p;
  n_recs.p = nullptr; n_wpool.p = nullptr; n_cpool.p = nullptr;
  h->n_rec = U; h->n_words = nwords; h->n_cnt = ncnt;
  h->cap_rec = std::max<uint64_t>(U, 1); h->cap_words = std::max<uint64_t>(nwords, 1); h->cap_cnt = std::max<uint64_t>(ncnt, 1);
  h->dirty = false;
  h->st.compactions++;
  h->st.store_bytes = pjoin_store_bytes(h->n_rec, h->n_words, h->n_cnt);
  phase(4);
  return MCX_OK;
}

// one array of the store grown (by doubling) to hold `need` items, what it holds kept
template <class T> static int pjoin_grow(mcx_pjoin *h, T **arr, uint64_t *cap, uint64_t used, uint64_t need)
{
  if (need <= *cap) return MCX_OK;
  uint64_t ncap = std::max<uint64_t>(*cap, 1024);
  while (ncap < need) ncap *= 2;
  T *p = nullptr;
  if (hipMalloc((void **)&p, ncap * sizeof(T)) != hipSuccess) {  // (doubling is a wish: exactly what is needed will do)
    (void)hipGetLastError();
    ncap = need;
    HIP_TRY(hipMalloc((void **)&p, ncap * sizeof(T)));
  }
  if (used) {
    const hipError_t e = hipMemcpyAsync(p, *arr, used * sizeof(T), hipMemcpyDeviceToDevice, h->stream);
    if (e != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) { (void)hipFree(p); return fail(MCX_ERR_HIP, "pjoin: the store could not be moved"); }
  }
  if (*arr) (void)hipFree(*arr);
  *arr = p;
  *cap = ncap;
  return MCX_OK;
}
// room for a piece's records, words and counts; a full store compacts once before the answer is MCX_ERR_NOMEM
static int pjoin_reserve(mcx_pjoin *h, uint64_t a_rec, uint64_t a_words, uint64_t a_cnt)
{
  for (int round = 0;; round++) {
    const uint64_t need = pjoin_store_bytes(h->n_rec + a_rec, h->n_words + a_words, h->n_cnt + a_cnt);
    int rc = MCX_OK;
    if (h->max_bytes && need > h->max_bytes) rc = fail(MCX_ERR_NOMEM, "pjoin: the store would take %llu bytes (\"max_bytes\" is %llu)", (unsigned long long)need, (unsigned long long)h->max_bytes);
    if (rc == MCX_OK) rc = pjoin_grow(h, &h->recs, &h->cap_rec, h->n_rec, h->n_rec + a_rec);
    if (rc == MCX_OK) rc = pjoin_grow(h, &h->wpool, &h->cap_words, h->n_words, h->n_words + a_words);
    if (rc == MCX_OK) rc = pjoin_grow(h, &h->cpool, &h->cap_cnt, h->n_cnt, h->n_cnt + a_cnt);
    if (rc != MCX_ERR_NOMEM || round || !h->dirty) return rc;
    if ((rc = pjoin_compact(h)) != MCX_OK) return rc;
  }
}

extern "C" int mcx_pjoin_add_text(mcx_pjoin *h, const void *text, uint64_t nbytes, int src_ncols, const int32_t *filter, int nfilter, mcx_pjoin_piece_stats *ps)
{
  if (ps) memset(ps, 0, sizeof(*ps));
  if (!h) return fail(MCX_ERR_ARG, "null argument");
  if (src_ncols < 1 || src_ncols > (1 << 20)) return fail(MCX_ERR_ARG, "pjoin: bad number of colours in the file: %d", src_ncols);
  if (nfilter < 0 || (nfilter && !filter)) return fail(MCX_ERR_ARG, "pjoin: bad filter");
  for (int i = 0; i < nfilter; i++)
    if (filter[2 * i] < 0 || filter[2 * i] >= src_ncols || filter[2 * i + 1] < 0 || filter[2 * i + 1] >= h->ncols)
      return fail(MCX_ERR_ARG, "pjoin: filter entry %d:%d is out of range (%d colours in the file, %d in the output)", filter[2 * i], filter[2 * i + 1], src_ncols, h->ncols);
  if (!nbytes) return MCX_OK;
  if (!text) return fail(MCX_ERR_ARG, "null text");
  if (nbytes >= (1ull << 31)) return fail(MCX_ERR_ARG, "pjoin: a piece of %llu bytes (2 GB at the most)", (unsigned long long)nbytes);
  if (((const uint8_t *)text)[nbytes - 1] != '\n') return fail(MCX_ERR_ARG, "pjoin: the text does not end with a newline");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  double t_ph = now_s();
  auto phase = [&](int i) { (void)hipStreamSynchronize(st); const double t = now_s(); h->ms[i] += (t - t_ph) * 1e3; t_ph = t; };
  const uint32_t k = (uint32_t)h->k, W = (uint32_t)h->W;
  int rc;
  h->err_code = 0; h->err_off = 0;

  // the filter by source colour
  std::vector<uint32_t> fstart((size_t)src_ncols + 1, 0), finto((size_t)std::max(nfilter, 1), 0);
  uint32_t lo = 0, hi = 0;
  for (int i = 0; i < nfilter; i++) fstart[(size_t)filter[2 * i] + 1]++;
  for (int c = 0; c < src_ncols; c++) fstart[(size_t)c + 1] += fstart[(size_t)c];
  {
    std::vector<uint32_t> at(fstart.begin(), fstart.end() - 1);
    for (int i = 0; i < nfilter; i++) {
      const uint32_t into = (uint32_t)filter[2 * i + 1];
      finto[at[(size_t)filter[2 * i]]++] = into;
      lo = i ? std::min(lo, into) : into;
      hi = i ? std::max(hi, into + 1) : into + 1;
    }
  }
  DevBuf<uint32_t> d_fstart, d_finto;
  HIP_TRY(d_fstart.alloc(fstart.size()));
  HIP_TRY(d_finto.alloc(finto.size()));
  HIP_TRY(hipMemcpyAsync(d_fstart.p, fstart.data(), fstart.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_finto.p, finto.data(), finto.size() * 4, hipMemcpyHostToDevice, st));
  PjFilter f;
  f.start = d_fstart.p; f.into = d_finto.p; f.src_ncols = (uint32_t)src_ncols; f.lo = lo; f.cn = hi - lo;

  // 1. lines
  const uint64_t n = nbytes;
  DevBuf<uint8_t> d_text, d_flag, d_kflag, d_lflag, d_keep;
  DevBuf<uint64_t> d_lidx, d_lstart, d_kx, d_lx, d_kline, d_kw, d_nw, d_woff, d_keepx;
  DevBuf<PjLine> d_lines;
  HIP_TRY(d_text.alloc(n + 16));
  HIP_TRY(d_flag.alloc(n + 1));
  HIP_TRY(d_lidx.alloc(n + 1));
  HIP_TRY(hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_text.p + n, 0, 16, st));
  HIP_TRY(hipMemsetAsync(h->d_ctr, 0, kPjNumCounters * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(h->d_err, 0xff, sizeof(unsigned long long), st));
  phase(0);
  PJ_LAUNCH(k_lk_mark, n + 1, (const uint8_t *)d_text.p, n, d_flag.p);
  uint64_t nlines = 0, nk = 0, nl = 0;
  if ((rc = scan_total(st, (const uint8_t *)d_flag.p, d_lidx.p, n + 1, &nlines)) != MCX_OK) return rc;
  HIP_TRY(d_lstart.alloc(nlines + 1));
  HIP_TRY(d_kflag.alloc(nlines + 1));
  HIP_TRY(d_lflag.alloc(nlines + 1));
  HIP_TRY(d_kx.alloc(nlines + 1));
  HIP_TRY(d_lx.alloc(nlines + 1));
  PJ_LAUNCH(k_lk_starts, n + 1, (const uint8_t *)d_flag.p, (const uint64_t *)d_lidx.p, n, d_lstart.p);
  PJ_LAUNCH(k_lk_class, nlines + 1, (const uint8_t *)d_text.p, (const uint64_t *)d_lstart.p, nlines, d_kflag.p, d_lflag.p);
  if ((rc = scan_total(st, (const uint8_t *)d_kflag.p, d_kx.p, nlines + 1, &nk)) != MCX_OK) return rc;
  if ((rc = scan_total(st, (const uint8_t *)d_lflag.p, d_lx.p, nlines + 1, &nl)) != MCX_OK) return rc;
  d_flag.release();
  d_lidx.release();
  HIP_TRY(d_kline.alloc(nk + 1));
  PJ_LAUNCH(k_lk_klines, nlines, (const uint8_t *)d_kflag.p, (const uint64_t *)d_kx.p, nlines, d_kline.p);
  phase(1);

  // 2. parse and store
  HIP_TRY(d_kw.alloc(4 * nk + 4));
  HIP_TRY(d_lines.alloc(nl + 1));
  HIP_TRY(d_keep.alloc(nl + 1));
  HIP_TRY(d_keepx.alloc(nl + 1));
  HIP_TRY(d_nw.alloc(nl + 1));
  HIP_TRY(d_woff.alloc(nl + 1));
  PJ_LAUNCH(k_pj_parse, nlines + 1, (const uint8_t *)d_text.p, (const uint64_t *)d_lstart.p, nlines, (const uint8_t *)d_kflag.p, (const uint8_t *)d_lflag.p,
            (const uint64_t *)d_kx.p, (const uint64_t *)d_lx.p, (const uint64_t *)d_kline.p, nk, k, W, f, d_lines.p, d_keep.p, d_nw.p, d_kw.p, h->d_err, h->d_ctr);
  unsigned long long h_err = 0, h_ctr[kPjNumCounters];
  HIP_TRY(hipMemcpyAsync(&h_err, h->d_err, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_ctr, h->d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h_err != kLkNoErr) {
    h->err_code = (int)(h_err & 0xffu);
    h->err_off = h_err >> 8;
    return fail(MCX_ERR_INVAL, "pjoin: bad line at byte %llu of the piece (refusal %d)", (unsigned long long)h->err_off, h->err_code);
  }
  uint64_t nkept = 0, nwords = 0;
  if ((rc = scan_total(st, (const uint8_t *)d_keep.p, d_keepx.p, nl + 1, &nkept)) != MCX_OK) return rc;
  if ((rc = scan_total(st, (const uint64_t *)d_nw.p, d_woff.p, nl + 1, &nwords)) != MCX_OK) return rc;
  if (nkept) {
    if ((rc = pjoin_reserve(h, nkept, nwords, nkept * f.cn)) != MCX_OK) return rc;
    PJ_LAUNCH(k_pj_store, nl, (const uint8_t *)d_text.p, (const PjLine *)d_lines.p, (const uint8_t *)d_keep.p, (const uint64_t *)d_keepx.p, (const uint64_t *)d_woff.p, nl,
              (const uint64_t *)d_kw.p, W, f, h->n_rec, h->n_words, h->n_cnt, h->recs, h->wpool, h->cpool);
    HIP_TRY(hipStreamSynchronize(st));
    h->n_rec += nkept; h->n_words += nwords; h->n_cnt += nkept * f.cn;
    h->maxlen = std::max(h->maxlen, (uint32_t)h_ctr[kPjMaxLen]);
    h->dirty = true;
  }
  h->st.kmer_lines += h_ctr[kPjKmerLines];
  h->st.link_lines += h_ctr[kPjLinkLines];
  h->st.links_kept += nkept;
  h->st.kmers_n_mismatch += h_ctr[kPjBadN];
  h->st.store_bytes = pjoin_store_bytes(h->n_rec, h->n_words, h->n_cnt);
  h->st.peak_store_bytes = std::max(h->st.peak_store_bytes, h->st.store_bytes);
  if (ps) { ps->kmer_lines = h_ctr[kPjKmerLines]; ps->link_lines = h_ctr[kPjLinkLines]; ps->links_kept = nkept; ps->kmers_n_mismatch = h_ctr[kPjBadN]; }
  phase(2);
  if (h->compact_each && (rc = pjoin_compact(h)) != MCX_OK) return rc;
  return MCX_OK;
}

extern "C" int mcx_pjoin_finish(mcx_pjoin *h, mcx_sink_fn sink, void *ctx, mcx_pjoin_stats *stats)
{
  if (!h) return fail(MCX_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  double t_ph = now_s();
  auto phase = [&](int i) { (void)hipStreamSynchronize(st); const double t = now_s(); h->ms[i] += (t - t_ph) * 1e3; t_ph = t; };
  int rc;
  h->st.kmers = h->st.links = h->st.path_bytes = 0;
  if (h->n_rec) {
    const uint32_t C = (uint32_t)h->ncols;
    PjSorted s;
    if ((rc = pjoin_sort(h, s)) != MCX_OK) return rc;
    phase(3);
    if ((rc = pjoin_runs(h, s)) != MCX_OK) return rc;
    const uint64_t U = s.U;
    DevBuf<uint8_t> d_mat, d_ghead, d_out;
    DevBuf<uint64_t> d_gx, d_gstart, d_len, d_off;
    HIP_TRY(d_mat.alloc(U * C));
    HIP_TRY(d_ghead.alloc(U + 1));
    HIP_TRY(d_gx.alloc(U + 1));
    PJ_LAUNCH(k_pj_reduce, U, (const PjRec *)h->recs, (const uint8_t *)h->cpool, (const uint64_t *)s.perm, (const uint64_t *)s.runstart, U, C, d_mat.p);
    PJ_LAUNCH(k_pj_groups, U + 1, (const PjRec *)h->recs, (const uint64_t *)s.perm, (const uint64_t *)s.runstart, U, (uint32_t)h->W, d_ghead.p);
    uint64_t G = 0;
    if ((rc = scan_total(st, (const uint8_t *)d_ghead.p, d_gx.p, U + 1, &G)) != MCX_OK) return rc;
    HIP_TRY(d_gstart.alloc(G + 1));
    PJ_LAUNCH(k_th_runs, U + 1, (const uint8_t *)d_ghead.p, (const uint64_t *)d_gx.p, U, d_gstart.p);
    HIP_TRY(hipMemsetAsync(h->d_ctr, 0, kPjNumCounters * sizeof(unsigned long long), st));
    PJ_LAUNCH(k_pj_totals, U, (const PjRec *)h->recs, (const uint64_t *)s.perm, (const uint64_t *)s.runstart, (const uint8_t *)d_ghead.p, U, h->d_ctr);
    unsigned long long h_ctr[kPjNumCounters];
    HIP_TRY(hipMemcpyAsync(h_ctr, h->d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->st.kmers = h_ctr[kPjKmers];
    h->st.links = U;
    h->st.path_bytes = h_ctr[kPjBytes];
    phase(4);
    if (sink) {
      HIP_TRY(d_len.alloc(U + 1));
      HIP_TRY(d_off.alloc(U + 1));
      PjText a;
      a.recs = h->recs; a.wpool = h->wpool; a.perm = s.perm; a.runstart = s.runstart; a.gx = d_gx.p; a.gstart = d_gstart.p; a.ghead = d_ghead.p; a.mat = d_mat.p;
      a.U = U; a.k = (uint32_t)h->k; a.W = (uint32_t)h->W; a.C = C;
      PJ_LAUNCH(k_pj_text<false>, (U + 1) * 8, a, d_len.p, (const uint64_t *)nullptr, (uint8_t *)nullptr);
      uint64_t total = 0;
      if ((rc = scan_total(st, (const uint64_t *)d_len.p, d_off.p, U + 1, &total)) != MCX_OK) return rc;
      HIP_TRY(d_out.alloc(total + 1));
      PJ_LAUNCH(k_pj_text<true>, (U + 1) * 8, a, (uint64_t *)nullptr, (const uint64_t *)d_off.p, d_out.p);
      if ((rc = text_deliver(st, h->out_chunk, &h->h_out, &h->h_out_cap, d_out.p, total, sink, ctx, "pjoin", ".ctp text")) != MCX_OK) return rc;
    }
    phase(5);
  }
  if (stats) *stats = h->st;
  return MCX_OK;
}
