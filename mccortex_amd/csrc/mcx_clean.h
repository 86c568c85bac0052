// mcx_clean.h -- `clean` on the device (included by mcx_api.hip).
//
// clean_graph (src/tools/clean_graph.c) over the table: split the graph into unitigs (db_unitig.c),
// take each unitig's median coverage and end degrees, decide once which unitigs stay, then prune
// (prune_nodes_lacking_flag, src/graph/prune_nodes.c).  Steps ("clean's device passes"):
//   A. k_cl_compact   occupied slots -> dense ids 0..n-1 (slot_of, map), union edges, summed coverage
//      k_cl_links     per oriented node (2 i + o) the linked neighbour: the side has exactly one edge, the
//                     neighbour exists, is not the same key, and its only edge facing back leads here
//   B. k_cl_jump      pointer jumping (Wyllie) over the 2n oriented nodes: nxt doubles, mn = the minimum
//                     dense id of the window [v, nxt(v)]; repeated until a round changes nothing
//      k_cl_unitig    unitig id = the minimum dense id over both directions, length, end degrees
//   C. radix sort of (unitig id << 32 | coverage), k_cl_median: exact median per unitig
//   D. k_cl_decide, k_cl_kmer_hist, k_cl_prune_edges, k_cl_tombstone
// Every kernel is a grid-stride loop (the "grid" knob caps the launches).
#pragma once
#include "mcx_kernels.h"
#include "mcx_infer.h"  // kmer_push_front

namespace mcx {

constexpr uint32_t kClNone = 0xFFFFFFFFu;
constexpr uint32_t kClBins = 1000;  // DUMP_COVG_ARRSIZE, DUMP_LEN_ARRSIZE (clean_graph.c)

__device__ __forceinline__ uint64_t cl_stride() { return (uint64_t)gridDim.x * blockDim.x; }
__device__ __forceinline__ uint64_t cl_first() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint32_t cl_outdeg(uint8_t ue, uint32_t o) { return (uint32_t)__popc((ue >> (4 * o)) & 15u); }
// end(v): oriented node v has no link on its out side
__device__ __forceinline__ bool cl_end(const uint8_t *lk, uint32_t v) { return !((lk[v >> 1] >> (v & 1u)) & 1u); }

template <int W> __device__ __forceinline__ Kmer<W> cl_key(const TableView &t, uint64_t slot)
{
  const uint64_t *r = key_ptr(t, slot);
  Kmer<W> x;
  x.w[0] = r[0] & ~kFlag;
  for (int i = 1; i < W; i++) x.w[i] = r[i];
  return x;
}

// neighbour of oriented node (key, o) over edge nucleotide x: its slot (kNoSlot: absent) and orientation
template <int W>
__device__ __forceinline__ uint64_t cl_next(const TableView &t, const Kmer<W> &key, uint32_t o, uint32_t x, int k, uint32_t &p)
{
  Kmer<W> nb = key;
  if (o == 0) kmer_push<W>(nb, x, k);
  else kmer_push_front<W>(nb, 3u - x, k);
  const Kmer<W> rc = revcomp<W>(nb, k);
  const bool fw = kmer_less<W>(nb, rc);
  p = o ^ (fw ? 0u : 1u);  // the oriented next sequence is nb (o = 0) or revcomp(nb) (o = 1)
  uint32_t novel = 0, full = 0;
  return find_or_insert_rec<W>(t, fw ? nb : rc, true, novel, full);  // must_exist: read-only
}

// dense ids: slot_of[id] = slot, map[slot] = id; ue = union of the colours' edges; cov = summed coverage
// (each colour clamped to 2^32-1, the sum saturating: db_node_sum_covg).  Ids >= cap are counted but not
// stored: the host compares the count with the k-mer counter and fails the call.
__global__ __launch_bounds__(256) void k_cl_compact(TableView t, uint32_t ncols, uint64_t cap, uint64_t *slot_of, uint32_t *map,
                                                    uint8_t *ue, uint32_t *cov, unsigned long long *cursor)
{
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < t.nslots; base += cl_stride()) {
    const uint64_t slot = base + threadIdx.x;
    const bool occ = slot < t.nslots && (key_ptr(t, slot)[0] & kFlag);
    const uint64_t id = wave_append(cursor, occ);
    if (!occ) continue;
    if (id >= cap) continue;
    slot_of[id] = slot;
    map[slot] = (uint32_t)id;
    uint32_t e = 0;
    uint64_t sum = 0;
    for (uint32_t c = 0; c < ncols; c++) {
      const uint64_t v = *val_ptr(t, slot, c);
      uint64_t cv = v >> 8;
      if (cv > 0xFFFFFFFFull) cv = 0xFFFFFFFFull;
      sum += cv;
      e |= (uint32_t)(v & 0xffu);
    }
    ue[id] = (uint8_t)e;
    cov[id] = (uint32_t)(sum > 0xFFFFFFFFull ? 0xFFFFFFFFull : sum);
  }
}

// lk[i] bit o: side o of k-mer i is linked; nxt[2i+o] = 2j+p of the link (or 2i+o itself at an end),
// mn[2i+o] = min(i, j) -- the window [v, nxt(v)] of the ranking
template <int W>
__global__ __launch_bounds__(256) void k_cl_links(TableView t, int k, uint64_t n, const uint64_t *slot_of, const uint32_t *map,
                                                  const uint8_t *ue, uint8_t *lk, uint32_t *nxt, uint32_t *mn)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const uint64_t slot = slot_of[i];
    const uint8_t e = ue[i];
    uint32_t bits = 0;
    Kmer<W> key;
    bool have_key = false;
    for (uint32_t o = 0; o < 2; o++) {
      const uint32_t v = (uint32_t)(2 * i + o);
      uint32_t to = v, m = (uint32_t)i;
      const uint32_t nib = (e >> (4 * o)) & 15u;
      if (__popc(nib) == 1) {
        if (!have_key) { key = cl_key<W>(t, slot); have_key = true; }
        const uint32_t x = (uint32_t)__ffs(nib) - 1u;
        uint32_t p = 0;
        const uint64_t s = cl_next<W>(t, key, o, x, k, p);
        if (s != kNoSlot && s != slot) {
          const uint32_t j = map[s];
          // the nucleotide on the neighbour's side facing back that leads to this k-mer
          const uint32_t y = o == 0 ? 3u - kmer_first_base<W>(key, k) : (uint32_t)(key.w[W - 1] & 3u);
          if (((ue[j] >> (4 * (p ^ 1u))) & 15u) == (1u << y)) {
            to = 2 * j + p;
            m = j < (uint32_t)i ? j : (uint32_t)i;
            bits |= 1u << o;
          }
        }
      }
      nxt[v] = to;
      mn[v] = m;
    }
    lk[i] = (uint8_t)bits;
  }
}

// one round of pointer jumping; *changed = 1 when some node reached an end this round or some window
// minimum fell.  When a round sets neither, every node off a cycle points at its chain's end and every
// minimum covers the node's whole chain (or whole cycle): DESIGN.md section 4 ("clean's device passes") gives the argument.
__global__ __launch_bounds__(256) void k_cl_jump(uint64_t n2, const uint8_t *lk, const uint32_t *nxt_in, const uint32_t *mn_in,
                                                 uint32_t *nxt_out, uint32_t *mn_out, uint32_t *changed)
{
  uint32_t ch = 0;
  for (uint64_t v = cl_first(); v < n2; v += cl_stride()) {
    const uint32_t a = nxt_in[v], m0 = mn_in[v];
    if (cl_end(lk, a)) { nxt_out[v] = a; mn_out[v] = m0; continue; }  // done
    const uint32_t b = nxt_in[a], ma = mn_in[a];
    const uint32_t m = ma < m0 ? ma : m0;
    nxt_out[v] = b;
    mn_out[v] = m;
    ch |= (m != m0) || cl_end(lk, b);
  }
  if (ch) *changed = 1u;
}

// unitig id, length and (at the id's own k-mer) the end degrees indeg(first) + outdeg(last); 2 on a cycle
__global__ __launch_bounds__(256) void k_cl_unitig(uint64_t n, const uint32_t *nxt, const uint32_t *mn, const uint8_t *lk,
                                                   const uint8_t *ue, uint32_t *uid, uint32_t *len, uint8_t *ends)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const uint32_t m0 = mn[2 * i], m1 = mn[2 * i + 1];
    const uint32_t u = m0 < m1 ? m0 : m1;
    uid[i] = u;
    atomicAdd(&len[u], 1u);
    if (u == (uint32_t)i) {
      const uint32_t a0 = nxt[2 * i], a1 = nxt[2 * i + 1];
      uint32_t d = 2;  // a closed cycle: every node has one edge in and one out
      if (cl_end(lk, a0)) d = cl_outdeg(ue[a0 >> 1], a0 & 1u) + cl_outdeg(ue[a1 >> 1], a1 & 1u);
      ends[i] = (uint8_t)d;
    }
  }
}

__global__ __launch_bounds__(256) void k_cl_keys(uint64_t n, const uint32_t *uid, const uint32_t *cov, uint64_t *keys)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) keys[i] = (uint64_t)uid[i] << 32 | cov[i];
}

// histogram bins accumulated in LDS (nearly every unitig lands in the low bins), flushed with one atomic per bin
struct ClHist {
  uint32_t *s;
  __device__ void zero(uint32_t nh) { for (uint32_t b = threadIdx.x; b < nh * kClBins; b += blockDim.x) s[b] = 0; __syncthreads(); }
  __device__ void add(uint32_t h, uint64_t x) { atomicAdd(&s[h * kClBins + (x < kClBins - 1 ? x : kClBins - 1)], 1u); }
  __device__ void flush(uint32_t nh, unsigned long long *g)
  {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nh * kClBins; b += blockDim.x)
      if (s[b]) atomicAdd(&g[b], (unsigned long long)s[b]);
  }
};

// sorted (unitig id, coverage) keys: at the first key of each unitig, the median (gca_median_uint32: the
// middle value, or the mean of the two middle values rounded down) and the "before" histograms
// hist[0..999] = unitig median coverage, hist[1000..1999] = unitig length
__global__ __launch_bounds__(256) void k_cl_median(uint64_t n, const uint64_t *sorted, const uint32_t *len, uint32_t *med,
                                                   unsigned long long *hist)
{
  __shared__ uint32_t s_h[2 * kClBins];
  ClHist h{s_h};
  h.zero(2);
  for (uint64_t s = cl_first(); s < n; s += cl_stride()) {
    const uint32_t u = (uint32_t)(sorted[s] >> 32);
    if (s > 0 && (uint32_t)(sorted[s - 1] >> 32) == u) continue;
    const uint32_t L = len[u];
    const uint64_t a = (uint32_t)sorted[s + (L - 1) / 2], b = (uint32_t)sorted[s + L / 2];
    const uint32_t m = (uint32_t)((a + b) >> 1);
    med[u] = m;
    if (hist) { h.add(0, m); h.add(1, L); }
  }
  if (hist) h.flush(2, hist);
}

// k-mer coverage histogram, of all k-mers (keep == nullptr) or of the kept ones
__global__ __launch_bounds__(256) void k_cl_kmer_hist(uint64_t n, const uint32_t *cov, const uint32_t *uid, const uint8_t *keep,
                                                      unsigned long long *hist)
{
  __shared__ uint32_t s_h[kClBins];
  ClHist h{s_h};
  h.zero(1);
  for (uint64_t i = cl_first(); i < n; i += cl_stride())
    if (!keep || keep[uid[i]]) h.add(0, cov[i]);
  h.flush(1, hist);
}

// unitig_mark (clean_graph.c): low = median < threshold, removable tip = length < min_keep_tip and
// indeg(first) + outdeg(last) <= 1.  st[0..5] = tip / tip k-mers, low / low k-mers, both / both k-mers
// (UnitigCleanerStats); hist = the "after" unitig coverage and length histograms of the kept unitigs
__global__ __launch_bounds__(256) void k_cl_decide(uint64_t n, const uint32_t *len, const uint32_t *med, const uint8_t *ends,
                                                   uint32_t threshold, uint32_t min_keep_tip, uint8_t *keep,
                                                   unsigned long long *st, unsigned long long *hist)
{
  __shared__ uint32_t s_h[2 * kClBins];
  ClHist h{s_h};
  h.zero(2);
  unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
  for (uint64_t u = cl_first(); u < n; u += cl_stride()) {
    const uint32_t L = len[u];
    if (!L) continue;  // not a unitig id
    const bool low = med[u] < threshold;
    const bool tip = L < min_keep_tip && ends[u] <= 1;
    const int cls = low && tip ? 4 : low ? 2 : tip ? 0 : -1;
    keep[u] = cls < 0;
    if (cls >= 0) { c[cls]++; c[cls + 1] += L; }
    else { h.add(0, med[u]); h.add(1, L); }
  }
  for (int i = 0; i < 6; i++) block_add(&st[i], c[i]);
  h.flush(2, hist);
}

// Which k-mers stay, asked by dense id.  clean and popbubbles keep whole unitigs: a byte per unitig id behind the
// k-mer's 4-byte unitig id.  (subgraph keeps marked k-mers: KeepMark, mcx_subgraph.h.)
struct KeepUnitig {
  const uint32_t *uid;
  const uint8_t *keep;
  __device__ __forceinline__ bool operator()(uint64_t id) const { return keep[uid[id]] != 0; }
};

// prune_edges_to_nodes_lacking_flag: a kept k-mer loses, in every colour, each union edge whose neighbour is
// not kept -- or is not in the graph at all (the reference asserts there)
template <int W, class Keep>
__device__ __forceinline__ void cl_prune_edges(const TableView &t, int k, uint32_t ncols, uint64_t n, const uint64_t *slot_of,
                                               const uint32_t *map, const uint8_t *ue, Keep keep)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) table_mark_written(t);
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const uint32_t e = ue[i];
    if (!e || !keep(i)) continue;
    const uint64_t slot = slot_of[i];
    const Kmer<W> key = cl_key<W>(t, slot);
    uint32_t mask = e;
    for (uint32_t b = 0; b < 8; b++) {
      if (!((e >> b) & 1u)) continue;
      uint32_t p = 0;
      const uint64_t s = cl_next<W>(t, key, b >> 2, b & 3u, k, p);
      if (s == kNoSlot || !keep(map[s])) mask &= ~(1u << b);
    }
    if (mask == e) continue;
    for (uint32_t c = 0; c < ncols; c++) {
      uint64_t *v = val_ptr(t, slot, c);
      const uint64_t x = *v;
      *v = (x & ~0xffULL) | (x & mask);
    }
  }
}

// prune_nodes_lacking_flag_no_edges: the slot becomes a tombstone as in k_intersect_finish
template <class Keep>
__device__ __forceinline__ void cl_tombstone(const TableView &t, uint64_t n, const uint64_t *slot_of, Keep keep, Counters *ctr,
                                             unsigned long long *removed)
{
  unsigned long long gone = 0;
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    if (keep(i)) continue;
    key_ptr(t, slot_of[i])[0] = kPending;
    gone++;
  }
  block_add(removed, gone);
  block_add(&ctr->novel, 0ULL - gone);
}

template <int W>
__global__ __launch_bounds__(256) void k_cl_prune_edges(TableView t, int k, uint32_t ncols, uint64_t n, const uint64_t *slot_of,
                                                        const uint32_t *map, const uint8_t *ue, const uint32_t *uid,
                                                        const uint8_t *keep)
{
  cl_prune_edges<W>(t, k, ncols, n, slot_of, map, ue, KeepUnitig{uid, keep});
}

__global__ __launch_bounds__(256) void k_cl_tombstone(TableView t, uint64_t n, const uint64_t *slot_of, const uint32_t *uid,
                                                      const uint8_t *keep, Counters *ctr, unsigned long long *removed)
{
  cl_tombstone(t, n, slot_of, KeepUnitig{uid, keep}, ctr, removed);
}

}  // namespace mcx
