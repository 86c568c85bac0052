// mcx_bubbles.h -- `bubbles` on the device (included by mcx_api.hip behind mcx_contigs.h).
//
// ctx_bubbles.c without link files: from every fork a walk per colour and branch over unitigs (graph_crawler.c), the
// per-fork cache of graph_cache.c, the candidates and filters of bubble_caller.c and the call text of print_bubble.
// include/mcx_gpu.h restates the semantics; tests/bubbles_restate.py is the same in Python.  The graph view is that of
// `correct`: union edges, in a sample iff the value word of the colour is non-zero, AN EDGE THAT NAMES AN ABSENT K-MER
// COUNTS AS NO EDGE.  Everything runs on the decomposition that mcx_graph_unitig_stats keeps and on what `unitigs`'
// passes A and B leave (unitigs_prepare): per k-mer its unitig number, per unitig its oriented first and last node,
// its length and its place in the base array.  A step of a walk is a jump over one of those unitigs.
// The passes ("bubbles' device passes"):
//   F. k_bb_forks, a scan, k_bb_forklist and sort_perm_by_words: the k-mers with a fork on either side in ascending key
//      order; item 2 f + o is fork k-mer f taken in orientation o (an item whose side does not fork is empty)
//      k_bb_hap: per unitig and haploid colour, whether every k-mer of the unitig is in that colour
//   Per batch of "bubbles_batch" fork k-mers:
//   W. k_bb_walk<COUNT>, a scan, k_bb_walk<WRITE>: path p = (item, colour, base) has four lanes, one successor candidate
//      each.  The counting pass walks without the repeat rule, which can only make a path longer, and so bounds every
//      path's steps (max_allele at the most); the scan places the paths in the step pool; the writing pass stores the
//      steps (unitig number << 1 | orientation), step n by lane n % 4, which alone reads it back for the repeat rule.
//      A LINK STORE WOULD DECIDE WHERE bb_choose RETURNS kBbNoLinks.
//   G. k_bb_first: a thread per path; per step the fork-local word (pool position of the unitig's first step in the
//      fork << 1 | orientation: the local ids of graph_cache_new_step in another numbering of the same order) and the
//      position of the path's first step
//      k_bb_group<COUNT>, two scans, k_bb_group<WRITE>: a thread per item; the candidates in local id order, FORWARD
//      then REVERSE, newest step first, and the four filters; calls and their branch lists at the scanned offsets
//   S. k_bb_size: a thread per call: the record and the text length; a scan gives 64-bit text offsets
//   T. k_bb_emit: driven by the output: a thread per byte of the requested range finds its call by binary search in
//      the offsets and works out the byte (bb_char) from the base array and offsets of `unitigs`' pass B.  Any byte
//      range of the text can be produced, so a chunk seam may fall anywhere.
// All are grid-stride loops (the "grid" knob caps the launches); the table is only read.  Per batch the scratch is the
// step pool (four 32-bit words per bounded step) and the calls.  The group pass is quadratic in a fork's steps.
#pragma once
#include "mcx_unitigs.h"

namespace mcx {

enum : uint32_t { kBbForks = 0, kBbPaths, kBbSteps, kBbLimit, kBbNoCovg, kBbNoColCovg, kBbNoLinks, kBbRepeat, kBbCands, kBbBubbles, kBbBranches, kBbHaploid,
                  kBbSerial, kBbNStats };
constexpr uint32_t kBbKeepSerial = 1;  // = MCX_BUBBLES_KEEP_SERIAL
constexpr uint32_t kBbMaxHaploid = 64;

struct BbGraph {  // the table, the decomposition and what unitigs' passes A and B leave
  TableView t;
  int k, W;
  uint32_t ncols;
  uint64_t n;
  const uint64_t *slot_of;
  const uint32_t *map, *kun, *ufirst, *ulast, *ulen, *ubase;
  const uint8_t *ue, *bases;
};
struct BbCall {
  uint64_t base, broff;  // pool position of the fork's first step; where the branch list starts
  uint32_t item, end0, nbr, pad;
};

// successor of the oriented node v (2 * dense id + orientation) over base x: the oriented node and its slot, kClNone
// when there is no such edge or it names an absent k-mer
template <int W> __device__ __forceinline__ uint32_t bb_succ(const BbGraph &a, uint32_t v, uint32_t x, bool on, uint64_t &slot)
{
  slot = kNoSlot;
  if (!on) return kClNone;
  const uint32_t i = v >> 1, o = v & 1u;
  if (!((a.ue[i] >> (4u * o + x)) & 1u)) return kClNone;
  uint32_t p = 0;
  slot = cl_next<W>(a.t, cl_key<W>(a.t, a.slot_of[i]), o, x, a.k, p);
  return slot == kNoSlot ? kClNone : 2u * a.map[slot] + p;
}
// the step that enters node v: unitig number << 1 | orientation (gc_unitig_get_orient: FORWARD iff v is the normalised
// unitig's first node; a single k-mer is normalised forward)
__device__ __forceinline__ uint32_t bb_word(const BbGraph &a, uint32_t v)
{
  const uint32_t j = a.kun[v >> 1];
  return j << 1 | (v == a.ufirst[j] ? 0u : 1u);
}
// graph_walker_choose:385-433 over the successors that exist (F) and those in the colour (S): the choice, or the stop
__device__ __forceinline__ uint32_t bb_choose(uint32_t F, uint32_t S, uint32_t &choice)
{
  choice = 0;
  if (!F) return kBbNoCovg;
  if (!(F & (F - 1u))) { choice = (uint32_t)__builtin_ctz(F); return 0; }  // COLFWD or POPFWD
  if (!S) return kBbNoColCovg;
  if (!(S & (S - 1u))) { choice = (uint32_t)__builtin_ctz(S); return 0; }  // POPFRK_COLFWD
  return kBbNoLinks;  // (held links would choose here)
}

// F. fmask[i] bit o: side o of k-mer i has more than one successor that is a key; flag[i] = fmask[i] != 0, flag[n] = 0
template <int W> __global__ __launch_bounds__(256) void k_bb_forks(BbGraph a, uint8_t *flag, uint8_t *fmask, unsigned long long *stats)
{
  unsigned long long nf = 0;
  for (uint64_t i = cl_first(); i <= a.n; i += cl_stride()) {
    if (i == a.n) { flag[i] = 0; continue; }
    uint32_t mask = 0;
    for (uint32_t o = 0; o < 2; o++) {
      if (cl_outdeg(a.ue[i], o) < 2) continue;
      uint32_t cnt = 0;
      for (uint32_t x = 0; x < 4; x++) {
        uint64_t s;
        cnt += bb_succ<W>(a, (uint32_t)(2 * i + o), x, true, s) != kClNone;
      }
      if (cnt > 1) { mask |= 1u << o; nf++; }
    }
    fmask[i] = (uint8_t)mask;
    flag[i] = mask != 0;
  }
  block_add(&stats[kBbForks], nf);
}
__global__ __launch_bounds__(256) void k_bb_forklist(const uint8_t *flag, const uint64_t *ex, uint64_t n, uint64_t *list)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride())
    if (flag[i]) list[ex[i]] = i;
}
// uhap[j * nhap + r] (1 before): cleared when a k-mer of unitig j is not in haploid colour r
__global__ __launch_bounds__(256) void k_bb_hap(BbGraph a, const uint32_t *hap, uint32_t nhap, uint8_t *uhap)
{
  for (uint64_t i = cl_first(); i < a.n; i += cl_stride())
    for (uint32_t r = 0; r < nhap; r++)
      if (*val_ptr(a.t, a.slot_of[i], hap[r]) == 0) uhap[(uint64_t)a.kun[i] * nhap + r] = 0;
}

struct BbWalk {
  const uint64_t *forks;  // the batch's fork k-mers (dense ids) in key order
  const uint8_t *fmask;
  uint64_t nitems;
  uint32_t max_allele;
  uint64_t *cap;         // COUNT: the bound of every path's steps
  const uint64_t *poff;  // WRITE: where the path starts in the pool
  uint32_t *plen, *steps;
  unsigned long long *stats;
};

// W. Four lanes per path.  One round of the loop is one step of graph_crawler_load_path: the step, the limit
// (gcrawler_load_path_limit_kmer_len), the choice at the unitig's far end and, in the writing pass, the repeat rule.
template <int W, bool WRITE> __device__ __forceinline__ void bb_walk(const BbGraph &a, const BbWalk &w)
{
  const uint32_t lane = threadIdx.x & 63u, sub = lane & 3u, g0 = lane & ~3u;
  const uint64_t per_block = blockDim.x >> 2, PC = 4ull * a.ncols, npaths = w.nitems * PC;
  unsigned long long c[kBbNStats];
  for (uint32_t i = 0; i < kBbNStats; i++) c[i] = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < npaths; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t p = base + (threadIdx.x >> 2);
    const bool mine = p < npaths;
    bool live = mine;
    uint32_t colour = 0, fork = 0;
    if (live) {
      const uint64_t item = p / PC;
      colour = (uint32_t)((p >> 2) % a.ncols);
      const uint32_t fi = (uint32_t)w.forks[item >> 1], fo = (uint32_t)(item & 1u);
      fork = 2u * fi + fo;
      live = ((w.fmask[fi] >> fo) & 1u) && *val_ptr(a.t, a.slot_of[fi], colour) != 0;  // the colour holds the fork node
    }
    uint64_t slot;
    uint32_t node = bb_succ<W>(a, fork, (uint32_t)(p & 3u), live, slot);  // (the four lanes alike)
    live = live && node != kClNone && *val_ptr(a.t, slot, colour) != 0;
    const uint64_t off = (WRITE && mine) ? w.poff[p] : 0;
    uint32_t ns = 0;
    uint64_t total = 0;
    if (live && sub == 0) c[kBbPaths]++;
    while (__builtin_amdgcn_ballot_w64(live)) {  // (the same for the whole wave: the votes cross lanes)
      uint32_t endnode = 0;
      if (live) {
        const uint32_t word = bb_word(a, node), j = word >> 1;
        if (WRITE && sub == (ns & 3u)) w.steps[off + ns] = word;
        ns++;
        total += a.ulen[j];
        if (sub == 0) c[kBbSteps]++;
        endnode = (word & 1u) ? (a.ufirst[j] ^ 1u) : a.ulast[j];
        if (total >= w.max_allele) {  // the step that crosses the limit stays
          live = false;
          if (sub == 0) c[kBbLimit]++;
        }
      }
      uint64_t nslot;
      const uint32_t cand = bb_succ<W>(a, endnode, sub, live, nslot);
      const bool ins = cand != kClNone && *val_ptr(a.t, nslot, colour) != 0;
      const uint32_t F = (uint32_t)(__builtin_amdgcn_ballot_w64(cand != kClNone) >> g0) & 15u;
      const uint32_t S = (uint32_t)(__builtin_amdgcn_ballot_w64(ins) >> g0) & 15u;
      uint32_t choice = 0;
      const uint32_t cause = bb_choose(F, S, choice);
      const uint32_t next = (uint32_t)__shfl((int)cand, (int)(g0 + choice));
      if (live && cause) {
        live = false;
        if (sub == 0) c[cause]++;
      }
      if (WRITE) {  // rpt_walker_attempt_traverse: the entries so far are the steps behind the first
        uint32_t cnt = 0;
        if (live) {
          const uint32_t word = bb_word(a, next);
          for (uint32_t i = sub ? sub : 4u; i < ns; i += 4)
            if (w.steps[off + i] == word) cnt++;
        }
        cnt += __shfl_xor(cnt, 1);
        cnt += __shfl_xor(cnt, 2);
        if (live && cnt >= 2u) {  // the third entry
          live = false;
          if (sub == 0) c[kBbRepeat]++;
        }
      }
      if (live) node = next;
    }
    if (mine && sub == 0) {
      if (WRITE) w.plen[p] = ns;
      else w.cap[p] = ns;
    }
  }
  if (WRITE)
    for (uint32_t i = kBbPaths; i <= kBbRepeat; i++) block_add(&w.stats[i], c[i]);
}

template <int W> __global__ __launch_bounds__(256) void k_bb_walk_count(BbGraph a, BbWalk w) { bb_walk<W, false>(a, w); }
template <int W> __global__ __launch_bounds__(256) void k_bb_walk_write(BbGraph a, BbWalk w) { bb_walk<W, true>(a, w); }

// G. a thread per path: lw = the fork-local word of every step, sfirst = the path's first step (both relative to the
// fork's first pool position)
__global__ __launch_bounds__(256) void k_bb_first(uint64_t npaths, uint32_t PC, const uint64_t *poff, const uint32_t *plen, const uint32_t *steps, uint32_t *lw,
                                                  uint32_t *sfirst)
{
  for (uint64_t p = cl_first(); p < npaths; p += cl_stride()) {
    const uint64_t p0 = p - p % PC, base = poff[p0], mine = poff[p];
    for (uint32_t s = 0; s < plen[p]; s++) {
      const uint32_t word = steps[mine + s], u = word >> 1;
      uint64_t fo = mine + s;
      bool found = false;
      for (uint64_t pp = p0; pp <= p && !found; pp++) {
        const uint32_t lim = pp == p ? s : plen[pp];
        for (uint32_t ss = 0; ss < lim; ss++)
          if ((steps[poff[pp] + ss] >> 1) == u) { fo = poff[pp] + ss; found = true; break; }
      }
      lw[mine + s] = (uint32_t)(fo - base) << 1 | (word & 1u);
      sfirst[mine + s] = (uint32_t)(mine - base);
    }
  }
}

struct BbGroup {
  uint64_t nitems;
  uint32_t PC, flags, nhap;
  const uint64_t *poff;
  const uint32_t *plen, *steps, *lw, *sfirst;
  uint32_t *scr;  // as large as the pool: an item sorts its candidate in its own range
  const uint8_t *uhap;
  uint64_t *ncall, *nbr;        // COUNT: per item
  const uint64_t *coff, *boff;  // WRITE: the scans of those
  BbCall *calls;
  uint32_t *brs;
  unsigned long long *stats;
};

// graph_cache_steps_cmp: the words along both paths up to and including the steps, then the lengths
__device__ __forceinline__ int bb_cmp(const uint32_t *lw, const uint32_t *sfirst, uint32_t a, uint32_t b)
{
  const uint32_t fa = sfirst[a], fb = sfirst[b], la = a - fa + 1u, lb = b - fb + 1u, m = la < lb ? la : lb;
  for (uint32_t i = 0; i < m; i++) {
    const uint32_t wa = lw[fa + i], wb = lw[fb + i];
    if (wa != wb) return wa < wb ? -1 : 1;
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}

// a thread per item (write_bubbles_to_file, find_bubbles_ending_with, filter_bubbles).  Positions are relative to the
// item's first pool position, where lw, sfirst, steps and scr are viewed from.
template <bool WRITE> __global__ __launch_bounds__(256) void k_bb_group(BbGroup a)
{
  unsigned long long c_cand = 0, c_bub = 0, c_br = 0, c_hap = 0, c_ser = 0;
  for (uint64_t item = cl_first(); item < a.nitems; item += cl_stride()) {
    const uint64_t p0 = item * a.PC, base = a.poff[p0];
    const uint32_t *lw = a.lw + base, *sfirst = a.sfirst + base, *steps = a.steps + base;
    uint32_t *e = a.scr + base;
    uint64_t ncall = 0, nbr = 0;
    for (uint32_t pp = 0; pp < a.PC; pp++) {
      const uint32_t at = (uint32_t)(a.poff[p0 + pp] - base);
      for (uint32_t ss = 0; ss < a.plen[p0 + pp]; ss++) {
        const uint32_t q = at + ss;
        if ((lw[q] >> 1) != q) continue;  // not the unitig's first step: its candidates are done
        for (uint32_t orient = 0; orient < 2; orient++) {
          const uint32_t word = q << 1 | orient;
          uint32_t n = 0;  // the steps on the unitig this way round, newest first
          for (uint32_t p2 = a.PC; p2-- > pp;) {
            const uint32_t at2 = (uint32_t)(a.poff[p0 + p2] - base);
            for (uint32_t s2 = a.plen[p0 + p2]; s2-- > 0;)
              if (lw[at2 + s2] == word) e[n++] = at2 + s2;
          }
          if (n < 2) continue;
          c_cand++;
          // graph_cache_is_3p_flank
          const uint32_t w0 = lw[sfirst[e[0]]];
          bool differ = false;
          for (uint32_t i = 1; i < n && !differ; i++) differ = lw[sfirst[e[i]]] != w0;
          if (!differ) continue;
          const bool none0 = e[0] == sfirst[e[0]];
          const uint32_t pw0 = none0 ? 0u : lw[e[0] - 1u];
          differ = false;
          for (uint32_t i = 1; i < n && !differ; i++) {
            const bool none = e[i] == sfirst[e[i]];
            differ = none0 ? !none : (none || lw[e[i] - 1u] != pw0);
          }
          if (!differ) continue;
          // graph_cache_remove_dupes
          for (uint32_t i = 1; i < n; i++) {
            const uint32_t x = e[i];
            uint32_t j = i;
            for (; j > 0 && bb_cmp(lw, sfirst, e[j - 1], x) > 0; j--) e[j] = e[j - 1];
            e[j] = x;
          }
          uint32_t m = 0;
          for (uint32_t i = 0; i + 1 < n; i++)
            if (bb_cmp(lw, sfirst, e[i], e[i + 1]) != 0) e[m++] = e[i];
          e[m++] = e[n - 1];
          if (m < 2) continue;
          // remove_haploid_paths
          if (a.nhap) {
            uint64_t seen = 0;
            for (uint32_t p = 0; p < m;) {
              uint32_t r = 0;
              for (; r < a.nhap; r++) {
                bool has = true;
                for (uint32_t s = sfirst[e[p]]; s <= e[p] && has; s++) has = a.uhap[(uint64_t)(steps[s] >> 1) * a.nhap + r] != 0;
                if (!has) continue;
                if ((seen >> r) & 1ull) break;
                seen |= 1ull << r;
              }
              if (r < a.nhap) {
                const uint32_t x = e[p];
                e[p] = e[m - 1];
                e[m - 1] = x;
                m--;
              } else p++;
            }
            if (m < 2) { c_hap++; continue; }
          }
          // paths_all_share_unitig
          if (!(a.flags & kBbKeepSerial)) {
            bool shared = false;
            for (uint32_t i = 0; i < m && !shared; i++)
              for (uint32_t s = sfirst[e[i]]; s < e[i] && !shared; s++) {
                uint32_t cnt = 0;
                for (uint32_t i2 = 0; i2 < m; i2++)
                  for (uint32_t s2 = sfirst[e[i2]]; s2 < e[i2]; s2++) cnt += lw[s2] == lw[s];
                shared = cnt == m;
              }
            if (shared) { c_ser++; continue; }
          }
          if (WRITE) {
            const uint64_t bo = a.boff[item] + nbr;
            a.calls[a.coff[item] + ncall] = BbCall{base, bo, (uint32_t)item, e[0], m, 0u};
            for (uint32_t i = 0; i < m; i++) a.brs[bo + i] = e[i];
          }
          ncall++;
          nbr += m;
          c_bub++;
          c_br += m;
        }
      }
    }
    if (!WRITE) { a.ncall[item] = ncall; a.nbr[item] = nbr; }
  }
  if (WRITE) {
    block_add(&a.stats[kBbCands], c_cand);
    block_add(&a.stats[kBbBubbles], c_bub);
    block_add(&a.stats[kBbBranches], c_br);
    block_add(&a.stats[kBbHaploid], c_hap);
    block_add(&a.stats[kBbSerial], c_ser);
  }
}

// ---- text ------------------------------------------------------------------------------------------------------------
struct BbText {
  BbGraph g;
  const uint64_t *forks;
  uint64_t id0, ncalls;  // the batch's first call id
  uint32_t max_flank;
  const BbCall *calls;
  const uint32_t *brs, *steps, *sfirst;
  const uint64_t *toff;
};
__host__ __device__ __forceinline__ uint32_t bb_digits(uint64_t x)
{
  uint32_t d = 1;
  while (x >= 10) { x /= 10; d++; }
  return d;
}
__device__ __forceinline__ char bb_digit(uint64_t x, uint32_t nd, uint32_t at)
{
  for (uint32_t i = at + 1; i < nd; i++) x /= 10;
  return (char)('0' + x % 10);
}
__device__ __forceinline__ char bb_comp(char ch) { return ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : 'A'; }
// base P of the sequence of normalised unitig j
__device__ __forceinline__ char bb_useq(const BbGraph &a, uint32_t j, uint64_t P)
{
  const uint32_t k1 = (uint32_t)(a.k - 1);
  if (P >= k1) return (char)a.bases[(uint64_t)a.ubase[j] + P - k1];
  const uint32_t h = a.ufirst[j], b = (h & 1u) ? k1 - (uint32_t)P : (uint32_t)P, bit = 2u * (k1 - b);
  const uint32_t nuc = (uint32_t)(key_ptr(a.t, a.slot_of[h >> 1])[a.W - 1 - (int)(bit >> 6)] >> (bit & 63u)) & 3u;
  return "ACGT"[(h & 1u) ? 3u - nuc : nuc];
}
// the last base of node s of the step `word` (the unitig read in the step's orientation)
__device__ __forceinline__ char bb_step_char(const BbGraph &a, uint32_t word, uint64_t s)
{
  const uint32_t j = word >> 1;
  if (!(word & 1u)) return (char)a.bases[(uint64_t)a.ubase[j] + s];
  return bb_comp(bb_useq(a, j, (uint64_t)a.ulen[j] - 1u - s));
}
// `>bubble.call<id>.5pflank kmers=<n>\n` (which 0), `.3pflank` (1), `.branch.<b> kmers=<n>\n` (2)
__device__ __forceinline__ uint32_t bb_hdr_len(uint64_t id, uint32_t which, uint32_t b, uint64_t n)
{
  return 12u + bb_digits(id) + (which < 2u ? 15u : 8u + bb_digits(b) + 7u) + bb_digits(n) + 1u;
}
__device__ char bb_hdr_char(uint64_t id, uint32_t which, uint32_t b, uint64_t n, uint32_t c)
{
  if (c < 12u) return ">bubble.call"[c];
  c -= 12u;
  const uint32_t di = bb_digits(id);
  if (c < di) return bb_digit(id, di, c);
  c -= di;
  if (which < 2u) {
    if (c < 15u) return (which ? ".3pflank kmers=" : ".5pflank kmers=")[c];
    c -= 15u;
  } else {
    if (c < 8u) return ".branch."[c];
    c -= 8u;
    const uint32_t db = bb_digits(b);
    if (c < db) return bb_digit(b, db, c);
    c -= db;
    if (c < 7u) return " kmers="[c];
    c -= 7u;
  }
  const uint32_t dn = bb_digits(n);
  return c < dn ? bb_digit(n, dn, c) : '\n';
}
// k-mers of the steps [from, to) of a path
__device__ __forceinline__ uint64_t bb_kmers(const BbGraph &a, const uint32_t *steps, uint32_t from, uint32_t to)
{
  uint64_t n = 0;
  for (uint32_t s = from; s < to; s++) n += a.ulen[steps[s] >> 1];
  return n;
}
// the k-mers of the 5' flank: db_unitig_extend from the reversed fork node, max_flank k-mers at the most
__device__ __forceinline__ uint32_t bb_flank5(const BbText &x, uint32_t fork)
{
  const uint32_t L = x.g.ulen[x.g.kun[fork >> 1]];
  return L < x.max_flank ? L : x.max_flank;
}
__device__ __forceinline__ uint32_t bb_fork(const BbText &x, const BbCall &c) { return 2u * (uint32_t)x.forks[c.item >> 1] + (c.item & 1u); }

// S. a thread per call: the record and the length of its text; text_off holds the call's id until k_bb_offsets
__global__ __launch_bounds__(256) void k_bb_size(BbText x, mcx_bubble_rec *recs, uint64_t *tlen)
{
  const BbGraph &a = x.g;
  for (uint64_t r = cl_first(); r <= x.ncalls; r += cl_stride()) {
    if (r == x.ncalls) { tlen[r] = 0; continue; }
    const BbCall c = x.calls[r];
    const uint64_t id = x.id0 + r;
    const uint32_t *steps = x.steps + c.base, *sfirst = x.sfirst + c.base;
    const uint32_t fork = bb_fork(x, c), n5 = bb_flank5(x, fork), n3 = a.ulen[steps[c.end0] >> 1];
    uint64_t len = (uint64_t)bb_hdr_len(id, 0, 0, n5) + (uint64_t)a.k + n5 + bb_hdr_len(id, 1, 0, n3) + n3 + 1u;
    for (uint32_t b = 0; b < c.nbr; b++) {
      const uint32_t e = x.brs[c.broff + b];
      const uint64_t nb = bb_kmers(a, steps, sfirst[e], e);
      len += (uint64_t)bb_hdr_len(id, 2, b, nb) + nb + 1u;
    }
    len += 1u;
    tlen[r] = len;
    mcx_bubble_rec R;
    const uint64_t *key = key_ptr(a.t, a.slot_of[fork >> 1]);
    for (int i = 0; i < 4; i++) R.fork_key[i] = i < a.W ? (i ? key[i] : (key[0] & kKeyMask)) : 0ull;
    R.text_off = 0;
    R.text_len = len;
    R.fork_orient = fork & 1u;
    R.num_branches = c.nbr;
    R.flank5p_kmers = n5;
    R.flank3p_kmers = n3;
    recs[r] = R;
  }
}
__global__ __launch_bounds__(256) void k_bb_offsets(uint64_t ncalls, const uint64_t *toff, uint64_t text_base, mcx_bubble_rec *recs)
{
  for (uint64_t r = cl_first(); r < ncalls; r += cl_stride()) recs[r].text_off = text_base + toff[r];
}

// byte q of the text of call r
__device__ char bb_char(const BbText &x, uint64_t r, uint64_t q)
{
  const BbGraph &a = x.g;
  const BbCall c = x.calls[r];
  const uint64_t id = x.id0 + r;
  const uint32_t *steps = x.steps + c.base, *sfirst = x.sfirst + c.base;
  const uint32_t fork = bb_fork(x, c), n5 = bb_flank5(x, fork);
  uint64_t len = bb_hdr_len(id, 0, 0, n5);
  if (q < len) return bb_hdr_char(id, 0, 0, n5, (uint32_t)q);
  q -= len;
  len = (uint64_t)a.k - 1u + n5;
  if (q < len) {  // the unitig of the fork node, read so that it ends there: its last n5 k-mers
    const uint32_t j = a.kun[fork >> 1];
    if (fork == a.ulast[j]) return bb_useq(a, j, (uint64_t)a.ulen[j] - n5 + q);
    return bb_comp(bb_useq(a, j, len - 1u - q));
  }
  if (q == len) return '\n';
  q -= len + 1u;
  const uint32_t w3 = steps[c.end0], n3 = a.ulen[w3 >> 1];
  len = bb_hdr_len(id, 1, 0, n3);
  if (q < len) return bb_hdr_char(id, 1, 0, n3, (uint32_t)q);
  q -= len;
  if (q < n3) return bb_step_char(a, w3, q);
  if (q == n3) return '\n';
  q -= (uint64_t)n3 + 1u;
  for (uint32_t b = 0; b < c.nbr; b++) {
    const uint32_t e = x.brs[c.broff + b];
    const uint64_t nb = bb_kmers(a, steps, sfirst[e], e);
    len = bb_hdr_len(id, 2, b, nb);
    if (q < len) return bb_hdr_char(id, 2, b, nb, (uint32_t)q);
    q -= len;
    if (q < nb) {
      for (uint32_t s = sfirst[e]; s < e; s++) {
        const uint32_t L = a.ulen[steps[s] >> 1];
        if (q < L) return bb_step_char(a, steps[s], q);
        q -= L;
      }
      return '?';  // (never: nb is the sum of those lengths)
    }
    if (q == nb) return '\n';
    q -= nb + 1u;
  }
  return '\n';  // the blank line
}

// T. bytes [p0, p0 + cnt) of the batch's text go to dst[0 .. cnt).  cnt > 0.
__global__ __launch_bounds__(256) void k_bb_emit(BbText x, uint64_t p0, uint64_t cnt, uint8_t *dst)
{
  for (uint64_t i = cl_first(); i < cnt; i += cl_stride()) {
    const uint64_t p = p0 + i, r = un_find(x.toff, 0, x.ncalls - 1, p);
    dst[i] = (uint8_t)bb_char(x, r, p - x.toff[r]);
  }
}

}  // namespace mcx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" int mcx_graph_bubbles(mcx_graph *g, const mcx_bubbles_params *p, mcx_sink_fn rec_sink, void *rec_ctx, mcx_sink_fn text_sink, void *text_ctx,
                                 mcx_bubbles_stats *stats)
{
  int rc = whole_table_only(g, "bubbles", " (unitigs cross shards)");
  if (rc != MCX_OK) return rc;
  if (!p) return fail(MCX_ERR_ARG, "bubbles: null parameters");
  if (!p->max_allele || !p->max_flank) return fail(MCX_ERR_ARG, "bubbles: max_allele and max_flank must be above 0");
  if (p->flags & ~(uint32_t)MCX_BUBBLES_KEEP_SERIAL) return fail(MCX_ERR_ARG, "bubbles: unknown flags 0x%x", p->flags);
  if (p->nhaploid && !p->haploid) return fail(MCX_ERR_ARG, "bubbles: null haploid colours");
  if (p->nhaploid > kBbMaxHaploid) return fail(MCX_ERR_ARG, "bubbles: %u haploid colours (%u at the most)", p->nhaploid, kBbMaxHaploid);
  for (uint32_t i = 0; i < p->nhaploid; i++)
    if (p->haploid[i] >= (uint32_t)g->ncols) return fail(MCX_ERR_ARG, "bubbles: haploid colour %u is not one of the graph's %d", p->haploid[i], g->ncols);
  const uint64_t PC = 4ull * (uint64_t)g->ncols;
  if (PC * p->max_allele >= (1ull << 31)) return fail(MCX_ERR_ARG, "bubbles: 4 x colours x max_allele must stay below 2^31");
  UnWork w;
  if ((rc = unitigs_prepare(g, -1, w)) != MCX_OK) return rc;
  if ((rc = ensure_stage(g)) != MCX_OK) return rc;
  hipStream_t st = g->stream;
  HIP_TRY(hipStreamSynchronize(st));  // the staging buffers are ours now
  HIP_TRY(hipStreamSynchronize(g->cstream));
  if (!w.n) return MCX_OK;
  const CleanCache *c = g->clean;
  const uint64_t n = w.n;
  const uint32_t nhap = p->nhaploid;
  const BbGraph G{g->t, g->k, g->W, (uint32_t)g->ncols, n, c->slot_of.p, c->map.p, w.kun.p, w.ufirst.p, w.ulast.p, w.ulen.p, w.ubase.p, c->ue.p, w.bases.p};
  const uint64_t B = std::max<uint64_t>(1, std::min<uint64_t>(g->bubbles_batch ? g->bubbles_batch : 65536, 1u << 20));  // fork k-mers per round
  uint64_t chunk = std::min<uint64_t>(kStageBytes, g->stage_alloc) & ~15ull;
  if (g->bubbles_chunk) chunk = std::min<uint64_t>(chunk, g->bubbles_chunk);
  DevBuf<unsigned long long> d_stats;
  DevBuf<uint8_t> flag, fmask, tmp, uhap;
  DevBuf<uint64_t> ex, l0, l1, k0, k1, cap, poff, ncall, nbr, coff, boff;
  DevBuf<uint32_t> d_hap, plen;
  uint64_t *forks = nullptr, m = 0, text_base = 0, id0 = 0;
  double t0 = now_s();

  // F. the fork k-mers in key order
  auto fork_list = [&]() -> int {
    int rc2;
    HIP_TRY(d_stats.alloc(kBbNStats));
    HIP_TRY(hipMemsetAsync(d_stats.p, 0, kBbNStats * 8, st));
    HIP_TRY(flag.alloc(n + 1));
    HIP_TRY(fmask.alloc(n));
    HIP_TRY(ex.alloc(n + 1));
    GRID_LAUNCH_W(k_bb_forks, n + 1, G, flag.p, fmask.p, d_stats.p);
    if ((rc2 = scan_total(st, (const uint8_t *)flag.p, ex.p, n + 1, &m)) != MCX_OK) return rc2;
    if (!m) return MCX_OK;
    HIP_TRY(l0.alloc(m));
    HIP_TRY(l1.alloc(m));
    HIP_TRY(k0.alloc(m));
    HIP_TRY(k1.alloc(m));
    GRID_LAUNCH(k_bb_forklist, n, (const uint8_t *)flag.p, (const uint64_t *)ex.p, n, l0.p);
    size_t tmp_bytes = 0;
    if ((rc2 = sort_perm_scratch(st, m, &tmp_bytes)) != MCX_OK) return rc2;
    HIP_TRY(tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    uint64_t *const keys[2] = {k0.p, k1.p}, *const perm[2] = {l0.p, l1.p};
    auto word = [&](int wd, bool, const uint64_t *through, uint64_t *dst, const uint64_t **) -> int {
      GRID_LAUNCH(k_un_keyword, m, g->t, m, (const uint64_t *)c->slot_of.p, through, (uint32_t)wd, dst);
      return MCX_OK;
    };
    if ((rc2 = sort_perm_by_words(st, m, g->W, 2 * g->k - 64 * (g->W - 1), keys, perm, tmp.p, tmp_bytes, g, word, &forks)) != MCX_OK) return rc2;
    if (nhap) {
      HIP_TRY(uhap.alloc(w.nu * nhap));
      HIP_TRY(d_hap.alloc(nhap));
      HIP_TRY(hipMemsetAsync(uhap.p, 1, w.nu * nhap, st));
      HIP_TRY(hipMemcpyAsync(d_hap.p, p->haploid, nhap * 4, hipMemcpyHostToDevice, st));
      GRID_LAUNCH(k_bb_hap, n, G, (const uint32_t *)d_hap.p, nhap, uhap.p);
    }
    const uint64_t maxitems = 2 * std::min(B, m);
    HIP_TRY(cap.alloc(maxitems * PC + 1));
    HIP_TRY(poff.alloc(maxitems * PC + 1));
    HIP_TRY(plen.alloc(maxitems * PC));
    HIP_TRY(ncall.alloc(maxitems + 1));
    HIP_TRY(nbr.alloc(maxitems + 1));
    HIP_TRY(coff.alloc(maxitems + 1));
    HIP_TRY(boff.alloc(maxitems + 1));
    HIP_TRY(hipStreamSynchronize(st));
    return MCX_OK;
  };

  // one batch: the fork k-mers [f0, f0 + nf)
  auto batch = [&](uint64_t f0, uint64_t nf) -> int {
    int rc2;
    const uint64_t nitems = 2 * nf, npaths = nitems * PC;
    uint64_t pool = 0, ncalls = 0, nbrs = 0, total = 0;
    DevBuf<uint32_t> steps, lw, sfirst, scr, brs;
    DevBuf<BbCall> calls;
    DevBuf<mcx_bubble_rec> recs;
    DevBuf<uint64_t> tlen, toff;
    // W.
    BbWalk W{forks + f0, fmask.p, nitems, p->max_allele, cap.p, poff.p, plen.p, nullptr, d_stats.p};
    HIP_TRY(hipMemsetAsync(cap.p + npaths, 0, 8, st));
    GRID_LAUNCH_W(k_bb_walk_count, npaths * 4, G, W);
    if ((rc2 = scan_total(st, (const uint64_t *)cap.p, poff.p, npaths + 1, &pool)) != MCX_OK) return rc2;
    if (steps.alloc(pool + 1) != hipSuccess || lw.alloc(pool + 1) != hipSuccess || sfirst.alloc(pool + 1) != hipSuccess || scr.alloc(pool + 1) != hipSuccess) {
      (void)hipGetLastError();
      return fail(MCX_ERR_NOMEM, "bubbles: no room for the %llu steps of %llu forks (a smaller bubbles_batch needs less)", (unsigned long long)pool,
                  (unsigned long long)nitems);
    }
    W.steps = steps.p;
    GRID_LAUNCH_W(k_bb_walk_write, npaths * 4, G, W);
    // G.
    GRID_LAUNCH(k_bb_first, npaths, npaths, (uint32_t)PC, (const uint64_t *)poff.p, (const uint32_t *)plen.p, (const uint32_t *)steps.p, lw.p, sfirst.p);
    BbGroup R{nitems, (uint32_t)PC, p->flags, nhap, poff.p, plen.p, steps.p, lw.p, sfirst.p, scr.p, uhap.p, ncall.p, nbr.p, coff.p, boff.p, nullptr, nullptr, d_stats.p};
    HIP_TRY(hipMemsetAsync(ncall.p + nitems, 0, 8, st));
    HIP_TRY(hipMemsetAsync(nbr.p + nitems, 0, 8, st));
    GRID_LAUNCH(k_bb_group<false>, nitems, R);
    if ((rc2 = scan_total(st, (const uint64_t *)ncall.p, coff.p, nitems + 1, &ncalls)) != MCX_OK) return rc2;
    if ((rc2 = scan_total(st, (const uint64_t *)nbr.p, boff.p, nitems + 1, &nbrs)) != MCX_OK) return rc2;
    HIP_TRY(calls.alloc(ncalls + 1));
    HIP_TRY(brs.alloc(nbrs + 1));
    R.calls = calls.p;
    R.brs = brs.p;
    GRID_LAUNCH(k_bb_group<true>, nitems, R);
    if (!ncalls) {
      HIP_TRY(hipStreamSynchronize(st));
      return MCX_OK;
    }
    // S.
    HIP_TRY(recs.alloc(ncalls));
    HIP_TRY(tlen.alloc(ncalls + 1));
    HIP_TRY(toff.alloc(ncalls + 1));
    const BbText X{G, forks + f0, id0, ncalls, p->max_flank, calls.p, brs.p, steps.p, sfirst.p, toff.p};
    GRID_LAUNCH(k_bb_size, ncalls + 1, X, recs.p, tlen.p);
    if ((rc2 = scan_total(st, (const uint64_t *)tlen.p, toff.p, ncalls + 1, &total)) != MCX_OK) return rc2;
    GRID_LAUNCH(k_bb_offsets, ncalls, ncalls, (const uint64_t *)toff.p, text_base, recs.p);
    if (rec_sink) {
      std::vector<mcx_bubble_rec> h(ncalls);
      HIP_TRY(hipMemcpyAsync(h.data(), recs.p, ncalls * sizeof(mcx_bubble_rec), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (rec_sink(rec_ctx, h.data(), ncalls * sizeof(mcx_bubble_rec)) != 0) return fail(MCX_ERR_SINK, "bubbles: the sink refused the records");
    }
    // T.
    if (text_sink) {
      auto produce = [&](uint64_t c0, int b) -> int {  // emit text bytes [c0, c0 + chunk) into buffer b, then copy them out
        const uint64_t c1 = std::min(total, c0 + chunk);
        GRID_LAUNCH(k_bb_emit, c1 - c0, X, c0, c1 - c0, (uint8_t *)g->d_stage[b]);
        HIP_TRY(hipEventRecord(g->ev[b], st));
        HIP_TRY(hipStreamWaitEvent(g->cstream, g->ev[b], 0));
        HIP_TRY(hipMemcpyAsync(g->h_stage[b], g->d_stage[b], c1 - c0, hipMemcpyDeviceToHost, g->cstream));
        HIP_TRY(hipEventRecord(g->ev_copy[b], g->cstream));
        return MCX_OK;
      };
      if ((rc2 = drain_to_sink(g, total, chunk, produce, text_sink, text_ctx, "bubbles: the sink refused the text")) != MCX_OK) return rc2;
    }
    HIP_TRY(hipStreamSynchronize(st));
    id0 += ncalls;
    text_base += total;
    return MCX_OK;
  };
  auto run = [&]() -> int {
    int rc2 = fork_list();
    phase_clock("bubbles", "forks listed and sorted", t0);
    for (uint64_t f0 = 0; rc2 == MCX_OK && f0 < m; f0 += B) rc2 = batch(f0, std::min(B, m - f0));
    phase_clock("bubbles", "walked, grouped and emitted", t0);
    return rc2;
  };
  rc = run();
  (void)hipStreamSynchronize(st);  // before the scratch goes
  (void)hipStreamSynchronize(g->cstream);
  if (rc != MCX_OK) return rc;
  if (stats) {
    unsigned long long h[kBbNStats];
    HIP_TRY(hipMemcpy(h, d_stats.p, sizeof(h), hipMemcpyDeviceToHost));
    uint64_t *dst = &stats->forks;
    for (uint32_t i = 0; i < kBbNStats; i++) dst[i] += h[i];
  }
  return MCX_OK;
}
