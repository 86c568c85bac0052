// mcx_breakpoints.h -- `breakpoints` on the device (included by mcx_api.hip behind mcx_bubbles.h).
//
// ctx_breakpoints.c without link files: the k-mer occurrence index of a reference genome (kmer_occur.c), from every
// break a 5' flank walk and allele walks per colour (graph_crawler.c) that carry the set of reference runs from k-mer
// to k-mer (kograph_filter_extend, gcrawler_stop_at_ref_covg), the merge of equal paths and the call text of
// process_contig (breakpoint_caller.c).  include/mcx_gpu.h restates the semantics; tests/breakpoints_restate.py is the
// same in Python.  The graph view is that of `bubbles`: union edges, in a colour iff the value word of the colour is
// non-zero, AN EDGE THAT NAMES AN ABSENT K-MER COUNTS AS NO EDGE.  The dense ids, slots and union edges are those of
// mcx_graph_unitig_stats' cache; the walks go k-mer by k-mer (every k-mer's occurrence list is needed anyway) and find
// the ends of a step's unitig as db_unitig_extend does.
// The passes ("breakpoints' device passes"):
//   R. the genome into the last colour: mcx_graph_add_reads, or with NO_REF_EDGES k_bp_kmers<keys>, a scan, k_bp_pack
//      and the tuple insert with empty edge bytes
//   O. k_bp_kmers<probe>: a thread per start position of the genome: the canonical key, a read-only lookup, the tuple
//      (dense id, chrom << 33 | offset << 1 | orient); a scan and k_bp_pack compact the hits in genome order, a stable
//      radix sort by id and k_bp_count with a scan give the CSR ooff / occ: per k-mer its occurrences by (chrom, offset)
//   B. k_bp_breaks, a scan, k_bb_forklist and sort_perm_by_words: the k-mers that occur in the genome and have a
//      successor that does not, in ascending key order; bit 4 o + x of bmask: successor x of orientation o is a break
//   Per batch of "breakpoints_batch" break k-mers; walk p = ((f * 2 + o) * 4 + x) * ncols + colour has four lanes:
//   W. bp_walk<COUNT>, scans, bp_walk<WRITE>.  The counting walk goes without the repeat rule (it stores no nodes to
//      look entries up in) and ends in a cycle once one node was entered three times since a checkpoint.  THE INVARIANT:
//      the writing walk is a prefix of the counting walk that ends at one of its step ends (or at the hard cap, where
//      both end).  So the counting walk's nodes bound the writing walk's.  The runs a walk hands out at its end -- the
//      ended ones and the active ones of at least min_ref k-mers -- do NOT grow along the walk (an active run of exactly
//      min_ref k-mers counts while it lasts and is dropped when it ends), so their bound is the largest such number at
//      any step end of the counting walk, not the number at its end.  The walks run first for the 5' flanks, then,
//      after k_bp_merge has merged the equal flanks of a break and dropped those without a run, for the alleles.  One round of the loop is one k-mer: lane 0
//      updates the walk's runs (its range of the run pool: active, next and ended runs, "breakpoints_runs" each; a walk
//      that outgrows it makes the host double the ranges and walk the batch again), the four lanes look up the four
//      successors.  At the end of a unitig: the stop rule, the walker's choice, the repeat rule.
//   M. k_bp_merge: a thread per break: the smallest colour with the same path, per colour; k_bp_calls<COUNT>, a scan,
//      k_bp_calls<WRITE>: the calls in the order (flank's smallest colour, allele's smallest colour)
//   S. k_bp_size: a thread per call: the record and the text length; a scan gives 64-bit text offsets
//   T. k_bp_emit: driven by the output: a thread per byte of the requested range finds its call by binary search and
//      runs bp_text up to that byte (sequence stretches are skipped by their length)
// All are grid-stride loops (the "grid" knob caps the launches); after pass R the table is only read.  Every loop is
// bounded: a walk by 4 n + 4 nodes for n k-mers (the repeat rule lets an oriented node be entered twice), the run
// updates by the pool range, the merges by the colours and the path lengths.
#pragma once
#include "mcx_bubbles.h"

namespace mcx {

enum : uint32_t { kBpOcc = 0, kBpRefKeys, kBpRefAdded, kBpBreaks, kBpFlankWalks, kBpFlanks, kBpFlanksNoRun, kBpAlleleWalks, kBpAlleles, kBpAllelesNoRun,
                  kBpCalls, kBpSteps, kBpRunsStarted, kBpRunsEnded, kBpStopRuns, kBpStopMaxRef, kBpStopFlank, kBpStopNoCovg, kBpStopNoColCovg,
                  kBpStopNoLinks, kBpStopRepeat, kBpStopBound, kBpReruns, kBpNStats };
constexpr uint32_t kBpNone = 0xFFFFFFFFu;

struct BpGraph {  // the table, the dense ids of `clean`'s cache and the occurrence index
  TableView t;
  int k, W;
  uint32_t ncols;
  uint64_t n;
  const uint64_t *slot_of;
  const uint32_t *map;
  const uint8_t *ue;
  const uint64_t *ooff, *occ;  // occ: chrom << 33 | offset << 1 | orient
};
struct BpRun {  // KOccurRun: cs = chrom << 2 | strand << 1 | used
  uint32_t first, last, qoffset, cs;
};
__device__ __forceinline__ uint32_t bp_len(const BpRun &r) { return (r.last > r.first ? r.last - r.first : r.first - r.last) + 1u; }

// successor of the oriented node v over base x, as bb_succ
template <int W> __device__ __forceinline__ uint32_t bp_succ(const BpGraph &a, uint32_t v, uint32_t x, bool on, uint64_t &slot)
{
  slot = kNoSlot;
  if (!on) return kBpNone;
  const uint32_t i = v >> 1, o = v & 1u;
  if (!((a.ue[i] >> (4u * o + x)) & 1u)) return kBpNone;
  uint32_t p = 0;
  slot = cl_next<W>(a.t, cl_key<W>(a.t, a.slot_of[i]), o, x, a.k, p);
  return slot == kNoSlot ? kBpNone : 2u * a.map[slot] + p;
}
// base P (0 .. k - 1) of the oriented node v, as a code
__device__ __forceinline__ uint32_t bp_base(const BpGraph &a, uint32_t v, uint32_t P)
{
  const uint32_t k1 = (uint32_t)(a.k - 1), o = v & 1u, b = o ? k1 - P : P, bit = 2u * (k1 - b);
  const uint32_t nuc = (uint32_t)(key_ptr(a.t, a.slot_of[v >> 1])[a.W - 1 - (int)(bit >> 6)] >> (bit & 63u)) & 3u;
  return o ? 3u - nuc : nuc;
}
// r with off[r] <= p < off[r + 1], for p < off[n]
__device__ __forceinline__ uint64_t bp_find(const uint64_t *off, uint64_t n, uint64_t p)
{
  uint64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// O / R. a thread per start position p of the genome (bases[off[c] .. off[c + 1]) is chromosome c).  KEYS: flag[p] = the
// k-mer is valid, keys[p * W ..] = its canonical key.  Otherwise: flag[p] = it is a key of the table, ids[p] = its dense
// id, tup[p] = chrom << 33 | offset << 1 | orient.  flag[total] = 0.
template <int W, bool KEYS>
__device__ __forceinline__ void bp_kmers(const BpGraph &a, const uint8_t *bases, const uint64_t *off, uint64_t nchroms, uint64_t total, uint8_t *flag,
                                         uint64_t *ids, uint64_t *tup)
{
  for (uint64_t p = cl_first(); p <= total; p += cl_stride()) {
    if (p == total) { flag[p] = 0; continue; }
    const uint64_t c = bp_find(off, nchroms, p);
    bool ok = p + (uint64_t)a.k <= off[c + 1];
    Kmer<W> fw;
    for (int i = 0; i < W; i++) fw.w[i] = 0;
    for (int i = 0; ok && i < a.k; i++) {
      const uint32_t ch = bases[p + i] & 0xDFu;
      ok = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
      kmer_push<W>(fw, base_code(ch), a.k);
    }
    if (!ok) { flag[p] = 0; continue; }
    const Kmer<W> rc = revcomp<W>(fw, a.k);
    uint32_t o = 0;
    const Kmer<W> key = canonical<W>(fw, rc, o);
    if (KEYS) {
      flag[p] = 1;
      for (int i = 0; i < W; i++) ids[p * W + i] = key.w[i];
    } else {
      uint32_t novel = 0, full = 0;
      const uint64_t slot = find_or_insert_rec<W>(a.t, key, true, novel, full);  // must_exist: read-only
      flag[p] = slot != kNoSlot;
      if (slot != kNoSlot) {
        ids[p] = a.map[slot];
        tup[p] = c << 33 | (p - off[c]) << 1 | o;
      }
    }
  }
}
template <int W>
__global__ __launch_bounds__(256) void k_bp_kmers_keys(BpGraph a, const uint8_t *bases, const uint64_t *off, uint64_t nchroms, uint64_t total, uint8_t *flag,
                                                       uint64_t *keys)
{
  bp_kmers<W, true>(a, bases, off, nchroms, total, flag, keys, nullptr);
}
template <int W>
__global__ __launch_bounds__(256) void k_bp_kmers_probe(BpGraph a, const uint8_t *bases, const uint64_t *off, uint64_t nchroms, uint64_t total, uint8_t *flag,
                                                        uint64_t *ids, uint64_t *tup)
{
  bp_kmers<W, false>(a, bases, off, nchroms, total, flag, ids, tup);
}
// the flagged items of `in` (nw words each) to their scanned places
__global__ __launch_bounds__(256) void k_bp_pack(uint64_t total, uint32_t nw, const uint8_t *flag, const uint64_t *ex, const uint64_t *in, uint64_t *out)
{
  for (uint64_t p = cl_first(); p < total; p += cl_stride())
    if (flag[p])
      for (uint32_t i = 0; i < nw; i++) out[ex[p] * nw + i] = in[p * nw + i];
}
// cnt[id]++ per occurrence; cnt[n] stays 0
__global__ __launch_bounds__(256) void k_bp_count(uint64_t m, const uint64_t *ids, unsigned long long *cnt)
{
  for (uint64_t i = cl_first(); i < m; i += cl_stride()) atomicAdd(&cnt[ids[i]], 1ull);
}

// B. bmask[i] bit 4 o + x: k-mer i occurs in the genome and its successor x on side o is a key that does not
template <int W> __global__ __launch_bounds__(256) void k_bp_breaks(BpGraph a, uint8_t *flag, uint8_t *bmask, unsigned long long *stats)
{
  unsigned long long nb = 0, nk = 0;
  for (uint64_t i = cl_first(); i <= a.n; i += cl_stride()) {
    if (i == a.n) { flag[i] = 0; continue; }
    uint32_t mask = 0;
    if (a.ooff[i + 1] > a.ooff[i]) {
      nk++;
      for (uint32_t ox = 0; ox < 8; ox++) {
        uint64_t s;
        const uint32_t v = bp_succ<W>(a, (uint32_t)(2 * i + (ox >> 2)), ox & 3u, true, s);
        if (v != kBpNone && a.ooff[(v >> 1) + 1] == a.ooff[v >> 1]) { mask |= 1u << ox; nb++; }
      }
    }
    bmask[i] = (uint8_t)mask;
    flag[i] = mask != 0;
  }
  block_add(&stats[kBpBreaks], nb);
  block_add(&stats[kBpRefKeys], nk);
}

// ---- walks -----------------------------------------------------------------------------------------------------------
struct BpPaths {  // what a round of walks leaves: per walk its nodes and its runs (sorted; a flank's reversed)
  uint64_t *pcnt, *rcnt;  // COUNT: the bounds per walk
  uint64_t *poff, *roff;  // the scans of those: the places in the pools
  uint32_t *plen, *nruns, *rep;
  uint32_t *nodes;
  BpRun *runs;
};
struct BpWalk {
  const uint64_t *brk;  // the batch's break k-mers (dense ids) in key order
  const uint8_t *bmask;
  uint64_t nwalks;
  uint32_t min_ref, max_ref, R, allele;
  uint64_t cap;          // nodes of a walk at the most
  const uint32_t *live;  // allele walks: per walk, whether its colour's flank has a run (k_bp_merge)
  BpPaths P;
  BpRun *pool;
  unsigned long long *over, *stats;
};

// korun_extend and the ended-run filter of kograph_filter_extend for one node: A (nA runs) is scanned against the
// node's occurrences, the extended and the new runs go to T, the runs that end with more than min_ref k-mers to E.
// false: T or E is full.
__device__ __forceinline__ bool bp_extend(const BpGraph &a, uint32_t v, uint32_t qoffset, uint32_t min_ref, uint32_t R, BpRun *A, uint32_t nA, BpRun *T,
                                          uint32_t &nT, BpRun *E, uint32_t &nE, unsigned long long &started, unsigned long long &ended)
{
  nT = 0;
  uint32_t starti = 0;
  for (uint64_t q = a.ooff[v >> 1]; q < a.ooff[(v >> 1) + 1]; q++) {
    const uint64_t oc = a.occ[q], offset = (oc >> 1) & 0xFFFFFFFFull;
    const uint32_t chrom = (uint32_t)(oc >> 33), strand = ((uint32_t)oc & 1u) == (v & 1u) ? 0u : 1u;
    while (starti < nA && ((A[starti].cs >> 2) < chrom || (uint64_t)A[starti].last + 1u < offset)) starti++;
    bool used = false;
    for (uint32_t i = starti; i < nA; i++) {
      if ((A[i].cs >> 2) > chrom || (uint64_t)A[i].last > offset + 1u) break;
      const uint64_t next = strand ? (uint64_t)A[i].last - 1u : (uint64_t)A[i].last + 1u;  // (last 0, strand -: no offset equals it)
      if (next == offset) {
        if (nT == R) return false;
        T[nT++] = BpRun{A[i].first, (uint32_t)offset, A[i].qoffset, chrom << 2 | strand << 1};
        A[i].cs |= 1u;
        used = true;
      }
    }
    if (!used) {
      if (nT == R) return false;
      T[nT++] = BpRun{(uint32_t)offset, (uint32_t)offset, qoffset, chrom << 2 | strand << 1};
      started++;
    }
  }
  for (uint32_t i = 0; i < nA; i++)
    if (!(A[i].cs & 1u) && bp_len(A[i]) > min_ref) {
      if (nE == R) return false;
      E[nE++] = A[i];
      ended++;
    }
  return true;
}
// korun_cmp_qoffset
__device__ __forceinline__ bool bp_run_less(const BpRun &x, const BpRun &y)
{
  if (x.qoffset != y.qoffset) return x.qoffset < y.qoffset;
  if ((x.cs >> 2) != (y.cs >> 2)) return (x.cs >> 2) < (y.cs >> 2);
  if (x.first != y.first) return x.first < y.first;
  return x.last < y.last;
}

// W. Four lanes per walk; one round of the loop is one k-mer of graph_crawler_load_path's current step.
template <int W, bool WRITE> __device__ __forceinline__ void bp_walk(const BpGraph &a, const BpWalk &w)
{
  const uint32_t lane = threadIdx.x & 63u, sub = lane & 3u, g0 = lane & ~3u;
  const uint64_t per_block = blockDim.x >> 2;
  unsigned long long c[kBpNStats];
  for (uint32_t i = 0; i < kBpNStats; i++) c[i] = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < w.nwalks; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t p = base + (threadIdx.x >> 2);
    const bool mine = p < w.nwalks;
    bool live = mine;
    uint32_t colour = 0, fork = 0, x = 0;
    if (live) {
      const uint64_t item = p / a.ncols;
      colour = (uint32_t)(p % a.ncols);
      const uint32_t fi = (uint32_t)w.brk[item >> 3], ox = (uint32_t)(item & 7u);
      fork = 2u * fi + (ox >> 2);
      x = ox & 3u;
      live = ((w.bmask[fi] >> ox) & 1u) && *val_ptr(a.t, a.slot_of[fi], colour) != 0;  // the colour holds the fork node
      if (w.allele) live = live && w.live[p] != 0;
    }
    uint64_t slot;
    const uint32_t succ = bp_succ<W>(a, fork, x, live, slot);  // (the four lanes alike)
    live = live && succ != kBpNone && *val_ptr(a.t, slot, colour) != 0;
    uint32_t v = w.allele ? succ : (fork ^ 1u), first = v;  // the node that the step in hand was entered by
    const uint64_t off = (WRITE && mine) ? w.P.poff[p] : 0;
    const uint64_t place = (WRITE && mine) ? w.P.poff[p + 1] - off : 0;  // the nodes the count found
    BpRun *A = w.pool + p * 3ull * w.R, *T = A + w.R, *E = T + w.R;
    uint32_t len = 0, nA = 0, nE = 0;
    uint32_t ck_node = kBpNone, ck_hits = 0;  // COUNT: the step entry kept to see a cycle by (Brent), and its entries since
    uint64_t nsteps = 0, ck_at = 1;
    uint32_t max_kept = 0;  // COUNT, lane 0: the most runs the walk would hand out were it to end at a step end so far
    bool over = false;
    if (live && sub == 0) c[w.allele ? kBpAlleleWalks : kBpFlankWalks]++;
    while (__builtin_amdgcn_ballot_w64(live)) {  // (the same for the whole wave: the votes cross lanes)
      if (WRITE && live && len >= place) {  // (never, by the invariant of pass W: counted, not written past the walk's place)
        live = false;
        if (sub == 0) c[kBpStopBound]++;
      }
      // the node joins the path; lane 0 carries the runs over it
      uint32_t code = 0;  // what ends the walk here: a stat, or kBpNStats for a full run range
      if (live && sub == 0) {
        uint32_t nT = 0;
        if (!bp_extend(a, v, len, w.min_ref, w.R, A, nA, T, nT, E, nE, c[kBpRunsStarted], c[kBpRunsEnded])) code = kBpNStats;
        BpRun *const t = A;
        A = T;
        T = t;
        nA = nT;
      }
      if (WRITE && live && sub == (len & 3u)) w.P.nodes[off + len] = v;  // node n by lane n % 4, which alone reads it back
      if (live) len++;
      // db_unitig_extend: the step goes on iff the node has one edge out, to a key with one edge in that is neither the
      // step's first k-mer nor this one
      uint64_t nslot;
      const uint32_t cand = bp_succ<W>(a, v, sub, live, nslot);
      const bool ins = cand != kBpNone && *val_ptr(a.t, nslot, colour) != 0;
      const uint32_t F = (uint32_t)(__builtin_amdgcn_ballot_w64(cand != kBpNone) >> g0) & 15u;
      const uint32_t S = (uint32_t)(__builtin_amdgcn_ballot_w64(ins) >> g0) & 15u;
      const uint32_t raw = live ? (a.ue[v >> 1] >> (4u * (v & 1u))) & 15u : 0u;
      const uint32_t only = (uint32_t)__shfl((int)cand, (int)(g0 + (raw ? (uint32_t)__builtin_ctz(raw) : 0u)));
      bool inside = live && raw && !(raw & (raw - 1u)) && F == raw;
      if (inside) inside = cl_outdeg(a.ue[only >> 1], 1u - (only & 1u)) == 1 && (only >> 1) != (first >> 1) && (only >> 1) != (v >> 1);
      // the end of a step: gcrawler_stop_at_ref_covg
      if (live && !inside && sub == 0 && !code) {
        uint32_t min_run = kBpNone, min_ended = kBpNone, maxlen = 0, kept = nE;
        for (uint32_t i = 0; i < nA; i++) {
          min_run = min(min_run, A[i].qoffset);
          maxlen = max(maxlen, bp_len(A[i]));
          kept += bp_len(A[i]) >= w.min_ref;
        }
        max_kept = max(max_kept, kept);
        for (uint32_t i = 0; i < nE; i++) {
          min_ended = min(min_ended, E[i].qoffset);
          maxlen = max(maxlen, bp_len(E[i]));
        }
        if (min_run > min_ended) code = kBpStopRuns;
        else if (w.max_ref && maxlen >= w.max_ref) code = kBpStopMaxRef;
        else if (!w.allele && !nA) code = kBpStopFlank;
      }
      code = (uint32_t)__shfl((int)code, (int)g0);
      uint32_t choice = 0;
      const uint32_t cause = bb_choose(F, S, choice);
      const uint32_t next = (uint32_t)__shfl((int)cand, (int)(g0 + choice));
      const bool was = live, at_end = live && !inside;
      if (live && code) {
        live = false;
        if (code == kBpNStats) over = true;
        else if (sub == 0) c[code]++;
      }
      if (was && at_end && sub == 0 && code != kBpNStats) c[kBpSteps]++;
      if (live && at_end && cause) {
        live = false;
        if (sub == 0) c[cause == kBbNoCovg ? kBpStopNoCovg : cause == kBbNoColCovg ? kBpStopNoColCovg : kBpStopNoLinks]++;
      }
      if (WRITE) {  // rpt_walker_attempt_traverse: the entries so far are the occurrences behind the walk's first node
        uint32_t cnt = 0;
        if (live && at_end)
          for (uint32_t i = sub ? sub : 4u; i < len; i += 4)
            if (w.P.nodes[off + i] == next) cnt++;
        cnt += __shfl_xor(cnt, 1);
        cnt += __shfl_xor(cnt, 2);
        if (live && at_end && cnt >= 2u) {  // the third entry
          live = false;
          if (sub == 0) c[kBpStopRepeat]++;
        }
      }
      if (!WRITE && live && at_end) {
        // The count goes without the repeat rule.  A walk that entered one node three times has been stopped by that
        // rule at the third entry or before (at a step end the count has passed), so the count may end there: the entry that is kept moves on at every power
        // of two of the steps, which finds a cycle within a few turns of it.
        if (next == ck_node && ++ck_hits >= 2u) live = false;
        if (live && ++nsteps == ck_at) {
          ck_node = next;
          ck_hits = 0;
          ck_at *= 2;
        }
      }
      if (live) {
        v = at_end ? next : only;
        if (at_end) first = v;
        if (len >= w.cap) {
          live = false;
          if (sub == 0) c[kBpStopBound]++;
        }
      }
    }
    // gcrawler_finish_ref_covg: the ended runs and the active ones of at least min_ref k-mers; a flank's are reversed
    // (koruns_reverse); sorted (koruns_sort_by_qoffset)
    if (mine && sub == 0) {
      uint32_t nr = 0;
      BpRun *out = WRITE ? w.P.runs + w.P.roff[p] : nullptr;
      const uint32_t room = WRITE ? (uint32_t)(w.P.roff[p + 1] - w.P.roff[p]) : 0u;
      for (uint32_t half = 0; half < 2; half++) {
        const BpRun *src = half ? A : E;
        const uint32_t ns = half ? nA : nE;
        for (uint32_t i = 0; i < ns; i++) {
          if (half && bp_len(src[i]) < w.min_ref) continue;
          if (WRITE && nr == room) {  // (never, by the invariant of pass W: counted, not written past the walk's place)
            c[kBpStopBound]++;
            break;
          }
          if (WRITE) {
            BpRun r = src[i];
            r.cs &= ~1u;
            if (!w.allele) {
              const uint32_t ln = bp_len(r) - 1u, f = r.first;
              r.first = r.last;
              r.last = f;
              r.cs ^= 2u;
              r.qoffset = len - 1u - r.qoffset - ln;
            }
            uint32_t j = nr;
            for (; j > 0 && bp_run_less(r, out[j - 1]); j--) out[j] = out[j - 1];
            out[j] = r;
          }
          nr++;
        }
      }
      if (WRITE) {
        w.P.plen[p] = len;
        w.P.nruns[p] = nr;
      } else {
        w.P.pcnt[p] = len;
        w.P.rcnt[p] = max(nr, max_kept);
        if (over) atomicAdd(w.over, 1ull);
      }
    }
  }
  if (WRITE)
    for (uint32_t i = kBpFlankWalks; i <= kBpStopBound; i++) block_add(&w.stats[i], c[i]);
}
template <int W> __global__ __launch_bounds__(256) void k_bp_walk_count(BpGraph a, BpWalk w) { bp_walk<W, false>(a, w); }
template <int W> __global__ __launch_bounds__(256) void k_bp_walk_write(BpGraph a, BpWalk w) { bp_walk<W, true>(a, w); }

// M. a thread per break (item): rep[p] = the smallest colour of the item whose walk has the nodes of p's (graph_crawler_fetch's
// merge), kBpNone where there was no walk.  group (alleles): only walks of one flank merge.  live (flanks): per walk,
// whether the merged flank has a run, so that its colour walks the allele.
__global__ __launch_bounds__(256) void k_bp_merge(uint64_t nitems, uint32_t ncols, BpPaths P, const uint32_t *group, uint32_t *live, unsigned long long *stats)
{
  unsigned long long n_merged = 0, n_norun = 0;
  for (uint64_t item = cl_first(); item < nitems; item += cl_stride()) {
    const uint64_t p0 = item * ncols;
    for (uint32_t cc = 0; cc < ncols; cc++) {
      const uint64_t p = p0 + cc;
      uint32_t rep = kBpNone;
      if (P.plen[p]) {
        rep = cc;
        for (uint32_t c2 = 0; c2 < cc; c2++) {
          const uint64_t q = p0 + c2;
          if (P.plen[q] != P.plen[p] || (group && group[q] != group[p])) continue;
          bool same = true;
          for (uint32_t i = 0; i < P.plen[p] && same; i++) same = P.nodes[P.poff[p] + i] == P.nodes[P.poff[q] + i];
          if (same) { rep = c2; break; }
        }
        if (rep == cc) {
          n_merged++;
          if (!P.nruns[p]) n_norun++;
        }
      }
      P.rep[p] = rep;
      if (live) live[p] = rep != kBpNone && P.nruns[p0 + rep] != 0;
    }
  }
  block_add(&stats[group ? kBpAlleles : kBpFlanks], n_merged);
  block_add(&stats[group ? kBpAllelesNoRun : kBpFlanksNoRun], n_norun);
}
// the calls of an item: the merged alleles with a run, by (flank's smallest colour, allele's smallest colour)
template <bool WRITE>
__global__ __launch_bounds__(256) void k_bp_calls(uint64_t nitems, uint32_t ncols, const uint32_t *rep5, const uint32_t *rep3, const uint32_t *nruns3,
                                                  uint64_t *ncall, const uint64_t *coff, uint64_t *calls)
{
  for (uint64_t item = cl_first(); item <= nitems; item += cl_stride()) {
    if (item == nitems) {
      if (!WRITE) ncall[item] = 0;
      continue;
    }
    const uint64_t p0 = item * ncols;
    uint64_t n = 0;
    for (uint32_t f = 0; f < ncols; f++) {
      if (rep5[p0 + f] != f) continue;
      for (uint32_t cc = f; cc < ncols; cc++)
        if (rep5[p0 + cc] == f && rep3[p0 + cc] == cc && nruns3[p0 + cc]) {
          if (WRITE) calls[coff[item] + n] = p0 + cc;
          n++;
        }
    }
    if (!WRITE) ncall[item] = n;
  }
}

// ---- text ------------------------------------------------------------------------------------------------------------
struct BpText {
  BpGraph g;
  const uint64_t *brk;
  uint64_t id0, ncalls;  // the batch's first call id
  BpPaths P5, P3;
  const uint64_t *calls, *toff;
  const char *names;
  const uint64_t *name_off;
};
// a writer that counts, and keeps the byte at `want`
struct BpOut {
  uint64_t pos, want;
  char ch;
  __device__ __forceinline__ void put(char x)
  {
    if (pos == want) ch = x;
    pos++;
  }
  __device__ __forceinline__ void str(const char *s)
  {
    for (; *s; s++) put(*s);
  }
  __device__ __forceinline__ void num(uint64_t x)
  {
    const uint32_t nd = bb_digits(x);
    for (uint32_t i = 0; i < nd; i++) put(bb_digit(x, nd, i));
  }
  __device__ __forceinline__ bool past() const { return pos > want; }
  // a stretch of n bytes: true when `want` lies in it, at *at
  __device__ __forceinline__ bool in(uint64_t n, uint64_t *at)
  {
    const bool hit = want >= pos && want - pos < n;
    *at = want - pos;
    pos += n;
    return hit;
  }
};
// korun_gzprint
__device__ __forceinline__ void bp_run_text(const BpText &x, BpOut &o, const BpRun &r, uint32_t first_kmer_idx, uint32_t kmer_offset)
{
  const uint32_t chrom = r.cs >> 2, strand = (r.cs >> 1) & 1u, k1 = (uint32_t)(x.g.k - 1);
  for (uint64_t i = x.name_off[chrom]; i < x.name_off[chrom + 1]; i++) o.put(x.names[i]);
  const uint64_t start = strand ? (uint64_t)r.first + k1 - kmer_offset : (uint64_t)r.first + kmer_offset, end = strand ? (uint64_t)r.last : (uint64_t)r.last + k1;
  o.put(':');
  o.num(start + 1u);
  o.put('-');
  o.num(end + 1u);
  o.put(':');
  o.put(strand ? '-' : '+');
  o.put(':');
  o.num((uint64_t)(r.qoffset - first_kmer_idx) + 1u);
}
// process_contig: the text of call r up to the byte o.want (all of it for a count); the record when rec is not null
__device__ void bp_text(const BpText &x, uint64_t r, BpOut &o, mcx_breakpoint_rec *rec)
{
  const BpGraph &a = x.g;
  const uint64_t p3 = x.calls[r], p0 = p3 - p3 % a.ncols, p5 = p0 + x.P5.rep[p3], id = x.id0 + r;
  const uint32_t *n5 = x.P5.nodes + x.P5.poff[p5], *n3 = x.P3.nodes + x.P3.poff[p3];
  const uint32_t nf = x.P5.plen[p5], na = x.P3.plen[p3], nr5 = x.P5.nruns[p5], nr3 = x.P3.nruns[p3], k1 = (uint32_t)(a.k - 1);
  const BpRun *r5 = x.P5.runs + x.P5.roff[p5], *r3 = x.P3.runs + x.P3.roff[p3];
  const uint32_t flank3pidx = r3[0].qoffset, extra = min(k1, flank3pidx), path_kmers = flank3pidx - extra, kmer3poffset = k1 - extra;
  uint64_t at;
  if (rec) {
    const uint64_t item = p3 / a.ncols;
    const uint32_t fi = (uint32_t)x.brk[item >> 3];
    const uint64_t *key = key_ptr(a.t, a.slot_of[fi]);
    for (int i = 0; i < 4; i++) rec->fork_key[i] = i < a.W ? (i ? key[i] : (key[0] & kKeyMask)) : 0ull;
    rec->fork_orient = (uint32_t)(item >> 2) & 1u;
    rec->succ_base = (uint32_t)item & 3u;
    rec->path_kmers = path_kmers;
    rec->flank5p_kmers = nf;
    rec->flank3p_kmers = na - path_kmers;
    rec->flank5p_runs = nr5;
    rec->flank3p_runs = nr3;
    uint32_t nc = 0;
    for (uint32_t cc = 0; cc < a.ncols; cc++) nc += x.P5.rep[p0 + cc] != kBpNone && x.P3.rep[p0 + cc] == (uint32_t)(p3 - p0);
    rec->num_cols = nc;
  }
  o.str(">brkpnt.call");
  o.num(id);
  o.str(".5pflank chr=");
  for (uint32_t i = 0; i < nr5 && !o.past(); i++) {
    if (i) o.put(',');
    bp_run_text(x, o, r5[i], 0, 0);
  }
  o.put('\n');
  if (o.past()) return;
  // the flank is the walk reversed: its first k-mer whole, then the last base of every further node
  if (o.in((uint64_t)a.k, &at)) { o.ch = "ACGT"[bp_base(a, n5[nf - 1] ^ 1u, (uint32_t)at)]; return; }
  if (o.in((uint64_t)nf - 1u, &at)) { o.ch = "ACGT"[bp_base(a, n5[nf - 2u - (uint32_t)at] ^ 1u, k1)]; return; }
  o.put('\n');
  o.str(">brkpnt.call");
  o.num(id);
  o.str(".3pflank chr=");
  for (uint32_t i = 0; i < nr3 && !o.past(); i++) {
    if (i) o.put(',');
    bp_run_text(x, o, r3[i], flank3pidx, kmer3poffset);
  }
  o.put('\n');
  if (o.past()) return;
  if (o.in((uint64_t)(na - path_kmers), &at)) { o.ch = "ACGT"[bp_base(a, n3[path_kmers + (uint32_t)at], k1)]; return; }
  o.put('\n');
  o.str(">brkpnt.call");
  o.num(id);
  o.str(".path cols=");
  bool any = false;
  for (uint32_t cc = 0; cc < a.ncols && !o.past(); cc++)
    if (x.P5.rep[p0 + cc] != kBpNone && x.P3.rep[p0 + cc] == (uint32_t)(p3 - p0)) {
      if (any) o.put(',');
      o.num(cc);
      any = true;
    }
  o.put('\n');
  if (o.past()) return;
  if (o.in((uint64_t)path_kmers, &at)) { o.ch = "ACGT"[bp_base(a, n3[(uint32_t)at], k1)]; return; }
  o.put('\n');
  o.put('\n');
}

// S. a thread per call: the record and the length of its text
__global__ __launch_bounds__(256) void k_bp_size(BpText x, mcx_breakpoint_rec *recs, uint64_t *tlen)
{
  for (uint64_t r = cl_first(); r <= x.ncalls; r += cl_stride()) {
    if (r == x.ncalls) { tlen[r] = 0; continue; }
    BpOut o{0, ~0ull, 0};
    mcx_breakpoint_rec R;
    bp_text(x, r, o, &R);
    R.text_off = 0;
    R.text_len = o.pos;
    tlen[r] = o.pos;
    recs[r] = R;
  }
}
__global__ __launch_bounds__(256) void k_bp_offsets(uint64_t ncalls, const uint64_t *toff, uint64_t text_base, mcx_breakpoint_rec *recs)
{
  for (uint64_t r = cl_first(); r < ncalls; r += cl_stride()) recs[r].text_off = text_base + toff[r];
}
// T. bytes [p0, p0 + cnt) of the batch's text go to dst[0 .. cnt).  cnt > 0.
__global__ __launch_bounds__(256) void k_bp_emit(BpText x, uint64_t p0, uint64_t cnt, uint8_t *dst)
{
  for (uint64_t i = cl_first(); i < cnt; i += cl_stride()) {
    const uint64_t p = p0 + i, r = un_find(x.toff, 0, x.ncalls - 1, p);
    BpOut o{0, p - x.toff[r], '?'};
    bp_text(x, r, o, nullptr);
    dst[i] = (uint8_t)o.ch;
  }
}

}  // namespace mcx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" int mcx_graph_breakpoints(mcx_graph *g, const uint8_t *ref_bases, const uint64_t *ref_offsets, uint64_t nchroms, const char *names,
                                     const uint64_t *name_off, const mcx_breakpoints_params *p, mcx_sink_fn rec_sink, void *rec_ctx, mcx_sink_fn text_sink,
                                     void *text_ctx, mcx_breakpoints_stats *stats)
{
  int rc = whole_table_only(g, "breakpoints", " (the walks cross shards)");
  if (rc != MCX_OK) return rc;
  if (!p) return fail(MCX_ERR_ARG, "breakpoints: null parameters");
  if (g->ncols < 2) return fail(MCX_ERR_ARG, "breakpoints: the graph needs a colour for the reference behind its samples (it has %d)", g->ncols);
  if (!nchroms || !ref_bases || !ref_offsets || !names || !name_off) return fail(MCX_ERR_ARG, "breakpoints: no reference sequence");
  if (nchroms > (1ull << 30)) return fail(MCX_ERR_ARG, "breakpoints: more chromosomes than permitted (%llu > 2^30)", (unsigned long long)nchroms);
  for (uint64_t i = 0; i < nchroms; i++) {
    if (ref_offsets[i + 1] < ref_offsets[i]) return fail(MCX_ERR_ARG, "breakpoints: the offsets of sequence %llu run backwards", (unsigned long long)i);
    if (ref_offsets[i + 1] - ref_offsets[i] > (1ull << 32))
      return fail(MCX_ERR_ARG, "breakpoints: sequence %llu is longer than the limit (%llu > 2^32)", (unsigned long long)i,
                  (unsigned long long)(ref_offsets[i + 1] - ref_offsets[i]));
  }
  if (!p->min_ref) return fail(MCX_ERR_ARG, "breakpoints: min_ref must be above 0");
  if (p->max_ref && p->min_ref > p->max_ref) return fail(MCX_ERR_ARG, "breakpoints: min_ref %u is above max_ref %u", p->min_ref, p->max_ref);
  if (p->flags & ~(uint32_t)(MCX_BREAKPOINTS_NO_REF_EDGES | MCX_BREAKPOINTS_REF_LOADED | MCX_BREAKPOINTS_LOAD_ONLY))
    return fail(MCX_ERR_ARG, "breakpoints: unknown flags 0x%x", p->flags);
  if ((p->flags & MCX_BREAKPOINTS_LOAD_ONLY) && (p->flags & MCX_BREAKPOINTS_REF_LOADED))
    return fail(MCX_ERR_ARG, "breakpoints: LOAD_ONLY and REF_LOADED leave nothing to do");
  HIP_TRY(hipSetDevice(g->device));
  hipStream_t st = g->stream;
  const uint64_t total = ref_offsets[nchroms] - ref_offsets[0], nname = name_off[nchroms];
  const int refcol = g->ncols - 1;
  unsigned long long h_stats[kBpNStats];
  for (uint32_t i = 0; i < kBpNStats; i++) h_stats[i] = 0;
  DevBuf<uint8_t> d_bases, flag;
  DevBuf<uint64_t> d_off, ex;
  std::vector<uint64_t> h_off(nchroms + 1);
  for (uint64_t i = 0; i <= nchroms; i++) h_off[i] = ref_offsets[i] - ref_offsets[0];
  HIP_TRY(d_bases.alloc(std::max<uint64_t>(total, 1)));
  HIP_TRY(d_off.alloc(nchroms + 1));
  HIP_TRY(flag.alloc(total + 1));
  HIP_TRY(ex.alloc(total + 1));
  HIP_TRY(hipMemcpyAsync(d_bases.p, ref_bases + ref_offsets[0], total, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), (nchroms + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  double t0 = now_s();

  // R. the genome into the last colour
  if (!(p->flags & MCX_BREAKPOINTS_REF_LOADED)) {
    uint64_t before = 0, after = 0;
    if ((rc = mcx_graph_nkmers(g, &before)) != MCX_OK) return rc;
    if (!(p->flags & MCX_BREAKPOINTS_NO_REF_EDGES)) {
      if ((rc = mcx_graph_add_reads(g, refcol, ref_bases + ref_offsets[0], nullptr, h_off.data(), nchroms, 0, 0, nullptr)) != MCX_OK) return rc;
      if ((rc = mcx_graph_sync(g)) != MCX_OK) return rc;
    } else if (total) {
      DevBuf<uint64_t> keys, packed;
      DevBuf<uint8_t> edges;
      uint64_t m = 0;
      BpGraph K{};
      K.t = g->t;
      K.k = g->k;
      K.W = g->W;
      HIP_TRY(keys.alloc(total * g->W));
      GRID_LAUNCH_W(k_bp_kmers_keys, total + 1, K, (const uint8_t *)d_bases.p, (const uint64_t *)d_off.p, nchroms, total, flag.p, keys.p);
      if ((rc = scan_total(st, (const uint8_t *)flag.p, ex.p, total + 1, &m)) != MCX_OK) return rc;
      if (m) {
        HIP_TRY(packed.alloc(m * g->W));
        HIP_TRY(edges.alloc(m));
        HIP_TRY(hipMemsetAsync(edges.p, 0, m, st));
        GRID_LAUNCH(k_bp_pack, total, total, (uint32_t)g->W, (const uint8_t *)flag.p, (const uint64_t *)ex.p, (const uint64_t *)keys.p, packed.p);
        HIP_TRY(hipStreamSynchronize(st));
        if ((rc = mcx_graph_insert_tuples_dev(g, refcol, packed.p, edges.p, m)) != MCX_OK) return rc;
        if ((rc = mcx_graph_sync(g)) != MCX_OK) return rc;
      }
    }
    if ((rc = mcx_graph_nkmers(g, &after)) != MCX_OK) return rc;
    h_stats[kBpRefAdded] = after - before;
    phase_clock("breakpoints", "reference loaded", t0);
  }
  if (p->flags & MCX_BREAKPOINTS_LOAD_ONLY) {
    if (stats) stats->ref_added += h_stats[kBpRefAdded];
    return MCX_OK;
  }

  uint64_t n = 0;
  if ((rc = ensure_decomposition(g, "breakpoints", true, &n)) != MCX_OK) return rc;
  if ((rc = ensure_stage(g)) != MCX_OK) return rc;
  HIP_TRY(hipStreamSynchronize(st));  // the staging buffers are ours now
  HIP_TRY(hipStreamSynchronize(g->cstream));
  auto finish = [&]() -> int {
    if (stats) {
      uint64_t *dst = &stats->occurrences;
      for (uint32_t i = 0; i < kBpNStats; i++) dst[i] += h_stats[i];
    }
    return MCX_OK;
  };
  if (!n) return finish();
  const CleanCache *c = g->clean;
  const uint32_t ncols = (uint32_t)g->ncols;
  BpGraph G{g->t, g->k, g->W, ncols, n, c->slot_of.p, c->map.p, c->ue.p, nullptr, nullptr};
  const uint64_t B = std::max<uint64_t>(1, std::min<uint64_t>(g->breakpoints_batch ? g->breakpoints_batch : 65536, 1u << 20));  // break k-mers per round
  uint64_t chunk = std::min<uint64_t>(kStageBytes, g->stage_alloc) & ~15ull;
  if (g->breakpoints_chunk) chunk = std::min<uint64_t>(chunk, g->breakpoints_chunk);
  uint32_t R = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(g->breakpoints_runs ? g->breakpoints_runs : 16, 1u << 24));
  DevBuf<unsigned long long> d_stats, cnt, d_over;
  DevBuf<uint64_t> ooff, occ, ids, tup, ids2, l0, l1, k0, k1, d_name_off;
  DevBuf<uint8_t> bmask, tmp;
  DevBuf<char> d_names;
  uint64_t *brk = nullptr, m = 0, nocc = 0, text_base = 0, id0 = 0;

  // O. the occurrence index, B. the break k-mers in key order
  auto index = [&]() -> int {
    int rc2;
    HIP_TRY(d_stats.alloc(kBpNStats));
    HIP_TRY(hipMemsetAsync(d_stats.p, 0, kBpNStats * 8, st));
    HIP_TRY(d_over.alloc(1));
    HIP_TRY(d_names.alloc(std::max<uint64_t>(nname, 1)));
    HIP_TRY(d_name_off.alloc(nchroms + 1));
    HIP_TRY(hipMemcpyAsync(d_names.p, names, nname, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_name_off.p, name_off, (nchroms + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ids.alloc(total + 1));
    HIP_TRY(tup.alloc(total + 1));
    GRID_LAUNCH_W(k_bp_kmers_probe, total + 1, G, (const uint8_t *)d_bases.p, (const uint64_t *)d_off.p, nchroms, total, flag.p, ids.p, tup.p);
    if ((rc2 = scan_total(st, (const uint8_t *)flag.p, ex.p, total + 1, &nocc)) != MCX_OK) return rc2;
    HIP_TRY(cnt.alloc(n + 1));
    HIP_TRY(ooff.alloc(n + 1));
    HIP_TRY(hipMemsetAsync(cnt.p, 0, (n + 1) * 8, st));
    HIP_TRY(occ.alloc(nocc + 1));
    if (nocc) {
      DevBuf<uint64_t> pid, ptup;
      HIP_TRY(pid.alloc(nocc));
      HIP_TRY(ptup.alloc(nocc));
      HIP_TRY(ids2.alloc(nocc));
      GRID_LAUNCH(k_bp_pack, total, total, 1u, (const uint8_t *)flag.p, (const uint64_t *)ex.p, (const uint64_t *)ids.p, pid.p);
      GRID_LAUNCH(k_bp_pack, total, total, 1u, (const uint8_t *)flag.p, (const uint64_t *)ex.p, (const uint64_t *)tup.p, ptup.p);
      size_t sb = 0;
      HIP_TRY(rocprim::radix_sort_pairs(nullptr, sb, (const uint64_t *)pid.p, ids2.p, (const uint64_t *)ptup.p, occ.p, nocc, 0, 32, st));
      DevBuf<uint8_t> stmp;
      HIP_TRY(stmp.alloc(std::max<size_t>(sb, 1)));
      {
        SpanGuard sp_(g, "k_bp_occ_sort");  // (rocprim's kernels, under one name of this pass)
        HIP_TRY(rocprim::radix_sort_pairs((void *)stmp.p, sb, (const uint64_t *)pid.p, ids2.p, (const uint64_t *)ptup.p, occ.p, nocc, 0, 32, st));
      }
      GRID_LAUNCH(k_bp_count, nocc, nocc, (const uint64_t *)ids2.p, cnt.p);
      HIP_TRY(hipStreamSynchronize(st));  // before the sort's scratch goes
    }
    if ((rc2 = device_scan(st, (const unsigned long long *)cnt.p, ooff.p, n + 1)) != MCX_OK) return rc2;
    ids.release();
    tup.release();
    ids2.release();
    G.ooff = ooff.p;
    G.occ = occ.p;
    h_stats[kBpOcc] = nocc;
    phase_clock("breakpoints", "occurrences indexed", t0);
    // B.
    DevBuf<uint8_t> bflag;
    DevBuf<uint64_t> bex;
    HIP_TRY(bflag.alloc(n + 1));
    HIP_TRY(bmask.alloc(n));
    HIP_TRY(bex.alloc(n + 1));
    GRID_LAUNCH_W(k_bp_breaks, n + 1, G, bflag.p, bmask.p, d_stats.p);
    if ((rc2 = scan_total(st, (const uint8_t *)bflag.p, bex.p, n + 1, &m)) != MCX_OK) return rc2;
    if (!m) return MCX_OK;
    HIP_TRY(l0.alloc(m));
    HIP_TRY(l1.alloc(m));
    HIP_TRY(k0.alloc(m));
    HIP_TRY(k1.alloc(m));
    GRID_LAUNCH(k_bb_forklist, n, (const uint8_t *)bflag.p, (const uint64_t *)bex.p, n, l0.p);
    size_t tmp_bytes = 0;
    if ((rc2 = sort_perm_scratch(st, m, &tmp_bytes)) != MCX_OK) return rc2;
    HIP_TRY(tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
    uint64_t *const keys[2] = {k0.p, k1.p}, *const perm[2] = {l0.p, l1.p};
    auto word = [&](int wd, bool, const uint64_t *through, uint64_t *dst, const uint64_t **) -> int {
      GRID_LAUNCH(k_un_keyword, m, g->t, m, (const uint64_t *)c->slot_of.p, through, (uint32_t)wd, dst);
      return MCX_OK;
    };
    if ((rc2 = sort_perm_by_words(st, m, g->W, 2 * g->k - 64 * (g->W - 1), keys, perm, tmp.p, tmp_bytes, g, word, &brk)) != MCX_OK) return rc2;
    HIP_TRY(hipStreamSynchronize(st));
    return MCX_OK;
  };

  // one round of walks (flanks or alleles) over the batch: count, scans, write; P's arrays are allocated here
  struct Round {
    DevBuf<uint64_t> pcnt, rcnt, poff, roff;
    DevBuf<uint32_t> plen, nruns, rep, nodes;
    DevBuf<BpRun> runs;
  };
  auto walks = [&](BpWalk &W, Round &o, DevBuf<BpRun> &pool, uint64_t &reruns) -> int {
    int rc2;
    const uint64_t nw = W.nwalks;
    uint64_t npool = 0, nruns = 0;
    HIP_TRY(o.pcnt.alloc(nw + 1));
    HIP_TRY(o.rcnt.alloc(nw + 1));
    HIP_TRY(o.poff.alloc(nw + 1));
    HIP_TRY(o.roff.alloc(nw + 1));
    HIP_TRY(o.plen.alloc(nw));
    HIP_TRY(o.nruns.alloc(nw));
    HIP_TRY(o.rep.alloc(nw));
    W.P = BpPaths{o.pcnt.p, o.rcnt.p, o.poff.p, o.roff.p, o.plen.p, o.nruns.p, o.rep.p, nullptr, nullptr};
    for (;;) {
      if (!pool.p && pool.alloc(nw * 3ull * R) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MCX_ERR_NOMEM, "breakpoints: no room for %u runs in each of %llu walks (a smaller breakpoints_batch needs less)", R, (unsigned long long)nw);
      }
      W.R = R;
      W.pool = pool.p;
      unsigned long long over = 0;
      HIP_TRY(hipMemsetAsync(d_over.p, 0, 8, st));
      HIP_TRY(hipMemsetAsync(o.pcnt.p + nw, 0, 8, st));
      HIP_TRY(hipMemsetAsync(o.rcnt.p + nw, 0, 8, st));
      GRID_LAUNCH_W(k_bp_walk_count, nw * 4, G, W);
      HIP_TRY(hipMemcpyAsync(&over, d_over.p, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (!over) break;
      if (R >= (1u << 24)) return fail(MCX_ERR_NOMEM, "breakpoints: a walk holds more than %u runs at a time", R);
      reruns += over;  // the walks that outgrew their range; the batch walks again with twice the room
      R *= 2;
      pool.release();
    }
    if ((rc2 = scan_total(st, (const uint64_t *)o.pcnt.p, o.poff.p, nw + 1, &npool)) != MCX_OK) return rc2;
    if ((rc2 = scan_total(st, (const uint64_t *)o.rcnt.p, o.roff.p, nw + 1, &nruns)) != MCX_OK) return rc2;
    if (o.nodes.alloc(npool + 1) != hipSuccess || o.runs.alloc(nruns + 1) != hipSuccess) {
      (void)hipGetLastError();
      return fail(MCX_ERR_NOMEM, "breakpoints: no room for the %llu nodes of %llu walks (a smaller breakpoints_batch needs less)", (unsigned long long)npool,
                  (unsigned long long)nw);
    }
    W.P.nodes = o.nodes.p;
    W.P.runs = o.runs.p;
    GRID_LAUNCH_W(k_bp_walk_write, nw * 4, G, W);
    return MCX_OK;
  };

  // one batch: the break k-mers [f0, f0 + nf)
  auto batch = [&](uint64_t f0, uint64_t nf) -> int {
    int rc2;
    const uint64_t nitems = 8 * nf, nw = nitems * ncols;
    uint64_t ncalls = 0, ttotal = 0, reruns = 0;
    Round r5, r3;
    DevBuf<BpRun> pool;
    DevBuf<uint32_t> live;
    DevBuf<uint64_t> ncall, coff, calls, tlen, toff;
    DevBuf<mcx_breakpoint_rec> recs;
    BpWalk W{brk + f0, bmask.p, nw, p->min_ref, p->max_ref, R, 0u, 4 * n + 4, nullptr, BpPaths{}, nullptr, d_over.p, d_stats.p};
    if ((rc2 = walks(W, r5, pool, reruns)) != MCX_OK) return rc2;
    const BpPaths P5 = W.P;
    HIP_TRY(live.alloc(nw));
    GRID_LAUNCH(k_bp_merge, nitems, nitems, ncols, P5, (const uint32_t *)nullptr, live.p, d_stats.p);
    W.allele = 1;
    W.live = live.p;
    if ((rc2 = walks(W, r3, pool, reruns)) != MCX_OK) return rc2;
    const BpPaths P3 = W.P;
    GRID_LAUNCH(k_bp_merge, nitems, nitems, ncols, P3, (const uint32_t *)P5.rep, (uint32_t *)nullptr, d_stats.p);
    h_stats[kBpReruns] += reruns;
    HIP_TRY(ncall.alloc(nitems + 1));
    HIP_TRY(coff.alloc(nitems + 1));
    GRID_LAUNCH(k_bp_calls<false>, nitems + 1, nitems, ncols, (const uint32_t *)P5.rep, (const uint32_t *)P3.rep, (const uint32_t *)P3.nruns, ncall.p,
                (const uint64_t *)nullptr, (uint64_t *)nullptr);
    if ((rc2 = scan_total(st, (const uint64_t *)ncall.p, coff.p, nitems + 1, &ncalls)) != MCX_OK) return rc2;
    if (!ncalls) {
      HIP_TRY(hipStreamSynchronize(st));
      return MCX_OK;
    }
    HIP_TRY(calls.alloc(ncalls));
    GRID_LAUNCH(k_bp_calls<true>, nitems + 1, nitems, ncols, (const uint32_t *)P5.rep, (const uint32_t *)P3.rep, (const uint32_t *)P3.nruns, ncall.p,
                (const uint64_t *)coff.p, calls.p);
    // S.
    HIP_TRY(recs.alloc(ncalls));
    HIP_TRY(tlen.alloc(ncalls + 1));
    HIP_TRY(toff.alloc(ncalls + 1));
    const BpText X{G, brk + f0, id0, ncalls, P5, P3, calls.p, toff.p, d_names.p, d_name_off.p};
    GRID_LAUNCH(k_bp_size, ncalls + 1, X, recs.p, tlen.p);
    if ((rc2 = scan_total(st, (const uint64_t *)tlen.p, toff.p, ncalls + 1, &ttotal)) != MCX_OK) return rc2;
    GRID_LAUNCH(k_bp_offsets, ncalls, ncalls, (const uint64_t *)toff.p, text_base, recs.p);
    if (rec_sink) {
      std::vector<mcx_breakpoint_rec> h(ncalls);
      HIP_TRY(hipMemcpyAsync(h.data(), recs.p, ncalls * sizeof(mcx_breakpoint_rec), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (rec_sink(rec_ctx, h.data(), ncalls * sizeof(mcx_breakpoint_rec)) != 0) return fail(MCX_ERR_SINK, "breakpoints: the sink refused the records");
    }
    // T.
    if (text_sink) {
      auto produce = [&](uint64_t c0, int b) -> int {  // emit text bytes [c0, c0 + chunk) into buffer b, then copy them out
        const uint64_t c1 = std::min(ttotal, c0 + chunk);
        GRID_LAUNCH(k_bp_emit, c1 - c0, X, c0, c1 - c0, (uint8_t *)g->d_stage[b]);
        HIP_TRY(hipEventRecord(g->ev[b], st));
        HIP_TRY(hipStreamWaitEvent(g->cstream, g->ev[b], 0));
        HIP_TRY(hipMemcpyAsync(g->h_stage[b], g->d_stage[b], c1 - c0, hipMemcpyDeviceToHost, g->cstream));
        HIP_TRY(hipEventRecord(g->ev_copy[b], g->cstream));
        return MCX_OK;
      };
      if ((rc2 = drain_to_sink(g, ttotal, chunk, produce, text_sink, text_ctx, "breakpoints: the sink refused the text")) != MCX_OK) return rc2;
    }
    HIP_TRY(hipStreamSynchronize(st));
    id0 += ncalls;
    text_base += ttotal;
    return MCX_OK;
  };
  auto run = [&]() -> int {
    int rc2 = index();
    phase_clock("breakpoints", "breaks listed and sorted", t0);
    for (uint64_t f0 = 0; rc2 == MCX_OK && f0 < m; f0 += B) rc2 = batch(f0, std::min(B, m - f0));
    phase_clock("breakpoints", "walked, merged and emitted", t0);
    return rc2;
  };
  rc = run();
  (void)hipStreamSynchronize(st);  // before the scratch goes
  (void)hipStreamSynchronize(g->cstream);
  if (rc != MCX_OK) return rc;
  unsigned long long h[kBpNStats];
  HIP_TRY(hipMemcpy(h, d_stats.p, sizeof(h), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < kBpNStats; i++) h_stats[i] += h[i];
  h_stats[kBpCalls] = id0;
  return finish();
}
