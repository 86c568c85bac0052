// mcx_correct.h -- `correct` on the device (included by mcx_api.hip).
//
// correct_aln_read and handle_read2 (src/alignment/correct_alignment.c, src/tools/correct_reads.c) over a batch of
// reads, without link files: the k-mers of a read that are in the sample are its alignment (db_alignment_from_read), the
// gaps between them are bridged by walking the graph (traverse_one_way2, traverse_two_way2), the two ends are extended
// (correct_aln_read:570-639) and the read is printed with the walked bases in place of its own (handle_read2).
//   Graph view (ctx_correct.c:116-121, 187): every key of the table is walked; a k-mer's edges are the OR of its edge
//   bytes over all colours; a k-mer is in the sample iff its value word in the chosen colour is non-zero.
//   Walker step (graph_walker_choose:385-433 with no paths held): the successors over the union edges; none: stop; one:
//   take it (POPFWD when it is not in the sample); several: those in the sample, exactly one: take it, otherwise stop.
//   The reference asserts that an edge never names an absent k-mer; HERE SUCH AN EDGE COUNTS AS NO EDGE.
//   Repeat rule (repeat_walker.h:18-50; graph_walker_hash64 is a function of (node, orient) when no paths are held): a
//   walk enters an oriented node twice at the most, the third entry stops it.  Every walk starts clean.  The visited
//   bits the reference leaves set after a POPFWD stop and the false positives of its 22-bit Bloom filter are artefacts
//   of its memory layout and are not reproduced.
// Every gap walk and every end extension depends on the alignment alone, so the walks of a batch are independent
// tasks.  The passes ("correct's device passes"):
//   A. k_cr_probe   rt_probe's walk (mcx_reads.h) with a sink that keeps the slots: per stream position one 64-bit node
//                   reference, slot << 1 | orient, all ones where there is no key or the key is not in the sample
//      k_cr_place   (host entry) a chunk's references, indexed by stream position, into the batch's, indexed by base
//                   position (rt_place of mcx_reads.h, as k_cv_place)
//   B. k_cr_tasks   a wave per read: its segments (db_alignment_next_gap) and its walk tasks, first counted, then, behind
//                   two scans, written: the left extension, every gap with its bounds, the right extension.  A task owns
//                   a range of gap_max + 2 (or the extension's limit) path entries.
//   C. k_cr_walk    four lanes per task, one successor candidate each; the path is kept in the task's own range and the
//                   third-entry test counts the node in it: no visited array, no atomics on the table
//   D. k_cr_len     a wave per read: the record's length; a 64-bit scan gives out_off
//      k_cr_emit    a wave per read writes the record
// All are grid-stride loops (the "grid" knob caps the launches); the table is only read.
#pragma once
#include "mcx_clean.h"
#include "mcx_reads.h"

namespace mcx {

constexpr uint64_t kCrNone = ~0ull;
constexpr uint32_t kCrTwoWay = 1;  // = MCX_CORRECT_TWO_WAY
enum : uint32_t { kCrGap = 0, kCrLeft = 1, kCrRight = 2 };
enum : uint32_t { kCrStopNone = 0, kCrStopDead = 1, kCrStopFork = 2, kCrStopColour = 3, kCrStopRepeat = 4 };
// the counters of a call (64-bit words in device memory), in the order of mcx_correct_stats from num_perfect on; behind
// them the walker steps made (what the benchmark tool divides by k_cr_walk's time)
enum : uint32_t {
  kCrPerfect = 0, kCrNoKmers, kCrGaps, kCrFilled, kCrFilledBack, kCrTooShort, kCrTooLong, kCrFork, kCrColour, kCrRepeat,
  kCrMissing, kCrEndGaps, kCrEndExt, kCrBasesFilled, kCrNumCounters, kCrSteps = kCrNumCounters, kCrAllCounters
};

// The sink of rt_probe that `correct` uses.  node has `pitch` entries (a multiple of 64, so a lane's 16 positions are
// inside or outside as a whole).
struct CrRefSink {
  static constexpr bool kSlots = true;
  TableView t;
  uint32_t colour;
  uint64_t pitch;
  uint64_t *node;
  __device__ __forceinline__ void operator()(uint64_t P0, uint32_t hit16, const uint64_t (&slot)[16], uint32_t o16) const
  {
    if (P0 >= pitch) return;
    uint64_t v[kPosPerLane];
#pragma unroll
    for (int j = 0; j < kPosPerLane; j++) v[j] = ((hit16 >> j) & 1u) ? *val_ptr(t, slot[j], colour) : 0ull;  // 16 loads in flight
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(node + P0);
#pragma unroll
    for (int j = 0; j < kPosPerLane; j += 2) {
      const uint64_t a = v[j] ? (slot[j] << 1) | ((o16 >> j) & 1u) : kCrNone;
      const uint64_t b = v[j + 1] ? (slot[j + 1] << 1) | ((o16 >> (j + 1)) & 1u) : kCrNone;
      d[j >> 1] = make_ulonglong2(a, b);
    }
  }
};

template <int W>
__global__ __launch_bounds__(kThreads) void k_cr_probe(StreamArgs a, TableView t, uint32_t colour, uint64_t pitch, uint64_t *node,
                                                       unsigned long long *cnt)
{
  rt_probe<W>(a, t, CrRefSink{t, colour, pitch, node}, cnt);
}

// rt_place (mcx_reads.h) for the node references
__global__ __launch_bounds__(256) void k_cr_place(const uint64_t *so, uint64_t n, const uint64_t *boff, uint64_t r0, uint64_t shift, uint64_t own,
                                                  const uint64_t *snode, uint64_t spitch, uint64_t *node, uint64_t pitch)
{
  rt_place(so, n, boff, r0, shift, own, spitch, pitch, [&](uint64_t p, uint64_t d) { node[d] = snode[p]; });
}

// A batch on the device.  Read r holds the positions [boff[r] - boff[0], boff[r + 1] - boff[0] - sep) of node, seq and
// qual (sep = 1: a stream with one separator behind every read).
struct CrView {
  const uint64_t *boff;
  uint64_t nreads;
  uint32_t sep;
  int k;
  const uint64_t *node;
  const uint8_t *seq, *qual;  // qual may be null
  uint32_t ncols, colour, flags;
  float D, d;  // gap_variance, gap_wiggle
  uint8_t fq_zero;
};

struct CrTask {
  uint64_t from, to;  // node references: where the walk starts (already turned for a left extension), the node behind the gap
  uint64_t off;       // its range of path entries starts here
  uint32_t cap;       // ... and holds this many
  uint32_t gmin, limit, kind;  // gap_min; gap_max or the extension's limit; kCrGap / kCrLeft / kCrRight
};
// What a walk leaves: nfront entries at the front of the task's range and nback at its end, which read in this order
// are the nodes that fill the gap (or extend the end) in the read's direction; codes holds the base each one prints.
struct CrRes { uint32_t nfront, nback, ok, pad; };

__device__ __forceinline__ uint64_t cr_len(const CrView &x, uint64_t r) { return x.boff[r + 1] - x.boff[r] - x.sep; }

// f(i, ref) for every aligned k-mer of a read in order, the same call in every lane of the wave (which is whole)
template <class F> __device__ __forceinline__ void cr_for_aligned(const CrView &x, uint64_t p0, uint64_t nk, uint32_t lane, F &&f)
{
  for (uint64_t i0 = 0; i0 < nk; i0 += 64) {
    const uint64_t i = i0 + lane;
    const unsigned long long ref = i < nk ? x.node[p0 + i] : kCrNone;
    unsigned long long m = __builtin_amdgcn_ballot_w64(ref != kCrNone);
    while (m) {
      const int s = __builtin_ctzll(m);
      m &= m - 1;
      f(i0 + (uint64_t)s, (uint64_t)__shfl(ref, s));
    }
  }
}

// gap_min and gap_max of a gap of `est` k-mers (correct_alignment_nxt:420-438): the wiggle in float arithmetic, the
// product and the sum rounded one after the other as C rounds them
__device__ __forceinline__ void cr_bounds(uint64_t est, float D, float d, uint32_t &gmin, uint32_t &gmax)
{
  float wf = __fadd_rn(__fmul_rn((float)est, D), d);
  wf = fminf(wf, 1073741824.f);
  const uint64_t wig = (uint64_t)(long long)wf;
  gmin = (uint32_t)(est > wig ? min(est - wig, (uint64_t)0x7ffffff0u) : 0u);
  gmax = (uint32_t)min(est + wig, (uint64_t)0x7ffffff0u);
}

// A wave per read.  WRITE = false: ntask[r] and ncap[r]; WRITE = true: the tasks at tasks[toff[r]], their ranges from
// coff[r] on, and the counters of the alignment.  Task order: the left extension, the gaps in read order, the right
// extension.  ENDS = false (`thread`, mcx_thread.h): the gaps alone, no extension is made a task or counted.
template <bool WRITE, bool ENDS = true>
__global__ __launch_bounds__(256) void k_cr_tasks(CrView x, TableView t, uint64_t *ntask, uint64_t *ncap, const uint64_t *toff, const uint64_t *coff,
                                                  CrTask *tasks, unsigned long long *ctr)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  unsigned long long c_perfect = 0, c_none = 0, c_gaps = 0, c_miss = 0, c_end = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < x.nreads; r += nwaves) {
    const uint64_t len = cr_len(x, r), p0 = x.boff[r] - x.boff[0], k = (uint64_t)x.k;
    const uint64_t nk = len >= k ? len - k + 1 : 0;
    uint64_t nt = 0, nc = 0, prev = 0, prevref = 0, ngaps = 0, nmiss = 0, first = kCrNone;
    auto add = [&](uint32_t kind, uint64_t from, uint64_t to, uint32_t gmin, uint32_t limit, uint32_t cap) {
      if (!ENDS && kind != kCrGap) return;
      if (WRITE && lane == 0) tasks[toff[r] + nt] = CrTask{from, to, coff[r] + nc, cap, gmin, limit, kind};
      nt++;
      nc += cap;
    };
    cr_for_aligned(x, p0, nk, lane, [&](uint64_t i, uint64_t ref) {
      if (first == kCrNone) {
        first = i;
        if (i > 0) add(kCrLeft, ref ^ 1ull, kCrNone, 0, (uint32_t)min(i, (uint64_t)0x7ffffff0u), (uint32_t)min(i, (uint64_t)0x7ffffff0u));
      } else if (i != prev + 1) {
        uint32_t gmin, gmax;
        cr_bounds(i - prev, x.D, x.d, gmin, gmax);
        add(kCrGap, prevref, ref, gmin, gmax, gmax + 2u);
        ngaps++;
      } else if (WRITE) {  // db_alignment_next_gap:166-173: do the union edges of the earlier k-mer hold the edge to this one
        uint32_t e = 0;
        for (uint32_t c = lane; c < x.ncols; c += 64) e |= (uint32_t)*val_ptr(t, prevref >> 1, c) & 0xffu;
        for (int dd = 32; dd >= 1; dd >>= 1) e |= __shfl_xor(e, dd);
        const uint32_t nuc = base_code(x.seq[p0 + i + k - 1]);
        if (!((e >> (4u * (uint32_t)(prevref & 1u) + nuc)) & 1u)) nmiss++;
      }
      prev = i;
      prevref = ref;
    });
    uint64_t right = 0;
    if (first != kCrNone) {
      right = len - (prev + k);
      if (right > 0) add(kCrRight, prevref, kCrNone, 0, (uint32_t)min(right, (uint64_t)0x7ffffff0u), (uint32_t)min(right, (uint64_t)0x7ffffff0u));
    }
    if (!WRITE) {
      if (lane == 0) { ntask[r] = nt; ncap[r] = nc; }
    } else if (lane == 0) {
      if (first == kCrNone) c_none++;
      else if (ngaps == 0 && first == 0 && right == 0) { c_perfect++; c_miss += nmiss ? 1 : 0; }  // correct_alignment_init:81-86
      else { c_miss += nmiss; c_gaps += ngaps; c_end += ENDS ? (first > 0) + (right > 0) : 0; }
    }
  }
  if (WRITE) {
    block_add(&ctr[kCrPerfect], c_perfect);
    block_add(&ctr[kCrNoKmers], c_none);
    block_add(&ctr[kCrGaps], c_gaps);
    block_add(&ctr[kCrMissing], c_miss);
    block_add(&ctr[kCrEndGaps], c_end);
  }
}

// ---- the walk --------------------------------------------------------------------------------------------------------
template <int W> struct CrWalker {
  Kmer<W> key;
  uint64_t slot;
  uint32_t o, n;  // orientation; nodes kept so far
  bool use;
};
template <int W> __device__ __forceinline__ void cr_walker_init(const TableView &t, CrWalker<W> &w, uint64_t ref, bool use)
{
  w.slot = ref >> 1;
  w.o = (uint32_t)(ref & 1u);
  w.n = 0;
  w.use = use;
  if (use) w.key = cl_key<W>(t, w.slot);
  else for (int i = 0; i < W; i++) w.key.w[i] = 0;
}
template <int W> __device__ __forceinline__ uint64_t cr_ref(const CrWalker<W> &w) { return (w.slot << 1) | w.o; }

// the key and the orientation of the neighbour of (key, o) over nucleotide x (cl_next without the lookup)
template <int W> __device__ __forceinline__ Kmer<W> cr_neighbour(const Kmer<W> &key, uint32_t o, uint32_t x, int k, uint32_t &p)
{
  Kmer<W> nb = key;
  if (o == 0) kmer_push<W>(nb, x, k);
  else kmer_push_front<W>(nb, 3u - x, k);
  const Kmer<W> rc = revcomp<W>(nb, k);
  const bool fw = kmer_less<W>(nb, rc);
  p = o ^ (fw ? 0u : 1u);
  return fw ? nb : rc;
}
// first and last base of the oriented node (key, o)
template <int W> __device__ __forceinline__ uint32_t cr_last_nuc(const Kmer<W> &key, uint32_t o, int k)
{
  return o == 0 ? (uint32_t)key.w[W - 1] & 3u : 3u - kmer_first_base<W>(key, k);
}
template <int W> __device__ __forceinline__ uint32_t cr_first_nuc(const Kmer<W> &key, uint32_t o, int k)
{
  return o == 0 ? kmer_first_base<W>(key, k) : 3u - ((uint32_t)key.w[W - 1] & 3u);
}

// One step of walker w by the four lanes of its group (sub = this lane's candidate nucleotide).  EVERY lane of the wave
// makes the call, `act` or not: the votes and the sums cross lanes.  The walker moves only when the step is kept; what
// stopped it otherwise is returned in `stop`.  path[i * dir], i < w.n, are the nodes the walk has kept.
template <int W>
__device__ __forceinline__ bool cr_step(const TableView &t, int k, uint32_t ncols, uint32_t colour, bool only_in_col, bool act, uint32_t lane,
                                        CrWalker<W> &w, const uint64_t *path, int dir, uint32_t &stop)
{
  const uint32_t sub = lane & 3u, g0 = lane & ~3u;
  uint32_t e = 0;
  if (act)
    for (uint32_t c = sub; c < ncols; c += 4) e |= (uint32_t)*val_ptr(t, w.slot, c) & 0xffu;
  e |= __shfl_xor(e, 1);
  e |= __shfl_xor(e, 2);
  uint64_t nslot = kNoSlot;
  bool ins = false;
  if (act && ((e >> (4u * w.o + sub)) & 1u)) {
    uint32_t p, novel = 0, full = 0;
    const Kmer<W> nk = cr_neighbour<W>(w.key, w.o, sub, k, p);
    nslot = find_or_insert_rec<W>(t, nk, true, novel, full);  // must_exist: read-only
    if (nslot != kNoSlot) ins = *val_ptr(t, nslot, colour) != 0;
  }
  const uint32_t F = (uint32_t)(__builtin_amdgcn_ballot_w64(nslot != kNoSlot) >> g0) & 15u;
  const uint32_t S = (uint32_t)(__builtin_amdgcn_ballot_w64(ins) >> g0) & 15u;
  int choice = -1;
  bool pop = false;
  stop = kCrStopNone;
  if (F == 0) stop = kCrStopDead;
  else if ((F & (F - 1u)) == 0) { choice = __builtin_ctz(F); pop = S == 0; }
  else if (S != 0 && (S & (S - 1u)) == 0) choice = __builtin_ctz(S);
  else stop = kCrStopFork;
  const uint64_t cslot = (uint64_t)__shfl((unsigned long long)nslot, (int)g0 + (choice < 0 ? 0 : choice));
  bool kept = act && choice >= 0;
  if (kept && only_in_col && pop) { stop = kCrStopColour; kept = false; }
  uint32_t p = 0, seen = 0;
  Kmer<W> nk = w.key;
  if (kept) {
    nk = cr_neighbour<W>(w.key, w.o, (uint32_t)choice, k, p);
    const uint64_t ref = (cslot << 1) | p;
    for (uint32_t i = sub; i < w.n; i += 4) seen += path[(int64_t)i * dir] == ref;
  }
  seen += __shfl_xor(seen, 1);
  seen += __shfl_xor(seen, 2);
  if (kept && seen >= 2) { stop = kCrStopRepeat; kept = false; }
  if (!act) stop = kCrStopNone;
  if (kept) { w.key = nk; w.slot = cslot; w.o = p; }
  return kept;
}

// Four lanes per task.  refs and codes hold the tasks' ranges: refs the nodes kept (what the third-entry test reads),
// codes the base each prints.  A gap is walked one way (forward from the node before it, then, if that fails, from the
// reverse of the node behind it: traverse_one_way) or, with kCrTwoWay, by two walkers stepping in turn
// (traverse_two_way2:208-236).  Walker 0 keeps its nodes from the front of the range, walker 1 from its end backwards.
template <int W>
__global__ __launch_bounds__(256) void k_cr_walk(TableView t, int k, uint32_t ncols, uint32_t colour, uint32_t flags, const CrTask *tasks, uint64_t ntasks,
                                                 uint64_t *refs, uint8_t *codes, CrRes *res, unsigned long long *ctr)
{
  const uint32_t lane = threadIdx.x & 63u, sub = lane & 3u;
  const uint64_t per_block = blockDim.x >> 2;
  unsigned long long c_fill = 0, c_back = 0, c_short = 0, c_long = 0, c_fork = 0, c_col = 0, c_rep = 0, c_ext = 0, c_steps = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < ntasks; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t ti = base + (threadIdx.x >> 2);
    bool live = ti < ntasks;
    CrTask T{0, 0, 0, 0, 0, 0, kCrRight};
    if (live) T = tasks[ti];
    const bool gap = T.kind == kCrGap, two = gap && (flags & kCrTwoWay);
    const uint32_t maxlen = gap ? T.limit + 1u : T.limit;  // nodes a one-way walk or an extension keeps at the most
    CrWalker<W> w0, w1;
    cr_walker_init<W>(t, w0, T.from, live && T.kind != kCrLeft);
    cr_walker_init<W>(t, w1, gap ? T.to ^ 1ull : T.from, live && (two || T.kind == kCrLeft));
    uint64_t *const r0 = refs + T.off, *const r1 = refs + T.off + (T.cap ? T.cap - 1u : 0u);
    uint8_t *const c0 = codes + T.off, *const c1 = codes + T.off + (T.cap ? T.cap - 1u : 0u);
    uint32_t turn = 0;
    bool reached = false, backward = false;
    while (__builtin_amdgcn_ballot_w64(live)) {  // (the same for the whole wave: cr_step crosses lanes)
      // which walker steps now, if any
      bool step1 = false, act = false;
      if (live) {
        if (two) {
          if (turn == 0 && !(w0.n + w1.n <= T.limit && (w0.use || w1.use))) live = false;
          step1 = turn == 1;
          act = live && (step1 ? w1.use : w0.use);
          turn ^= 1u;
        } else {
          step1 = !w0.use;
          if ((step1 ? w1.n : w0.n) >= maxlen) {  // the walk ran out of room
            if (gap && !step1) { w0.use = false; w0.n = 0; cr_walker_init<W>(t, w1, T.to ^ 1ull, true); backward = true; }
            else live = false;
          } else act = true;
        }
      }
      CrWalker<W> w = step1 ? w1 : w0;
      uint32_t stop;
      const bool kept = cr_step<W>(t, k, ncols, colour, gap, act, lane, w, step1 ? r1 : r0, step1 ? -1 : 1, stop);
      if (!act) continue;
      if (sub == 0) { c_steps++; c_fork += stop == kCrStopFork; c_col += stop == kCrStopColour; c_rep += stop == kCrStopRepeat; }
      if (kept) {
        if (step1) w1 = w; else w0 = w;
        const uint64_t here = cr_ref(w);
        bool met;
        if (two) met = cr_ref(w0) == (cr_ref(w1) ^ 1ull);
        else met = gap && here == (step1 ? T.from ^ 1ull : T.to);
        if (met) {
          reached = two ? w0.n + w1.n <= T.limit : true;
          if (two) live = false;
          else if (step1 || w0.n >= T.gmin) live = false;
          else { w0.use = false; w0.n = 0; reached = false; cr_walker_init<W>(t, w1, T.to ^ 1ull, true); backward = true; }  // too short: the other way
        } else {
          const uint32_t n = step1 ? w1.n : w0.n;
          // entry n is stored by lane n % 4 of the group, the lane that cr_step has read it: a lane reads its own stores
          if (w0.n + w1.n < T.cap && sub == (n & 3u)) {
            if (step1) {
              r1[-(int64_t)n] = here;
              c1[-(int64_t)n] = (uint8_t)(3u - (T.kind == kCrLeft ? cr_last_nuc<W>(w.key, w.o, k) : cr_first_nuc<W>(w.key, w.o, k)));
            } else {
              r0[n] = here;
              c0[n] = (uint8_t)cr_last_nuc<W>(w.key, w.o, k);
            }
          }
          if (step1) w1.n++; else w0.n++;
        }
      } else if (two) {
        if (step1) w1.use = false; else w0.use = false;
        if (stop == kCrStopRepeat) { w0.use = false; w1.use = false; }
      } else if (gap && !step1) {  // the forward walk failed: the other way
        w0.use = false;
        w0.n = 0;
        cr_walker_init<W>(t, w1, T.to ^ 1ull, true);
        backward = true;
      } else live = false;
    }
    if (ti < ntasks && sub == 0) {
      const uint32_t glen = w0.n + w1.n;
      const bool ok = gap ? reached && glen >= T.gmin : true;
      res[ti] = CrRes{w0.n, w1.n, ok ? 1u : 0u, 0u};
      if (gap) {
        if (ok) { c_fill++; c_back += backward; }
        else if (glen < T.gmin) c_short++;
        else c_long++;
      } else c_ext += glen > 0;
    }
  }
  block_add(&ctr[kCrFilled], c_fill);
  block_add(&ctr[kCrFilledBack], c_back);
  block_add(&ctr[kCrTooShort], c_short);
  block_add(&ctr[kCrTooLong], c_long);
  block_add(&ctr[kCrFork], c_fork);
  block_add(&ctr[kCrColour], c_col);
  block_add(&ctr[kCrRepeat], c_rep);
  block_add(&ctr[kCrEndExt], c_ext);
  block_add(&ctr[kCrSteps], c_steps);
}

// ---- the records ----------------------------------------------------------------------------------------------------
// handle_read2 for read r by a whole wave, every lane with the same control flow: the sequence's length.  With EMIT the
// sequence goes to out and, when the batch has qualities, the qualities to out + qoff: those of the read's own bases,
// fq_zero for a base that a walk supplied.  nfill += the bases supplied.
template <bool EMIT>
__device__ __forceinline__ uint64_t cr_render(const CrView &x, const CrTask *tasks, const CrRes *res, const uint8_t *codes, uint64_t tk, uint64_t r,
                                              uint32_t lane, uint8_t *out, uint64_t qoff, uint64_t &nfill)
{
  const uint64_t len = cr_len(x, r), p0 = x.boff[r] - x.boff[0], k = (uint64_t)x.k;
  const uint64_t nk = len >= k ? len - k + 1 : 0;
  uint64_t o = 0, printed = 0, first = kCrNone, a = 0, prev = 0;
  auto put_read = [&](uint64_t s, uint64_t e, bool upper) {  // strbuf_append_strn_uc / _lc of the read's [s, e)
    if (e <= s) return;
    if (EMIT)
      for (uint64_t j = lane; j < e - s; j += 64) {
        uint8_t c = x.seq[p0 + s + j];
        if (upper) { if (c >= 'a' && c <= 'z') c -= 32; }
        else if (c >= 'A' && c <= 'Z') c += 32;
        out[o + j] = c;
        if (x.qual) out[qoff + o + j] = x.qual[p0 + s + j];
      }
    o += e - s;
  };
  auto put_fill = [&](const CrTask &T, const CrRes &R, uint64_t n) {  // the first n nodes of the task's result
    if (EMIT)
      for (uint64_t j = lane; j < n; j += 64) {
        const uint64_t at = j < R.nfront ? j : (uint64_t)T.cap - R.nback + (j - R.nfront);
        out[o + j] = (uint8_t)"ACGT"[codes[T.off + at] & 3u];
        if (x.qual) out[qoff + o + j] = x.fq_zero;
      }
    o += n;
    nfill += n;
  };
  auto put_run = [&](uint64_t s, uint64_t e) {  // _print_read_kmer for the k-mers at s .. e, which are consecutive
    if (s > printed) { put_read(printed, s, false); printed = s; }
    if (e + k > printed) put_read(printed, e + k, true);
    printed = e + k;
  };
  cr_for_aligned(x, p0, nk, lane, [&](uint64_t i, uint64_t) {
    if (first == kCrNone) {
      first = i;
      uint64_t nl = 0;
      if (i > 0) {
        const CrTask T = tasks[tk];
        const CrRes R = res[tk];
        tk++;
        nl = R.nback;
        put_read(0, i - nl, false);
        put_fill(T, R, nl);
      }
      printed = i;
      a = i;
    } else if (i != prev + 1) {
      put_run(a, prev);
      const CrTask T = tasks[tk];
      const CrRes R = res[tk];
      tk++;
      if (R.ok) {  // handle_read2:170-194
        const uint64_t neg = (uint64_t)R.nfront + R.nback, exp = i - prev - 1;
        uint64_t nprint = 0;
        if (neg >= k) nprint = neg - k + 1;
        if (neg > exp) nprint = neg - exp;
        put_fill(T, R, nprint);
        uint64_t nextpos = i;
        if (neg < k) nextpos += k - neg - 1;
        if (neg > 0 && nextpos > printed) printed = nextpos;
      }
      a = i;
    }
    prev = i;
  });
  if (first == kCrNone) { put_read(0, len, false); return o; }
  put_run(a, prev);
  if (len > prev + k) {
    const CrTask T = tasks[tk];
    const CrRes R = res[tk];
    put_fill(T, R, R.nfront);
    printed += R.nfront;
  }
  put_read(printed, len, false);
  return o;
}

// len[r] = the bytes of record r: the sequence, and as many qualities when the batch has them
__global__ __launch_bounds__(256) void k_cr_len(CrView x, const CrTask *tasks, const CrRes *res, const uint64_t *toff, uint64_t *len, unsigned long long *ctr)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  unsigned long long c_fill = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < x.nreads; r += nwaves) {
    uint64_t nfill = 0;
    const uint64_t n = cr_render<false>(x, tasks, res, nullptr, toff[r], r, lane, nullptr, 0, nfill);
    if (lane == 0) { len[r] = x.qual ? 2 * n : n; c_fill += nfill; }
  }
  block_add(&ctr[kCrBasesFilled], c_fill);
}

__global__ __launch_bounds__(256) void k_cr_emit(CrView x, const CrTask *tasks, const CrRes *res, const uint8_t *codes, const uint64_t *toff,
                                                 const uint64_t *out_off, uint8_t *out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t r = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < x.nreads; r += nwaves) {
    uint64_t nfill = 0;
    const uint64_t bytes = out_off[r + 1] - out_off[r];
    (void)cr_render<true>(x, tasks, res, codes, toff[r], r, lane, out + out_off[r], x.qual ? bytes / 2 : 0, nfill);
  }
}

}  // namespace mcx
