// mcx_reads.h -- `reads` on the device (included by mcx_api.hip).
//
// read_touches_graph (src/commands/ctx_reads.c) over a batch of reads: a read touches the graph iff one of its k-mers
// is a key of the table.  The k-mers of a read are those of its maximal ACGTacgt runs of at least k bases; there is no
// quality or homopolymer cutoff, the lookup is by canonical key and colours play no part.  Two passes (DESIGN.md
// section 4, "reads' device passes"):
//   A. k_rt_probe   the batch's stream, tile by tile as k_sg_seed walks it: canonical key, read-only lookup, four in flight per lane; a lane hands
//                   the 16 outcomes of its 16 start positions to the sink.  The mask sink stores them as one 16-bit word
//                   (position P = bit P % 16 of word P / 16, so the words of a batch are a little-endian bit array
//                   indexed by stream position): 128 contiguous bytes per wave, no atomics, zeros included.
//   B. k_rt_reads   read i = stream positions [off[i], off[i + 1] - 1); ORs the bits of its start positions
//                   [off[i], off[i + 1] - k) into one byte.
// The reference stops at a read's first hit; this pass probes every k-mer, which costs no more than finding out
// which reads are already decided, and makes the two counts (occurrences probed, occurrences found) exact.
// Both kernels are grid-stride loops (the "grid" knob caps the launches).
#pragma once
#include "mcx_kernels.h"

namespace mcx {

// Start positions above which a wave, not a lane, ORs a read's bits.  One coalesced wave load of 64-bit words covers
// 64 x 64 = 4096 positions: a shorter read cannot give every lane of that load a word, so a lane of its own is
// cheaper (short reads: 3 words at 150 bases); a longer one read by a single lane makes the other 63 wait for a walk
// of more than 64 dependent cache lines (a wave ends with its slowest lane), which a multi-megabase contig would
// stretch to tens of thousands.
constexpr uint64_t kRtLongStarts = 4096;

// What a lane hands to the sink of rt_probe for its 16 start positions P0 .. P0 + 15: hit16 has position P0 + j at bit
// j.  A sink that sets kSlots also receives, per position, the slot of the k-mer (kNoSlot where hit16 has no bit) and
// in o16 bit j the orientation canonical<W> returned for it (1: the key is the reverse complement of the read's k-mer);
// for a sink that does not, the two are not computed (slot[] holds nothing) and the walk is the one `reads` always had.
// The sink of `reads`: one 16-bit word per lane.  `coverage` passes a sink of its own (mcx_coverage.h).
struct RtMaskSink {
  static constexpr bool kSlots = false;
  uint16_t *hit;
  __device__ __forceinline__ void operator()(uint64_t P0, uint32_t hit16, const uint64_t (&)[16], uint32_t) const { hit[P0 >> 4] = (uint16_t)hit16; }
};

constexpr int kRtBatch = 4;  // lookups in flight per lane (divides 16), as k_stream's kBatch: the first probes are independent loads

// Whether `key` is in the table, given `cur`, the word read at the key's first slot.  An empty first slot ends the
// probe sequence and a one-word key that equals it is found -- the two common outcomes, and what
// find_or_insert_rec(must_exist) returns for them; everything else is left to that function from the start (its loads
// of the first slot then hit the cache).
template <int W> __device__ __forceinline__ bool rt_found(const TableView &t, const Kmer<W> &key, uint64_t cur)
{
  if (cur == 0) return false;
  if (W == 1 && cur == (key.w[0] | kFlag)) return true;
  uint32_t novel = 0, full = 0;
  return find_or_insert_rec<W>(t, key, true, novel, full) != kNoSlot;  // must_exist: read-only
}

// The slot of `key` (kNoSlot: absent), given the word `cur` read at its first slot s0: rt_found's two shortcuts, with
// the slot kept.
template <int W> __device__ __forceinline__ uint64_t rt_find(const TableView &t, const Kmer<W> &key, uint64_t cur, uint64_t s0)
{
  if (cur == 0) return kNoSlot;
  if (W == 1 && cur == (key.w[0] | kFlag)) return s0;
  uint32_t novel = 0, full = 0;
  return find_or_insert_rec<W>(t, key, true, novel, full);  // must_exist: read-only
}

// cnt[0] += k-mer occurrences probed, cnt[1] += occurrences whose k-mer is in the table.  Every lane of every tile in
// [tile0, ntiles) calls the sink once, also with no k-mer start among its positions.
template <int W, class Sink>
__device__ __forceinline__ void rt_probe(const StreamArgs &a, const TableView &t, const Sink &sink, unsigned long long *cnt)
{
  __shared__ uint32_t s_code[kChunks + 4];
  __shared__ uint32_t s_inv[kChunks / 2 + 4];
  const int tid = threadIdx.x, k = a.k;
  const int topb = k - 32 * (W - 1);  // bases in the top word
  const int fs = 2 * topb - 2;        // bit position of base 0 in w[0]
  unsigned long long n_occ = 0, n_hit = 0;
  for (uint64_t tile = a.tile0 + blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    __syncthreads();
    {
      TileSrc ts;
      tile_fetch<false>(a, tile, tid, ts);
      tile_stage<false>(a, ts, tid, s_code, s_inv);
    }
    if (tid < 4) { s_code[kChunks + tid] = 0; s_inv[kChunks / 2 + tid] = 0xFFFFFFFFu; }
    __syncthreads();
    const uint32_t pl = 16u * (uint32_t)(tid + 1);  // region index of this lane's first position
    const uint64_t P0 = tile * kTile + 16ull * (uint64_t)tid;
    const int j_lo = a.pos_lo > P0 ? (int)min((uint64_t)kPosPerLane, a.pos_lo - P0) : 0;
    const int j_hi = a.pos_hi > P0 ? (int)min((uint64_t)kPosPerLane, a.pos_hi - P0) : 0;
    uint32_t ok16, nok16;
    lane_masks_wide(s_inv, pl, k, ok16, nok16);
    ok16 &= ((0x10000u >> j_lo) - 1u) & ~((0x10000u >> j_hi) - 1u);
    uint32_t hit16 = 0, o16 = 0;
    uint64_t slot[kPosPerLane];
    if constexpr (Sink::kSlots)
      for (int j = 0; j < kPosPerLane; j++) slot[j] = kNoSlot;
    if (ok16) {
      Kmer<W> fw, rc;
      fw.w[0] = code_win64(s_code, pl) >> (64 - 2 * topb);
      for (int i = 1; i < W; i++) fw.w[i] = code_win64(s_code, pl + (uint32_t)(topb + 32 * (i - 1)));
      rc = revcomp<W>(fw, k);
      const uint64_t feed = code_win64(s_code, pl + (uint32_t)k);
      for (int j0 = 0; j0 < kPosPerLane; j0 += kRtBatch) {
        Kmer<W> key[kRtBatch];
        uint64_t cur[kRtBatch], s0[kRtBatch];
        bool ov[kRtBatch];
#pragma unroll
        for (int b = 0; b < kRtBatch; b++) {  // issue the first probe of every k-mer of the batch before looking at any
          const int j = j0 + b;
          ov[b] = ((ok16 >> (15 - j)) & 1u) != 0;
          cur[b] = 0;
          if (ov[b]) {
            uint32_t o;
            key[b] = canonical<W>(fw, rc, o);
            const uint64_t s = key_slot<W>(t, key[b]);
            cur[b] = __hip_atomic_load(key_ptr(t, s), MCX_RLX, MCX_AGENT);
            if constexpr (Sink::kSlots) { s0[b] = s; o16 |= o << j; }
          }
          const uint32_t nuc_next = (uint32_t)(feed >> (62 - 2 * j)) & 3u;
          kmer_push<W>(fw, nuc_next, k);
          for (int i = W - 1; i >= 1; i--) rc.w[i] = (rc.w[i] >> 2) | (rc.w[i - 1] << 62);
          rc.w[0] = (rc.w[0] >> 2) | ((uint64_t)(3u - nuc_next) << fs);
        }
#pragma unroll
        for (int b = 0; b < kRtBatch; b++)
          if (ov[b]) {
            n_occ++;
            if constexpr (Sink::kSlots) {
              slot[j0 + b] = rt_find<W>(t, key[b], cur[b], s0[b]);
              if (slot[j0 + b] != kNoSlot) hit16 |= 1u << (j0 + b);
            } else {
              if (rt_found<W>(t, key[b], cur[b])) hit16 |= 1u << (j0 + b);
            }
          }
      }
    }
    n_hit += (unsigned long long)__popc(hit16);
    sink(P0, hit16, slot, o16);
  }
  block_add(&cnt[0], n_occ);
  block_add(&cnt[1], n_hit);
}

template <int W> __global__ __launch_bounds__(kThreads) void k_rt_probe(StreamArgs a, TableView t, uint16_t *hit, unsigned long long *cnt)
{
  rt_probe<W>(a, t, RtMaskSink{hit}, cnt);
}

// What a sink of rt_probe left per stream position of a chunk, placed by base position (k_cv_place, k_cr_place; host
// entries only).  The chunk holds n reads (or one piece of a read): read i of it sits at the chunk's stream positions
// [so[i], so[i + 1] - 1) and is read r0 + i of the batch.  Of every read the first `own` positions (all of them when
// own = ~0, Chunk::own of mcx_chunk.h) go to the batch's arrays at base position boff[r0 + i] - boff[0] + shift: the
// separators drop out, a piece of a long read lands behind the one before it.  copy(p, d) moves stream position p
// (< spitch) to base position d (< pitch).  One thread per stream position finds its read by bisection (the lanes of a
// wave mostly meet the same few offsets).
template <class Copy>
__device__ __forceinline__ void rt_place(const uint64_t *so, uint64_t n, const uint64_t *boff, uint64_t r0, uint64_t shift, uint64_t own,
                                         uint64_t spitch, uint64_t pitch, const Copy &copy)
{
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, np = so[n];
  const uint64_t b0 = boff[0];
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < np; p += stride) {
    uint64_t lo = 0, hi = n;  // the last i with so[i] <= p
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (so[mid] <= p) lo = mid; else hi = mid;
    }
    const uint64_t q = p - so[lo], len = so[lo + 1] - so[lo] - 1;
    if (q >= (own < len ? own : len)) continue;  // the separator, or the tail that the next piece owns
    const uint64_t d = boff[r0 + lo] - b0 + shift + q;
    if (d >= pitch || p >= spitch) continue;
    copy(p, d);
  }
}

// bits [s, e) of the bit array `m` that fall into its 64-bit word w (s < e, w in [s / 64, (e - 1) / 64])
__device__ __forceinline__ uint64_t rt_word(const uint64_t *m, uint64_t w, uint64_t s, uint64_t e)
{
  uint64_t v = m[w];
  if (w == (s >> 6)) v &= ~0ull << (s & 63u);
  if (w == ((e - 1) >> 6) && (e & 63u)) v &= ~0ull >> (64u - (e & 63u));
  return v;
}

// hit[i] = 1 iff a start position of read i has its bit set.  `mask` holds npos bits (a multiple of 64: whole tiles);
// a range that leaves them is cut short, so offsets that do not describe the stream cannot make the kernel read
// outside the array.  The first and the last word of a read are masked to its own start positions: the bits of the
// neighbouring reads in the same word never count.  A read of more than kRtLongStarts start positions is taken by the
// whole wave of the lane that met it.
__global__ __launch_bounds__(256) void k_rt_reads(const uint64_t *mask, uint64_t npos, const uint64_t *off, uint64_t nreads, int k,
                                                  uint8_t *hit)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < nreads; base += stride) {
    const uint64_t i = base + threadIdx.x;
    uint64_t s = 0, e = 0;
    if (i < nreads) {
      s = off[i];
      const uint64_t nx = off[i + 1];
      e = nx > (uint64_t)k ? min(nx - (uint64_t)k, npos) : 0;
      if (e <= s) s = e = 0;
    }
    const bool is_long = e - s > kRtLongStarts;
    uint64_t acc = 0;
    if (e > s && !is_long)
      for (uint64_t w = s >> 6; w <= ((e - 1) >> 6) && !acc; w++) acc = rt_word(mask, w, s, e);
    unsigned long long todo = __builtin_amdgcn_ballot_w64(is_long);  // (uniform per wave)
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint64_t ls = __shfl((unsigned long long)s, src), le = __shfl((unsigned long long)e, src);
      uint64_t part = 0;
      for (uint64_t w0 = ls >> 6; w0 <= ((le - 1) >> 6); w0 += 64) {
        const uint64_t w = w0 + lane;
        if (w <= ((le - 1) >> 6)) part |= rt_word(mask, w, ls, le);
        if (__builtin_amdgcn_ballot_w64(part != 0)) break;
      }
      const bool any = __builtin_amdgcn_ballot_w64(part != 0) != 0;
      if ((int)lane == src) acc = any ? 1 : 0;
    }
    if (i < nreads) hit[i] = acc ? 1 : 0;
  }
}

}  // namespace mcx
