// mcx_subgraph.h -- `subgraph` on the device (included by mcx_api.hip).
//
// subgraph_from_reads (src/tools/subgraph.c) over the table: mark the seed k-mers that are in the graph, extend the
// marked set breadth first over the union of the colours' edges, then prune what is not marked
// (prune_nodes_lacking_flag, src/graph/prune_nodes.c).  Steps ("subgraph's device passes"):
//   A. k_sg_seed     a seed stream, tile by tile as k_stream walks it: canonical key, read-only lookup, mark, enqueue
//                    (--unitigs: flag the k-mer's unitig instead; k_sg_grab then marks and enqueues whole unitigs)
//   B. k_sg_expand   one level of a wide frontier, one lane per (entry, edge); the last block to finish advances the queue
//      k_sg_narrow   one workgroup, many levels of a narrow frontier in one launch
//   C. k_sg_prune_edges, k_sg_tombstone   clean's prune bodies (cl_prune_edges, cl_tombstone) with keep = mark bit XOR
//                    invert per k-mer
// State: the dense ids of k_cl_compact (mcx_clean.h), a mark bitset in 32-bit words, ONE queue of n dense ids and a
// control block.  A k-mer is enqueued by the lane whose atomicOr found its bit clear, so at most once: n entries
// cannot overflow, and the frontier of a level is the window queue[head, tail) of that array.
// Every kernel is a grid-stride loop (the "grid" knob caps the launches).
#pragma once
#include "mcx_clean.h"

namespace mcx {

constexpr int kSgBlock = 256;  // threads of k_sg_narrow's one workgroup = the largest frontier it takes
// control block (32-bit words in device memory)
enum : uint32_t {
  kSgHead = 0,   // the frontier is queue[head, tail)
  kSgTail = 1,
  kSgWtail = 2,  // where the next entry goes (>= tail)
  kSgLevel = 3,  // levels run
  kSgAdded = 4,  // levels that added k-mers
  kSgMaxF = 5,   // largest frontier
  kSgDone = 6,   // blocks of the running k_sg_expand that have finished
  kSgOver = 7,   // an entry did not fit the queue (a k-mer enqueued twice: never, unless the ids are stale)
  kSgCtlWords = 8
};

struct SgView {
  const uint64_t *slot_of;  // dense id -> slot
  const uint32_t *map;      // slot -> dense id
  const uint8_t *ue;        // union edges
  uint32_t *mark, *queue, *ctl;
  uint64_t n;
};

// set the k-mer's bit; true for the one caller that found it clear
__device__ __forceinline__ bool sg_mark(uint32_t *mark, uint32_t id)
{
  const uint32_t bit = 1u << (id & 31u);
  return !(atomicOr(&mark[id >> 5], bit) & bit);
}

// append the ids of the pushing lanes behind *cursor: one reservation per wave (every lane of the wave calls this)
__device__ __forceinline__ void sg_push(const SgView &s, uint32_t *cursor, bool push, uint32_t id)
{
  const uint64_t at = wave_append(cursor, push);
  if (!push) return;
  if (at < s.n) s.queue[at] = id;
  else s.ctl[kSgOver] = 1u;
}

// the frontier that was expanded is done: the entries appended meanwhile are the next one
__device__ __forceinline__ void sg_advance(uint32_t *c, uint32_t wtail, bool count_level)
{
  const uint32_t tail = c[kSgTail], f = wtail - tail;
  c[kSgHead] = tail;
  c[kSgTail] = wtail;
  if (count_level) {
    c[kSgLevel]++;
    if (f) c[kSgAdded]++;
  }
  if (f > c[kSgMaxF]) c[kSgMaxF] = f;
}

// the seeds are in: they are the first frontier (level 0)
__global__ void k_sg_open(uint32_t *ctl)
{
  if (blockIdx.x == 0 && threadIdx.x == 0) sg_advance(ctl, ctl[kSgWtail], false);
}

// A seed stream.  cnt[0] += k-mer occurrences (stats.num_kmers_loaded of the reference), cnt[1] += k-mers newly marked.
// With uflag the k-mer's unitig is flagged instead and nothing is marked (k_sg_grab does that).  The stream is ASCII:
// no entry of the interface hands over packed seeds.
template <int W>
__global__ __launch_bounds__(kThreads) void k_sg_seed(StreamArgs a, TableView t, SgView s, const uint32_t *uid, uint8_t *uflag,
                                                      unsigned long long *cnt)
{
  __shared__ uint32_t s_code[kChunks + 4];
  __shared__ uint32_t s_inv[kChunks / 2 + 4];
  const int tid = threadIdx.x, k = a.k;
  const int topb = k - 32 * (W - 1);  // bases in the top word
  const int fs = 2 * topb - 2;        // bit position of base 0 in w[0]
  unsigned long long n_occ = 0, n_new = 0;
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
    if (!__builtin_amdgcn_ballot_w64(ok16 != 0)) continue;  // (per wave: sg_push needs the whole wave)
    Kmer<W> fw, rc;
    fw.w[0] = code_win64(s_code, pl) >> (64 - 2 * topb);
    for (int i = 1; i < W; i++) fw.w[i] = code_win64(s_code, pl + (uint32_t)(topb + 32 * (i - 1)));
    rc = revcomp<W>(fw, k);
    const uint64_t feed = code_win64(s_code, pl + (uint32_t)k);
    for (int j = 0; j < kPosPerLane; j++) {
      bool push = false;
      uint32_t id = 0;
      if ((ok16 >> (15 - j)) & 1u) {
        n_occ++;
        uint32_t o, novel = 0, full = 0;
        const Kmer<W> key = canonical<W>(fw, rc, o);
        const uint64_t slot = find_or_insert_rec<W>(t, key, true, novel, full);  // must_exist: read-only
        if (slot != kNoSlot) {
          id = s.map[slot];
          if (uflag) uflag[uid[id]] = 1;
          else push = sg_mark(s.mark, id);
        }
      }
      n_new += push;
      sg_push(s, &s.ctl[kSgWtail], push, id);
      const uint32_t nuc_next = (uint32_t)(feed >> (62 - 2 * j)) & 3u;
      kmer_push<W>(fw, nuc_next, k);
      for (int i = W - 1; i >= 1; i--) rc.w[i] = (rc.w[i] >> 2) | (rc.w[i - 1] << 62);
      rc.w[0] = (rc.w[0] >> 2) | ((uint64_t)(3u - nuc_next) << fs);
    }
  }
  block_add(&cnt[0], n_occ);
  block_add(&cnt[1], n_new);
}

// --unitigs: every k-mer of a flagged unitig is marked and enqueued (db_unitig_fetch of mark_unitig)
__global__ __launch_bounds__(256) void k_sg_grab(SgView s, const uint32_t *uid, const uint8_t *uflag, unsigned long long *cnt)
{
  unsigned long long n_new = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < s.n; base += cl_stride()) {
    const uint64_t i = base + threadIdx.x;
    const bool push = i < s.n && uflag[uid[i]] && sg_mark(s.mark, (uint32_t)i);
    n_new += push;
    sg_push(s, &s.ctl[kSgWtail], push, (uint32_t)i);
  }
  block_add(&cnt[1], n_new);
}

// item i of a frontier that starts at queue[head]: entry i / 8 over edge bit i % 8 (store_node_neighbours).  True when
// this lane marked the neighbour; a neighbour that is not in the table is passed over, as k_cl_prune_edges does.
template <int W>
__device__ __forceinline__ bool sg_visit(const TableView &t, int k, const SgView &s, uint32_t head, uint64_t i, uint32_t &id2)
{
  const uint32_t id = s.queue[head + (uint32_t)(i >> 3)], b = (uint32_t)i & 7u;
  if (!((s.ue[id] >> b) & 1u)) return false;
  uint32_t p = 0;
  const uint64_t slot = cl_next<W>(t, cl_key<W>(t, s.slot_of[id]), b >> 2, b & 3u, k, p);
  if (slot == kNoSlot) return false;
  id2 = s.map[slot];
  return sg_mark(s.mark, id2);
}

// One level of a wide frontier.  Every block reads head, tail and the level from device memory; the block that
// finishes last advances them (by then every other block has read them and has appended what it found).
template <int W> __global__ __launch_bounds__(256) void k_sg_expand(TableView t, int k, SgView s, uint32_t dist)
{
  const uint32_t head = s.ctl[kSgHead], tail = s.ctl[kSgTail];
  const bool run = s.ctl[kSgLevel] < dist && tail != head;
  if (run) {
    const uint64_t items = (uint64_t)(tail - head) * 8;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < items; base += cl_stride()) {
      const uint64_t i = base + threadIdx.x;
      uint32_t id2 = 0;
      const bool push = i < items && sg_visit<W>(t, k, s, head, i, id2);
      sg_push(s, &s.ctl[kSgWtail], push, id2);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(&s.ctl[kSgDone], 1u) == gridDim.x - 1u) {
      __threadfence();
      s.ctl[kSgDone] = 0;
      if (run) sg_advance(s.ctl, atomicAdd(&s.ctl[kSgWtail], 0u), true);
    }
  }
}

// Many levels of a narrow frontier: one workgroup, the control block in LDS, a barrier between levels.  Returns when
// `dist` levels have run, the frontier is empty or it holds more than `limit` entries.  __syncthreads() is a barrier and
// a workgroup-scope release / acquire fence, so the queue entries stored in level L by any wave of the block are read
// by every wave in level L + 1; the marks are device-scope atomics.  Nothing else runs on the stream meanwhile.
template <int W> __global__ __launch_bounds__(kSgBlock) void k_sg_narrow(TableView t, int k, SgView s, uint32_t dist, uint32_t limit)
{
  __shared__ uint32_t c[kSgCtlWords];
  if (threadIdx.x < kSgCtlWords) c[threadIdx.x] = s.ctl[threadIdx.x];
  __syncthreads();
  for (;;) {
    const uint32_t head = c[kSgHead], tail = c[kSgTail];
    if (c[kSgLevel] >= dist || tail == head || tail - head > limit) break;  // (the same for every thread)
    const uint32_t items = (tail - head) * 8;
    for (uint32_t base = 0; base < items; base += kSgBlock) {
      const uint32_t i = base + threadIdx.x;
      uint32_t id2 = 0;
      const bool push = i < items && sg_visit<W>(t, k, s, head, i, id2);
      sg_push(s, &c[kSgWtail], push, id2);
    }
    __syncthreads();  // the level's entries and the append cursor are complete
    if (threadIdx.x == 0) sg_advance(c, c[kSgWtail], true);
    __syncthreads();
  }
  if (threadIdx.x < kSgCtlWords && threadIdx.x != kSgOver) s.ctl[threadIdx.x] = c[threadIdx.x];
}

// The prune keeps the marked k-mers, or with `invert` the others.  clean's form (KeepUnitig) reads a byte per unitig
// behind a 4-byte id per k-mer; serving it an identity uid would cost 5 n bytes of scratch and a pass to unpack the bitset.
struct KeepMark {
  const uint32_t *mark;
  uint32_t invert;
  __device__ __forceinline__ bool operator()(uint64_t id) const { return (((mark[id >> 5] >> (id & 31u)) & 1u) ^ invert) != 0; }
};

template <int W>
__global__ __launch_bounds__(256) void k_sg_prune_edges(TableView t, int k, uint32_t ncols, SgView s, uint32_t invert)
{
  cl_prune_edges<W>(t, k, ncols, s.n, s.slot_of, s.map, s.ue, KeepMark{s.mark, invert});
}

__global__ __launch_bounds__(256) void k_sg_tombstone(TableView t, SgView s, uint32_t invert, Counters *ctr, unsigned long long *removed)
{
  cl_tombstone(t, s.n, s.slot_of, KeepMark{s.mark, invert}, ctr, removed);
}

}  // namespace mcx
