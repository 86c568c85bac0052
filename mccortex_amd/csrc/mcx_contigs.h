// mcx_contigs.h -- `contigs` on the device (included by mcx_api.hip behind mcx_links.h: it uses that file's line marking
// and the link store of the `thread` section).
//
// ctx_contigs.c: every seed k-mer is walked both ways by a GraphWalker that holds links (src/graph/graph_walker.c,
// src/tools/assemble_contigs.c:_assemble_contig without a seed link).  include/mcx_gpu.h restates the walker, the assembly
// and the seeding rule; tests/contigs_restate.py is the same in Python.  The graph view is that of `correct`: union
// edges, in the sample iff the value word of the colour is non-zero, AN EDGE THAT NAMES AN ABSENT K-MER COUNTS AS NO EDGE.
// The passes ("contigs' device passes"):
//   L. mcx_graph_links_load_text: the line marking of mcx_links.h (k_lk_mark, k_lk_starts, k_lk_class, k_lk_klines),
//      k_cg_kmers (a thread per k-mer line: canonical key, looked up read-only), k_cg_parse (a thread per line: the
//      columns of a link line, seq= and juncpos= ignored), k_lk_store (the junctions packed), k_cg_links (ThLink
//      records) and the sort and reduce of `thread` (th_sort_reduce, th_merge)
//   S. k_cg_flag, a scan, k_cg_slots and sort_perm_by_words: the keys in the sample in ascending key order; or
//      k_cg_seeds: the seed reads' keys looked up
//   W. k_cg_walk    four lanes per seed, one successor candidate each (the probes are cr_step's: cr_neighbour and the
//                   read-only find_or_insert_rec).  The held links, the counter links and the segments live in the walk's
//                   range of HBM scratch and are touched by the group's first lane alone, which hands the other three
//                   its decision; the nodes live in the walk's range of the node arena, entry n stored and later read
//                   by lane n % 4 (a lane reads its own stores).  A range that fills ends the walk as unfinished: the
//                   host runs it again from its seed with twice the range.  Every loop is bounded by a capacity.
//   R. k_cg_claim, k_cg_hits: which kept contig holds the seed of a later item of the batch; the host resolves the
//      forward-only dependency over those hits in item order; k_cg_visit marks the nodes of the kept contigs
//   T. k_cg_text    a wave per kept contig: its bases (db_nodes_print) at the offset the host has summed
// All are grid-stride loops (the "grid" knob caps the launches); the table and the link store are only read.
// A walk whose state never repeats on a cycle without a fork (a link put by hand, or by a foreign .ctp, on a node of such a
// cycle is picked up again every round, so the held list grows) is run again with doubled ranges until the call ends
// with MCX_ERR_NOMEM; the reference spins there.
// Repeat rule: the state of a later entry is compared through cg_hash, a chain of splitmix64 finalisers over both lists
// as (count, then per link: id, pos | len << 32, age); a link's id is its index in the merged store.
#pragma once
#include <deque>
#include <unordered_map>
#include "mcx_thread.h"

namespace mcx {

enum : uint32_t { kCgPopFwd = 0, kCgColFwd, kCgPopFrkColFwd, kCgNoCovg, kCgNoColCovg, kCgNoLinks, kCgSplitLinks, kCgMissingLinks, kCgUseLinks, kCgCorrupt };
enum : uint32_t { kCgStopUnknown = 0, kCgStopNoCovg, kCgStopNoColCovg, kCgStopNoPaths, kCgStopSplit, kCgStopMissing, kCgStopCycle, kCgStopLowStep, kCgStopLowCumul };
constexpr uint32_t kCgReseed = 1, kCgNoCheck = 2;  // = MCX_CONTIGS_RESEED, MCX_CONTIGS_NO_MISSING_CHECK
constexpr uint64_t kCgFirst = 1ull << 63;          // on a stored node: its first entry of this direction
constexpr uint32_t kCgNoItem = 0xffffffffu;

// an entry of a list: a held or counter link (link = its index in the store), or a segment (link = num_nodes,
// pos = in_fork, age = out_fork)
struct CgFollow { uint32_t link, pos, age, len; };
struct CgTask {
  uint64_t seed;            // slot of the seed key
  uint64_t *nodes, *hashes;  // its ranges: node_cap nodes and as many hashes,
  CgFollow *lists;           // ... 3 * list_cap list entries
  uint32_t node_cap, list_cap;
};
struct CgRes {
  uint64_t seed_key[4];
  uint64_t max_step_gap[2];
  double gap_conf[2];
  uint32_t n[2];  // nodes walked per direction (the seed is in neither)
  uint32_t num_junc, paths_held[2], paths_cntr[2], unfinished /* 1: the nodes, 2: the lists */, corrupt;
  uint32_t wlk_steps[9];
  uint8_t stop_causes[2], outdegree_rv, outdegree_fw;
};

__device__ __forceinline__ uint64_t cg_mix(uint64_t x)
{
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the lists of one walk, as the group's first lane keeps them
struct CgLists {
  CgFollow *held, *cntr, *segs;  // oldest first, all three
  uint32_t nheld, ncntr, nseg, cap, full;
};
__device__ __forceinline__ uint32_t cg_fbase(const ThLink *links, const CgFollow &f) { return th_base(links[f.link], f.pos); }

__device__ __forceinline__ void cg_lists_start(CgLists &w)
{
  w.nheld = w.ncntr = 0;
  w.nseg = 1;
  w.segs[0] = CgFollow{1u, 0u, 0u, 0u};  // _gw_gseg_init
}

// pickup_paths:173-190 for the oriented node (key, o): its links in store order
template <int W>
__device__ __forceinline__ void cg_pickup(const ThLink *links, uint64_t nlinks, const Kmer<W> &key, uint32_t o, bool counter, bool filter, uint32_t next_base,
                                          CgLists &w)
{
  uint64_t kw[4] = {0, 0, 0, 0};
  for (int j = 0; j < W; j++) kw[j] = (key.w[j] << 1) | (j + 1 < W ? key.w[j + 1] >> 63 : (uint64_t)o);
  auto cmp = [&](const ThLink &L) -> int {
    for (int j = 0; j < W; j++)
      if (L.kw[j] != kw[j]) return L.kw[j] < kw[j] ? -1 : 1;
    return 0;
  };
  uint64_t lo = 0, hi = nlinks;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (cmp(links[mid]) < 0) lo = mid + 1;
    else hi = mid;
  }
  for (uint64_t i = lo; i < nlinks && cmp(links[i]) == 0; i++) {
    const ThLink L = links[i];
    uint32_t pos = 0;
    if (filter) {  // a counter link at a fork: it has taken its first base already
      if (th_base(L, 0) != next_base || L.len < 2) continue;
      pos = 1;
    }
    uint32_t &n = counter ? w.ncntr : w.nheld;
    if (n == w.cap) { w.full = 1; return; }
    (counter ? w.cntr : w.held)[n++] = CgFollow{(uint32_t)i, pos, 0u, L.len};
  }
}

// graph_walker_choose:433-511 at a fork of which the successors S (a mask over ACGT) are in the sample
__device__ __forceinline__ uint32_t cg_choose(const ThLink *links, const CgLists &w, uint32_t S, bool check, uint32_t &base, uint64_t &gap)
{
  gap = 0;
  if (!w.nheld) return kCgNoLinks;
  uint32_t taken = 0;
  for (uint32_t i = 0; i < w.nheld; i++) taken |= 1u << cg_fbase(links, w.held[i]);
  for (uint32_t i = 0; i < w.ncntr; i++) taken |= 1u << cg_fbase(links, w.cntr[i]);
  if (taken & ~S) return kCgCorrupt;
  const uint32_t age = w.held[0].age, nuc = cg_fbase(links, w.held[0]);
  if (age == 0) return kCgNoLinks;
  uint32_t i = 1;
  while (i < w.nheld && cg_fbase(links, w.held[i]) == nuc) i++;
  if (i < w.nheld && w.held[i].age == age) return kCgSplitLinks;
  uint32_t at = i < w.nheld ? w.held[i].age : 0u;  // choice_age; the segments are kept oldest first here
  while (at < w.nseg && !w.segs[w.nseg - 1u - at].pos) at++;
  if (at >= w.nseg) return kCgCorrupt;  // (the reference would read past its list)
  for (uint32_t j = 0; j <= at; j++) gap += w.segs[w.nseg - 1u - j].link;
  if (check && (uint32_t)__popc(taken) < (uint32_t)__popc(S)) return kCgMissingLinks;
  base = nuc;
  return kCgUseLinks;
}

// _graph_walker_force_jump:554-602: the lists behind a fork taken over base b
__device__ __forceinline__ void cg_fork(const ThLink *links, CgLists &w, uint32_t b)
{
  uint32_t j = 0;
  for (uint32_t i = 0; i < w.nheld; i++) {
    CgFollow f = w.held[i];
    if (cg_fbase(links, f) != b) continue;
    f.pos++;
    if (f.pos < f.len) w.held[j++] = f;
  }
  w.nheld = j;
  j = 0;
  for (uint32_t i = 0; i < w.ncntr; i++) {
    CgFollow f = w.cntr[i];
    if (cg_fbase(links, f) != b || f.pos + 1u >= f.len) continue;
    f.pos++;
    w.cntr[j++] = f;
  }
  w.ncntr = j;
}

// _gw_gseg_update:104-147 for a step of one node
__device__ __forceinline__ void cg_seg_update(CgLists &w, bool fw_fork, bool rv_fork)
{
  if (fw_fork) w.segs[w.nseg - 1u].age = 1u;
  if (fw_fork || rv_fork) {
    if (w.nseg == w.cap) { w.full = 1; return; }
    w.segs[w.nseg++] = CgFollow{0u, rv_fork ? 1u : 0u, 0u, 0u};
    for (uint32_t i = 0; i < w.nheld; i++) w.held[i].age++;
    for (uint32_t i = 0; i < w.ncntr; i++) w.cntr[i].age++;
    uint32_t keep = 1;
    if (w.nheld) keep = max(keep, w.held[0].age + 1u);
    if (w.ncntr) keep = max(keep, w.cntr[0].age + 1u);
    if (keep < w.nseg) {  // the oldest segments hold no link any more
      const uint32_t drop = w.nseg - keep;
      for (uint32_t i = 0; i < keep; i++) w.segs[i] = w.segs[i + drop];
      w.nseg = keep;
    }
  }
  w.segs[w.nseg - 1u].link++;
}

__device__ __forceinline__ uint64_t cg_hash(const CgLists &w)
{
  uint64_t h = cg_mix((uint64_t)w.nheld);
  for (uint32_t i = 0; i < w.nheld; i++) {
    const CgFollow f = w.held[i];
    h = cg_mix(h ^ f.link);
    h = cg_mix(h ^ ((uint64_t)f.pos | (uint64_t)f.len << 32));
    h = cg_mix(h ^ f.age);
  }
  h = cg_mix(h ^ (uint64_t)w.ncntr);
  for (uint32_t i = 0; i < w.ncntr; i++) {
    const CgFollow f = w.cntr[i];
    h = cg_mix(h ^ f.link);
    h = cg_mix(h ^ ((uint64_t)f.pos | (uint64_t)f.len << 32));
    h = cg_mix(h ^ f.age);
  }
  return h;
}

// union edges of a slot by the four lanes of a group (every lane of the wave makes the call)
__device__ __forceinline__ uint32_t cg_union_edges(const TableView &t, uint64_t slot, uint32_t ncols, uint32_t sub, bool on)
{
  uint32_t e = 0;
  if (on)
    for (uint32_t c = sub; c < ncols; c += 4) e |= (uint32_t)*val_ptr(t, slot, c) & 0xffu;
  e |= __shfl_xor(e, 1);
  e |= __shfl_xor(e, 2);
  return e;
}
// this lane's successor candidate of (key, o): its slot (kNoSlot: no edge, or the edge names an absent k-mer), in the sample?
template <int W>
__device__ __forceinline__ uint64_t cg_probe(const TableView &t, int k, uint32_t colour, const Kmer<W> &key, uint32_t o, uint32_t e, uint32_t sub, bool on, bool &ins)
{
  uint64_t nslot = kNoSlot;
  ins = false;
  if (on && ((e >> (4u * o + sub)) & 1u)) {
    uint32_t p, novel = 0, full = 0;
    const Kmer<W> nk = cr_neighbour<W>(key, o, sub, k, p);
    nslot = find_or_insert_rec<W>(t, nk, true, novel, full);  // must_exist: read-only
    if (nslot != kNoSlot) ins = *val_ptr(t, nslot, colour) != 0;
  }
  return nslot;
}

struct CgArgs {
  int k;
  uint32_t ncols, colour, flags;
  const ThLink *links;
  uint64_t nlinks;
  const double *conf;
  uint64_t nconf;
  double min_step, min_cumul;
  const CgTask *tasks;
  const uint32_t *todo;  // the items to walk
  uint64_t ntodo;
  CgRes *res;
};

// W. Four lanes per seed.  One round of the loop is one graph_walker_next, or, behind a stop that the walk itself
// raised (a loop, a low confidence), the probe that counts the last node's successors in the sample.
template <int W> __global__ __launch_bounds__(256) void k_cg_walk(TableView t, CgArgs a)
{
  const uint32_t lane = threadIdx.x & 63u, sub = lane & 3u, g0 = lane & ~3u;
  const uint64_t per_block = blockDim.x >> 2;
  const bool check = !(a.flags & kCgNoCheck);
  const int k = a.k;
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < a.ntodo; base += (uint64_t)gridDim.x * per_block) {
    const uint64_t ti = base + (threadIdx.x >> 2);
    bool live = ti < a.ntodo;
    const uint32_t item = live ? a.todo[ti] : 0u;
    CgTask T{0, nullptr, nullptr, nullptr, 0, 0};
    if (live) T = a.tasks[item];
    const bool first_lane = live && sub == 0;
    CgRes *const R = a.res + item;
    uint64_t *const nd = T.nodes, *const hs = T.hashes;
    CgLists w;
    w.cap = T.list_cap;
    w.held = T.lists;
    w.cntr = w.held + T.list_cap;
    w.segs = w.cntr + T.list_cap;
    w.nheld = w.ncntr = w.nseg = 0;
    w.full = 0;
    Kmer<W> seed, key;
    for (int i = 0; i < W; i++) seed.w[i] = 0;
    if (live) seed = cl_key<W>(t, T.seed);
    key = seed;
    uint64_t slot = T.seed;
    uint32_t o = 0, dir = 0, n[2] = {0, 0}, fork_count = 0, pending = 0;
    bool ending = false;
    double gap_conf = 1.0;
    uint64_t max_gap = 0;
    if (live && T.node_cap == 0) live = false;  // (the host gives every walk a node at least)
    if (first_lane) {
      for (int i = 0; i < 4; i++) R->seed_key[i] = i < W ? seed.w[i] : 0ull;
      R->num_junc = R->corrupt = 0;
      R->unfinished = live ? 0u : 1u;
      for (int i = 0; i < 9; i++) R->wlk_steps[i] = 0;
      R->n[0] = R->n[1] = 0;
      if (live) {
        nd[0] = T.seed << 1;
        hs[0] = 0;
        cg_lists_start(w);
        if (*val_ptr(t, slot, a.colour) != 0) cg_pickup<W>(a.links, a.nlinks, key, o, false, false, 0u, w);
        if (w.full) R->unfinished = 2;
      }
    }
    if ((uint32_t)__shfl((int)((first_lane && live) ? w.full : 0u), (int)g0)) live = false;  // the first pick-up found no room
    while (__builtin_amdgcn_ballot_w64(live)) {  // (the same for the whole wave: the votes cross lanes)
      // the successors of the node the walker is on
      const uint32_t e = cg_union_edges(t, slot, a.ncols, sub, live);
      bool ins;
      const uint64_t nslot = cg_probe<W>(t, k, a.colour, key, o, e, sub, live, ins);
      const uint32_t F = (uint32_t)(__builtin_amdgcn_ballot_w64(nslot != kNoSlot) >> g0) & 15u;
      const uint32_t S = (uint32_t)(__builtin_amdgcn_ballot_w64(ins) >> g0) & 15u;
      uint32_t ctl = 0;  // status | choice << 8 | the direction ends << 16 | a list is full << 17
      uint64_t gap = 0;
      if (first_lane && live) {
        uint32_t status = kCgNoCovg, choice = 0, cause = pending;
        bool finish = ending;
        if (!ending) {
          if (!F) status = kCgNoCovg;
          else if (!(F & (F - 1u))) { choice = (uint32_t)__builtin_ctz(F); status = S ? kCgColFwd : kCgPopFwd; }
          else if (!S) status = kCgNoColCovg;
          else if (!(S & (S - 1u))) { choice = (uint32_t)__builtin_ctz(S); status = kCgPopFrkColFwd; }
          else status = cg_choose(a.links, w, S, check, choice, gap);
          finish = status >= kCgNoCovg && status != kCgUseLinks;
          if (finish) {
            cause = status == kCgNoCovg ? kCgStopNoCovg : status == kCgNoColCovg ? kCgStopNoColCovg : status == kCgNoLinks ? kCgStopNoPaths
                    : status == kCgSplitLinks ? kCgStopSplit : status == kCgMissingLinks ? kCgStopMissing : kCgStopUnknown;
            if (status == kCgCorrupt) R->corrupt++;
          }
        }
        if (finish) {  // what _assemble_contig keeps of a direction
          R->paths_held[dir] = w.nheld;
          R->paths_cntr[dir] = w.ncntr;
          R->stop_causes[dir] = (uint8_t)cause;
          R->max_step_gap[dir] = max_gap;
          R->gap_conf[dir] = gap_conf;
          R->num_junc += fork_count;
          R->n[dir] = n[dir];
          if (dir == 0) R->outdegree_rv = (uint8_t)__popc(S);
          else R->outdegree_fw = (uint8_t)__popc(S);
        }
        ctl = status | choice << 8 | (finish ? 1u << 16 : 0u);
      }
      ctl = (uint32_t)__shfl((int)ctl, (int)g0);
      const uint32_t status = ctl & 0xffu, choice = (ctl >> 8) & 3u;
      const bool finish = live && ((ctl >> 16) & 1u);
      const bool moving = live && !finish;
      if (finish) {
        if (dir == 0) {  // the other way: from the reverse of the seed, with a clean walker
          dir = 1;
          key = seed; slot = T.seed; o = 1;
          ending = false; pending = 0; fork_count = 0; gap_conf = 1.0; max_gap = 0;
          if (first_lane) {
            cg_lists_start(w);
            if (*val_ptr(t, slot, a.colour) != 0) cg_pickup<W>(a.links, a.nlinks, key, o, false, false, 0u, w);
          }
        } else live = false;
      }
      // the step (graph_walker_force)
      const uint64_t cslot = (uint64_t)__shfl((unsigned long long)nslot, (int)(g0 + choice));
      const bool cins = moving && ((S >> choice) & 1u);
      const bool is_fork = status == kCgPopFrkColFwd || status == kCgUseLinks;
      uint32_t lost = 0, nb = 0;
      if (moving) {
        uint32_t p;
        lost = cr_first_nuc<W>(key, o, k);
        key = cr_neighbour<W>(key, o, choice, k, p);
        o = p;
        slot = cslot;
        nb = cr_last_nuc<W>(key, o, k);
        if (first_lane && is_fork) { cg_fork(a.links, w, nb); fork_count++; }
      }
      // the other previous nodes in the sample (db_graph_prev_nodes_with_mask), where the new node is in the sample
      const uint32_t e2 = cg_union_edges(t, slot, a.ncols, sub, cins);
      bool pin;
      const uint64_t pslot = cg_probe<W>(t, k, a.colour, key, o ^ 1u, e2, sub, cins && sub != 3u - lost, pin);
      const uint32_t P = (uint32_t)(__builtin_amdgcn_ballot_w64(pin) >> g0) & 15u;
      if (check)
        for (uint32_t q = 0; q < 4; q++) {  // (every lane goes round four times: the votes cross lanes)
          const bool on = cins && ((P >> q) & 1u);
          const uint64_t qslot = (uint64_t)__shfl((unsigned long long)pslot, (int)(g0 + q));
          uint32_t qp = 0;
          Kmer<W> qk = key;
          if (on) qk = cr_neighbour<W>(key, o ^ 1u, q, k, qp);
          const uint32_t qo = qp ^ 1u;  // turned towards the new node
          const uint32_t e3 = cg_union_edges(t, qslot, a.ncols, sub, on);
          bool din;
          (void)cg_probe<W>(t, k, a.colour, qk, qo, e3, sub, on, din);
          const uint32_t D = (uint32_t)__popc((uint32_t)(__builtin_amdgcn_ballot_w64(din) >> g0) & 15u);
          if (first_lane && on) cg_pickup<W>(a.links, a.nlinks, qk, qo, true, D > 1u, nb, w);
        }
      // segments, pick-up, the node and the stops that the assembly raises
      uint32_t ctl2 = 0;  // low confidence cause | a list is full << 8
      uint64_t h = 0;
      if (first_lane && moving) {
        cg_seg_update(w, is_fork, P != 0);
        if (cins) cg_pickup<W>(a.links, a.nlinks, key, o, false, false, 0u, w);
        R->wlk_steps[status]++;
        uint32_t low = 0;
        if (status == kCgUseLinks) {
          const uint64_t gap_length = gap + (uint64_t)k + 1u;
          const double confid = gap_length < a.nconf ? a.conf[gap_length] : 0.0;
          max_gap = max(max_gap, gap_length);
          gap_conf = gap_conf * confid;
          if (confid < a.min_step) low = kCgStopLowStep;
          else if (gap_conf < a.min_cumul) low = kCgStopLowCumul;
        }
        h = cg_hash(w);
        ctl2 = low | (w.full ? 1u << 8 : 0u);
      }
      ctl2 = (uint32_t)__shfl((int)ctl2, (int)g0);
      h = (uint64_t)__shfl((unsigned long long)h, (int)g0);
      if (moving) {
        const uint32_t m = n[dir], low = ctl2 & 0xffu;
        const uint64_t ref = (slot << 1) | o;
        uint32_t cnt = 0, dup = 0;
        // entry i of this direction is at nd[1 + i] or, the second way, at nd[cap - 1 - i]; lane i % 4 has stored it
        for (uint32_t i = sub; i < m; i += 4) {
          const uint64_t at = dir == 0 ? 1ull + i : (uint64_t)T.node_cap - 1u - i;
          const uint64_t x = nd[at];
          if ((x & ~kCgFirst) != ref) continue;
          cnt++;
          if (!(x & kCgFirst) && hs[at] == h) dup = 1;
        }
        cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2);
        dup |= __shfl_xor(dup, 1); dup |= __shfl_xor(dup, 2);
        if ((ctl2 >> 8) & 1u) {  // a list ran out of room
          if (sub == 0) R->unfinished = 2;
          live = false;
        } else if (1ull + n[0] + n[1] >= (uint64_t)T.node_cap) {  // no room for the node
          if (sub == 0) R->unfinished = 1;
          live = false;
        } else {
          if (sub == (m & 3u)) {
            const uint64_t at = dir == 0 ? 1ull + m : (uint64_t)T.node_cap - 1u - m;
            nd[at] = ref | (cnt == 0 ? kCgFirst : 0ull);
            hs[at] = h;
          }
          n[dir] = m + 1u;
          if (low) { ending = true; pending = low; }
          else if (cnt && dup) { ending = true; pending = kCgStopCycle; }  // rpt_walker_attempt_traverse said no: the node stays
        }
      }
      // (the shuffles of a group's own branch stay inside the group, whose four lanes take the branch together)
      if (live && finish) {  // the pick-up at the start of the second direction may have filled the list
        uint32_t f = first_lane ? w.full : 0u;
        f = (uint32_t)__shfl((int)f, (int)g0);
        if (f) { if (sub == 0) R->unfinished = 2; live = false; }
      }
    }
  }
}

// S. flag[slot] = the slot holds a key of the sample; flag[nslots] = 0 for the scan
__global__ __launch_bounds__(256) void k_cg_flag(TableView t, uint32_t colour, uint8_t *flag)
{
  for (uint64_t s = cl_first(); s <= t.nslots; s += cl_stride())
    flag[s] = s < t.nslots && (key_ptr(t, s)[0] & kFlag) && *val_ptr(t, s, colour) != 0;
}
__global__ __launch_bounds__(256) void k_cg_slots(const uint8_t *flag, const uint64_t *ex, uint64_t nslots, uint64_t *slots)
{
  for (uint64_t s = cl_first(); s < nslots; s += cl_stride())
    if (flag[s]) slots[ex[s]] = s;
}
// word w of the key in slots[through[i]]
template <int W> __global__ __launch_bounds__(256) void k_cg_keyword(TableView t, const uint64_t *slots, const uint64_t *through, uint32_t w, uint64_t *dst, uint64_t n)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) dst[i] = cl_key<W>(t, slots[through[i]]).w[w];
}
__global__ __launch_bounds__(256) void k_cg_gather(const uint64_t *slots, const uint64_t *perm, uint64_t n, uint64_t *out)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) out[i] = slots[perm[i]];
}
// the seed reads: k bases each at bases + i * k; out[i] = the slot of the canonical key, kNoSlot: no key, kNoSlot - 1: not in the sample
template <int W> __global__ __launch_bounds__(256) void k_cg_seeds(TableView t, int k, uint32_t colour, const uint8_t *bases, uint64_t n, uint64_t *out)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    Kmer<W> x;
    for (int j = 0; j < W; j++) x.w[j] = 0;
    for (int j = 0; j < k; j++) kmer_push<W>(x, base_code(bases[i * (uint64_t)k + j]), k);
    const Kmer<W> rc = revcomp<W>(x, k);
    uint32_t novel = 0, full = 0;
    const uint64_t s = find_or_insert_rec<W>(t, kmer_less<W>(x, rc) ? x : rc, true, novel, full);
    out[i] = s == kNoSlot ? kNoSlot : *val_ptr(t, s, colour) != 0 ? s : kNoSlot - 1;
  }
}

// R. seeditem[slot of item i's seed] = the smallest such i (CLEAR: back to none)
template <bool CLEAR> __global__ __launch_bounds__(256) void k_cg_claim(const CgTask *tasks, uint64_t n, uint32_t *seeditem)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    if (CLEAR) seeditem[tasks[i].seed] = kCgNoItem;
    else atomicMin(&seeditem[tasks[i].seed], (uint32_t)i);
  }
}
// f(contig index, node reference) for the nodes of item j by a wave
template <class F> __device__ __forceinline__ void cg_for_nodes(const CgTask &T, const CgRes &R, uint32_t lane, F &&f)
{
  const uint64_t total = 1ull + R.n[0] + R.n[1];
  for (uint64_t i = lane; i < total; i += 64) {
    const uint64_t x = i <= R.n[0] ? T.nodes[R.n[0] - i] ^ 1ull : T.nodes[T.node_cap - 1u - (i - R.n[0] - 1u)];
    f(i, x & ~kCgFirst);
  }
}
// a wave per item j: a pair (j, i) for every node of its contig that is the seed of a later item i
__global__ __launch_bounds__(256) void k_cg_hits(const CgTask *tasks, const CgRes *res, uint64_t n, const uint32_t *seeditem, uint64_t *hits, uint64_t cap,
                                                 unsigned long long *nhits)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t j = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < n; j += nwaves)
    cg_for_nodes(tasks[j], res[j], lane, [&](uint64_t, uint64_t ref) {
      const uint32_t i = seeditem[ref >> 1];
      if (i == kCgNoItem || (uint64_t)i <= j) return;
      const uint64_t at = atomicAdd(nhits, 1ull);
      if (at < cap) hits[at] = j << 32 | i;
    });
}
// a wave per kept item: its nodes are visited
__global__ __launch_bounds__(256) void k_cg_visit(const CgTask *tasks, const CgRes *res, const uint32_t *kept, uint64_t nkept, uint8_t *visited)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t c = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < nkept; c += nwaves)
    cg_for_nodes(tasks[kept[c]], res[kept[c]], lane, [&](uint64_t, uint64_t ref) { visited[ref >> 1] = 1; });
}
__global__ __launch_bounds__(256) void k_cg_unvisited(const uint64_t *cand, uint64_t n, const uint8_t *visited, uint8_t *out)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) out[i] = !visited[cand[i]];
}

// T. A wave per kept contig: `<bases>\n` at out + off[c] (db_nodes_print: the first node's k bases, then the last base
// of every other node)
template <int W>
__global__ __launch_bounds__(256) void k_cg_text(TableView t, int k, const CgTask *tasks, const CgRes *res, const uint32_t *kept, uint64_t nkept,
                                                 const uint64_t *off, uint8_t *out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  for (uint64_t c = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < nkept; c += nwaves) {
    const CgTask T = tasks[kept[c]];
    const CgRes R = res[kept[c]];
    uint8_t *dst = out + off[c];
    const uint64_t total = 1ull + R.n[0] + R.n[1];
    cg_for_nodes(T, R, lane, [&](uint64_t i, uint64_t ref) {
      const Kmer<W> key = cl_key<W>(t, ref >> 1);
      const uint32_t o = (uint32_t)(ref & 1u);
      if (i == 0)
        for (int j = 0; j < k; j++) dst[j] = (uint8_t)"ACGT"[o ? 3u - th_kmer_base<W>(key, k, k - 1 - j) : th_kmer_base<W>(key, k, j)];
      else dst[(uint64_t)k - 1u + i] = (uint8_t)"ACGT"[cr_last_nuc<W>(key, o, k)];
    });
    if (lane == 0) dst[(uint64_t)k - 1u + total] = '\n';
  }
}

// ---- L. the links of a .ctp --------------------------------------------------------------------------------------------
// a thread per k-mer line: kw[4 * ordinal ..] = (canonical key << 1) as ThLink keeps it, flip[ordinal] = the line holds
// the key's reverse complement; a k-mer that is no key of the table is counted
template <int W>
__global__ __launch_bounds__(256) void k_cg_kmers(TableView t, int k, const uint8_t *text, const uint64_t *lstart, const uint64_t *kline, uint64_t nk, uint64_t *kw,
                                                  uint8_t *flip, unsigned long long *err, unsigned long long *nmissing)
{
  unsigned long long miss = 0;
  for (uint64_t i = cl_first(); i < nk; i += cl_stride()) {
    const uint64_t p = lstart[kline[i]], e = lstart[kline[i] + 1] - 1;
    bool ok = e - p >= (uint64_t)k + 2 && text[p + k] == ' ';
    for (uint64_t j = 0; ok && j < (uint64_t)k; j++) ok = lk_acgt(text[p + j]);
    for (uint64_t j = p + k + 1; ok && j < e; j++) ok = lk_digit(text[j]);
    if (!ok) { lk_fail(err, p, MCX_LINKS_BAD_KMER_LINE); continue; }
    Kmer<W> x;
    for (int j = 0; j < W; j++) x.w[j] = 0;
    for (int j = 0; j < k; j++) kmer_push<W>(x, base_code(text[p + j]), k);
    const Kmer<W> rc = revcomp<W>(x, k);
    const bool fw = kmer_less<W>(x, rc) || !kmer_less<W>(rc, x);
    const Kmer<W> key = fw ? x : rc;
    uint32_t novel = 0, full = 0;
    if (find_or_insert_rec<W>(t, key, true, novel, full) == kNoSlot) miss++;  // must_exist: read-only
    for (int j = 0; j < 4; j++) kw[4 * i + j] = j < W ? (key.w[j] << 1) | (j + 1 < W ? key.w[j + 1] >> 63 : 0ull) : 0ull;
    flip[i] = fw ? 0 : 1;
  }
  block_add(nmissing, miss);
}
// a thread per line: `<F|R> <njuncs> <nseen> <juncs>` of a link line, whatever follows behind a blank ignored.  Link i of
// the piece gets links[i] and nw[i] (junction words); nw[nl] = 0 for the scan.
__global__ __launch_bounds__(256) void k_cg_parse(const uint8_t *text, const uint64_t *lstart, uint64_t nlines, const uint8_t *lflag, const uint64_t *kx,
                                                  const uint64_t *lx, LkLink *links, uint64_t *nw, unsigned long long *err, unsigned long long *maxlen)
{
  unsigned long long c_max = 0;
  for (uint64_t l = cl_first(); l <= nlines; l += cl_stride()) {
    if (l == nlines) { nw[lx[l]] = 0; continue; }
    if (!lflag[l]) continue;
    const uint64_t p = lstart[l], e = lstart[l + 1] - 1;
    LkLink L;
    L.line = p; L.cnt = 0; L.woff = L.poff = 0; L.key = 0; L.len = 0; L.junc_at = L.seq_at = L.seq_len = L.jp_at = L.jp_len = 0;
    uint32_t code = 0;
    if (kx[l] == 0) code = MCX_LINKS_LINK_BEFORE_KMER;
    else if (e - p < 2 || (text[p] != 'F' && text[p] != 'R') || text[p + 1] != ' ') code = MCX_LINKS_BAD_ORIENT;
    else {
      uint64_t q = p + 2, nj = 0, cnt = 0;
      uint32_t nd = 0;
      for (; q < e && lk_digit(text[q]); q++, nd++) nj = min(nj * 10 + (uint64_t)(text[q] - '0'), 1ull << 40);
      if (!nd || q >= e || text[q] != ' ') code = MCX_LINKS_BAD_NUMBER;
      else {
        q++;
        nd = 0;
        for (; q < e && lk_digit(text[q]); q++, nd++) cnt = min(cnt * 10 + (uint64_t)(text[q] - '0'), 1ull << 40);
        if (q < e && text[q] == ',' && nd) code = MCX_LINKS_MULTI_COLOUR;
        else if (!nd || q >= e || text[q] != ' ') code = MCX_LINKS_BAD_NUMBER;
        else {
          q++;
          const uint64_t j0 = q;
          for (; q < e && text[q] != ' '; q++)
            if (!lk_acgt(text[q])) { code = MCX_LINKS_BAD_JUNCTION; break; }
          if (!code) {
            if (nj == 0 || nj > kThMaxJuncs) code = MCX_LINKS_NJUNCS_RANGE;
            else if (nj != q - j0) code = MCX_LINKS_NJUNCS_LENGTH;
            else { L.cnt = cnt; L.len = (uint32_t)nj; L.junc_at = (uint32_t)(j0 - p); L.key = ((kx[l] - 1) << 1) | (text[p] == 'R' ? 1ull : 0ull); }
          }
        }
      }
    }
    if (code) { lk_fail(err, p, code); L.len = 0; }
    links[lx[l]] = L;
    nw[lx[l]] = (L.len + 31u) / 32u;
    c_max = max(c_max, (unsigned long long)L.len);
  }
  if (c_max) atomicMax(maxlen, c_max);
}
// the parsed links as the store keeps them, viewing wpool
__global__ __launch_bounds__(256) void k_cg_links(const LkLink *in, uint64_t nl, const uint64_t *kw, const uint8_t *flip, const uint64_t *wpool, uint32_t W, ThLink *out)
{
  for (uint64_t i = cl_first(); i < nl; i += cl_stride()) {
    const LkLink L = in[i];
    const uint64_t ord = L.key >> 1;
    ThLink T;
    for (int j = 0; j < 4; j++) T.kw[j] = kw[4 * ord + j];
    T.kw[W - 1] |= (L.key & 1ull) ^ (uint64_t)flip[ord];
    T.base = wpool;
    T.start = L.woff * 32u;
    T.len = L.len;
    T.cnt = (uint32_t)min(L.cnt, (uint64_t)kThMaxSeen);
    out[i] = T;
  }
}

}  // namespace mcx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
extern "C" int mcx_graph_links_load_text(mcx_graph *g, const void *text, uint64_t nbytes, uint64_t *nlinks, uint64_t *nmissing)
{
  if (nlinks) *nlinks = 0;
  if (nmissing) *nmissing = 0;
  int rc = lookup_begin(g, "thread");
  if (rc != MCX_OK) return rc;
  if (!nbytes) return MCX_OK;
  if (!text) return fail(MCX_ERR_ARG, "null text");
  if (nbytes >= (1ull << 31)) return fail(MCX_ERR_ARG, "links: a piece of %llu bytes (2 GB at the most)", (unsigned long long)nbytes);
  if (((const uint8_t *)text)[nbytes - 1] != '\n') return fail(MCX_ERR_ARG, "links: the text does not end with a newline");
  if (!g->links) {
    g->links = new ThreadStore();
    g->links->seg.push_back(ThSegment());
  }
  hipStream_t st = g->stream;
  const uint64_t n = nbytes;
  DevBuf<uint8_t> d_text, d_flag, d_kflag, d_lflag, d_flip;
  DevBuf<uint64_t> d_lidx, d_lstart, d_kx, d_lx, d_kline, d_kw, d_nw, d_woff, d_poff, d_wpool;
  DevBuf<unsigned long long> d_ctr;  // the first refusal, the k-mers missing, the longest link
  DevBuf<LkLink> d_links;
  DevBuf<uint32_t> d_ppool;
  DevBuf<ThLink> d_th;
  auto run = [&]() -> int {
    int rc2;
    HIP_TRY(d_text.alloc(n + 16));
    HIP_TRY(d_flag.alloc(n + 1));
    HIP_TRY(d_lidx.alloc(n + 1));
    HIP_TRY(d_ctr.alloc(3));
    HIP_TRY(hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_text.p + n, 0, 16, st));
    HIP_TRY(hipMemsetAsync(d_ctr.p, 0xff, 8, st));
    HIP_TRY(hipMemsetAsync(d_ctr.p + 1, 0, 16, st));
    GRID_LAUNCH(k_lk_mark, n + 1, (const uint8_t *)d_text.p, n, d_flag.p);
    uint64_t nlines = 0, nk = 0, nl = 0;
    if ((rc2 = scan_total(st, (const uint8_t *)d_flag.p, d_lidx.p, n + 1, &nlines)) != MCX_OK) return rc2;
    HIP_TRY(d_lstart.alloc(nlines + 1));
    HIP_TRY(d_kflag.alloc(nlines + 1));
    HIP_TRY(d_lflag.alloc(nlines + 1));
    HIP_TRY(d_kx.alloc(nlines + 1));
    HIP_TRY(d_lx.alloc(nlines + 1));
    GRID_LAUNCH(k_lk_starts, n + 1, (const uint8_t *)d_flag.p, (const uint64_t *)d_lidx.p, n, d_lstart.p);
    GRID_LAUNCH(k_lk_class, nlines + 1, (const uint8_t *)d_text.p, (const uint64_t *)d_lstart.p, nlines, d_kflag.p, d_lflag.p);
    if ((rc2 = scan_total(st, (const uint8_t *)d_kflag.p, d_kx.p, nlines + 1, &nk)) != MCX_OK) return rc2;
    if ((rc2 = scan_total(st, (const uint8_t *)d_lflag.p, d_lx.p, nlines + 1, &nl)) != MCX_OK) return rc2;
    HIP_TRY(d_kline.alloc(nk + 1));
    HIP_TRY(d_kw.alloc(4 * nk + 4));
    HIP_TRY(d_flip.alloc(nk + 1));
    HIP_TRY(d_links.alloc(nl + 1));
    HIP_TRY(d_nw.alloc(nl + 1));
    HIP_TRY(d_woff.alloc(nl + 1));
    HIP_TRY(d_poff.alloc(nl + 1));
    HIP_TRY(hipMemsetAsync(d_poff.p, 0, (nl + 1) * 8, st));
    GRID_LAUNCH(k_lk_klines, nlines, (const uint8_t *)d_kflag.p, (const uint64_t *)d_kx.p, nlines, d_kline.p);
    if (nk)
      GRID_LAUNCH_W(k_cg_kmers, nk, g->t, g->k, (const uint8_t *)d_text.p, (const uint64_t *)d_lstart.p, (const uint64_t *)d_kline.p, nk, d_kw.p, d_flip.p, d_ctr.p,
                    d_ctr.p + 1);
    GRID_LAUNCH(k_cg_parse, nlines + 1, (const uint8_t *)d_text.p, (const uint64_t *)d_lstart.p, nlines, (const uint8_t *)d_lflag.p, (const uint64_t *)d_kx.p,
                (const uint64_t *)d_lx.p, d_links.p, d_nw.p, d_ctr.p, d_ctr.p + 2);
    unsigned long long h[3];
    HIP_TRY(hipMemcpyAsync(h, d_ctr.p, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h[0] != kLkNoErr)
      return fail(MCX_ERR_INVAL, "links: bad line at byte %llu of the piece (refusal %d)", (unsigned long long)(h[0] >> 8), (int)(h[0] & 0xffu));
    if (nmissing) *nmissing = h[1];
    if (h[1]) return fail(MCX_ERR_INVAL, "links: %llu k-mers of the piece are not in the graph", h[1]);
    if (!nl) return MCX_OK;
    uint64_t nwords = 0;
    if ((rc2 = scan_total(st, (const uint64_t *)d_nw.p, d_woff.p, nl + 1, &nwords)) != MCX_OK) return rc2;
    HIP_TRY(d_wpool.alloc(nwords + 2));
    HIP_TRY(d_ppool.alloc(1));
    HIP_TRY(d_th.alloc(nl));
    HIP_TRY(hipMemsetAsync(d_wpool.p + nwords, 0, 16, st));
    GRID_LAUNCH(k_lk_store, nl, (const uint8_t *)d_text.p, d_links.p, (const uint64_t *)d_woff.p, (const uint64_t *)d_poff.p, nl, d_wpool.p, d_ppool.p);
    GRID_LAUNCH(k_cg_links, nl, (const LkLink *)d_links.p, nl, (const uint64_t *)d_kw.p, (const uint8_t *)d_flip.p, (const uint64_t *)d_wpool.p, (uint32_t)g->W, d_th.p);
    ThSegment seg;
    if ((rc2 = th_sort_reduce(g, d_th.p, nl, nl, (uint32_t)h[2], &seg)) != MCX_OK) return rc2;
    g->links->seg.push_back(seg);
    if (nlinks) *nlinks = nl;
    return th_merge(g, false);
  };
  rc = run();
  (void)hipStreamSynchronize(st);  // before the scratch goes
  return rc;
}

// the candidate seeds in order: slots of keys in the sample
static int contigs_candidates(mcx_graph *g, uint32_t colour, const uint8_t *seed_bases, const uint64_t *seed_offsets, uint64_t nseeds, bool from_reads,
                              std::vector<uint64_t> &cand, uint64_t *not_found)
{
  hipStream_t st = g->stream;
  int rc;
  if (from_reads) {
    const uint64_t k = (uint64_t)g->k;
    std::vector<uint8_t> flat(std::max<uint64_t>(nseeds * k, 1));
    for (uint64_t i = 0; i < nseeds; i++) {
      if (seed_offsets[i + 1] - seed_offsets[i] != k) return fail(MCX_ERR_INVAL, "contigs: seed %llu is not %d bases long", (unsigned long long)i, g->k);
      for (uint64_t j = 0; j < k; j++) {
        const uint8_t c = seed_bases[seed_offsets[i] + j];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return fail(MCX_ERR_INVAL, "contigs: seed %llu holds a base that is not one of ACGT", (unsigned long long)i);
        flat[i * k + j] = c;
      }
    }
    if (!nseeds) return MCX_OK;
    DevBuf<uint8_t> d_b;
    DevBuf<uint64_t> d_s;
    HIP_TRY(d_b.alloc(flat.size()));
    HIP_TRY(d_s.alloc(nseeds));
    std::vector<uint64_t> s(nseeds);
    auto run = [&]() -> int {
      HIP_TRY(hipMemcpyAsync(d_b.p, flat.data(), flat.size(), hipMemcpyHostToDevice, st));
      GRID_LAUNCH_W(k_cg_seeds, nseeds, g->t, g->k, colour, (const uint8_t *)d_b.p, nseeds, d_s.p);
      HIP_TRY(hipMemcpyAsync(s.data(), d_s.p, nseeds * 8, hipMemcpyDeviceToHost, st));
      return MCX_OK;
    };
    rc = run();
    (void)hipStreamSynchronize(st);
    if (rc != MCX_OK) return rc;
    for (uint64_t i = 0; i < nseeds; i++) {
      if (s[i] == kNoSlot) ++*not_found;
      else if (s[i] != kNoSlot - 1) cand.push_back(s[i]);
    }
    return MCX_OK;
  }
  const uint64_t ns = g->t.nslots;
  DevBuf<uint8_t> flag, tmp;
  DevBuf<uint64_t> ex, slots, k0, k1, p0, p1, sorted;
  auto run = [&]() -> int {
    HIP_TRY(flag.alloc(ns + 1));
    HIP_TRY(ex.alloc(ns + 1));
    GRID_LAUNCH(k_cg_flag, ns + 1, g->t, colour, flag.p);
    uint64_t m = 0;
    int rc2 = scan_total(st, (const uint8_t *)flag.p, ex.p, ns + 1, &m);
    if (rc2 != MCX_OK) return rc2;
    if (!m) return MCX_OK;
    HIP_TRY(slots.alloc(m));
    GRID_LAUNCH(k_cg_slots, ns, (const uint8_t *)flag.p, (const uint64_t *)ex.p, ns, slots.p);
    HIP_TRY(k0.alloc(m));
    HIP_TRY(k1.alloc(m));
    HIP_TRY(p0.alloc(m));
    HIP_TRY(p1.alloc(m));
    HIP_TRY(sorted.alloc(m));
    hipLaunchKernelGGL(k_iota, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, p0.p, m);
    HIP_TRY(hipGetLastError());
    size_t tmp_bytes = 0;
    if ((rc2 = sort_perm_scratch(st, m, &tmp_bytes)) != MCX_OK) return rc2;
    HIP_TRY(tmp.alloc(tmp_bytes ? tmp_bytes : 16));
    auto word = [&](int w, bool, const uint64_t *through, uint64_t *dst, const uint64_t **) -> int {
      GRID_LAUNCH_W(k_cg_keyword, m, g->t, (const uint64_t *)slots.p, through, (uint32_t)w, dst, m);
      return MCX_OK;
    };
    uint64_t *const keys[2] = {k0.p, k1.p}, *const perms[2] = {p0.p, p1.p}, *perm = nullptr;
    if ((rc2 = sort_perm_by_words(st, m, g->W, 64, keys, perms, tmp.p, tmp_bytes, g, word, &perm)) != MCX_OK) return rc2;
    GRID_LAUNCH(k_cg_gather, m, (const uint64_t *)slots.p, (const uint64_t *)perm, m, sorted.p);
    cand.resize(m);
    HIP_TRY(hipMemcpyAsync(cand.data(), sorted.p, m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MCX_OK;
  };
  rc = run();
  (void)hipStreamSynchronize(st);
  return rc;
}

extern "C" int mcx_graph_contigs(mcx_graph *g, const uint8_t *seed_bases, const uint64_t *seed_offsets, uint64_t nseeds, const mcx_contigs_params *p,
                                 mcx_sink_fn rec_sink, void *rec_ctx, mcx_sink_fn seq_sink, void *seq_ctx, mcx_contigs_stats *stats)
{
  int rc = lookup_begin(g, "contigs");
  if (rc != MCX_OK) return rc;
  if (!p) return fail(MCX_ERR_ARG, "contigs: null parameters");
  if (p->colour >= (uint32_t)g->ncols) return fail(MCX_ERR_ARG, "contigs: colour %u is not one of the graph's %d", p->colour, g->ncols);
  if (p->flags & ~(uint32_t)(MCX_CONTIGS_RESEED | MCX_CONTIGS_NO_MISSING_CHECK)) return fail(MCX_ERR_ARG, "contigs: unknown flags 0x%x", p->flags);
  if (p->nconf && !p->conf) return fail(MCX_ERR_ARG, "contigs: null confidence table");
  if (std::isnan(p->min_step_confid) || std::isnan(p->min_cumul_confid)) return fail(MCX_ERR_ARG, "contigs: the confidence bounds must be numbers");
  const bool from_reads = seed_offsets != nullptr;
  if (nseeds && !from_reads) return fail(MCX_ERR_ARG, "contigs: seed reads without offsets");
  if (from_reads && !seed_bases && nseeds && seed_offsets[nseeds] != seed_offsets[0]) return fail(MCX_ERR_ARG, "null read buffers");
  if ((rc = th_merge(g, true)) != MCX_OK) return rc;
  static const ThSegment none;
  const ThSegment *seg = g->links ? &g->links->seg[0] : &none;
  if (seg->n >= 0xffffffffull) return fail(MCX_ERR_ARG, "contigs: the store holds %llu links (2^32 - 2 at the most)", (unsigned long long)seg->n);
  if ((rc = ensure_stage(g)) != MCX_OK) return rc;
  hipStream_t st = g->stream;
  const bool reseed = p->flags & MCX_CONTIGS_RESEED;
  mcx_contigs_stats S;
  memset(&S, 0, sizeof(S));
  std::vector<uint64_t> cand;
  if ((rc = contigs_candidates(g, p->colour, seed_bases, seed_offsets, nseeds, from_reads, cand, &S.seeds_not_found)) != MCX_OK) return rc;

  const uint64_t B = std::max<uint64_t>(1, std::min<uint64_t>(g->contigs_batch ? g->contigs_batch : 4096, 1u << 20));
  const uint64_t ns = g->t.nslots;
  DevBuf<double> d_conf;
  DevBuf<uint8_t> d_visited, d_unv;
  DevBuf<uint32_t> d_seeditem;
  DevBuf<uint64_t> d_cand;
  uint64_t ncontigs = 0, seq_off = 0;
  bool done = false;
  auto setup = [&]() -> int {
    HIP_TRY(d_conf.alloc(std::max<uint64_t>(p->nconf, 1)));
    if (p->nconf) HIP_TRY(hipMemcpyAsync(d_conf.p, p->conf, p->nconf * 8, hipMemcpyHostToDevice, st));
    if (!reseed) {
      HIP_TRY(d_visited.alloc(std::max<uint64_t>(ns, 1)));
      HIP_TRY(d_seeditem.alloc(std::max<uint64_t>(ns, 1)));
      HIP_TRY(d_unv.alloc(B));
      HIP_TRY(d_cand.alloc(B));
      HIP_TRY(hipMemsetAsync(d_visited.p, 0, std::max<uint64_t>(ns, 1), st));
      HIP_TRY(hipMemsetAsync(d_seeditem.p, 0xff, std::max<uint64_t>(ns, 1) * 4, st));
    }
    return MCX_OK;
  };
  // one batch: the candidates [c0, c0 + nb)
  auto batch = [&](uint64_t c0, uint64_t nb) -> int {
    int rc2;
    std::vector<uint8_t> unv(nb, 1);
    if (!reseed) {
      HIP_TRY(hipMemcpyAsync(d_cand.p, cand.data() + c0, nb * 8, hipMemcpyHostToDevice, st));
      GRID_LAUNCH(k_cg_unvisited, nb, (const uint64_t *)d_cand.p, nb, (const uint8_t *)d_visited.p, d_unv.p);
      HIP_TRY(hipMemcpyAsync(unv.data(), d_unv.p, nb, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    // the items: the window's candidates that no earlier batch has visited
    std::vector<CgTask> tasks;
    std::vector<uint32_t> item_of(nb, kCgNoItem);
    for (uint64_t i = 0; i < nb; i++)
      if (unv[i]) { item_of[i] = (uint32_t)tasks.size(); tasks.push_back(CgTask{cand[c0 + i], nullptr, nullptr, nullptr, 0, 0}); }
    const uint64_t ni = tasks.size();
    std::vector<CgRes> res(ni);
    DevBuf<CgTask> d_tasks;
    DevBuf<CgRes> d_res;
    DevBuf<uint32_t> d_todo;
    std::deque<DevBuf<uint64_t>> arenas;  // per launch: the nodes and the hashes of its walks
    std::deque<DevBuf<CgFollow>> listbufs;
    if (ni) {
      HIP_TRY(d_tasks.alloc(ni));
      HIP_TRY(d_res.alloc(ni));
      HIP_TRY(d_todo.alloc(ni));
      std::vector<uint32_t> todo(ni);
      const uint32_t node_cap = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(g->contigs_nodes ? g->contigs_nodes : 1024, 1u << 30));
      const uint32_t list_cap = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(g->contigs_held ? g->contigs_held : 64, 1u << 30));
      for (uint64_t i = 0; i < ni; i++) { todo[i] = (uint32_t)i; tasks[i].node_cap = node_cap; tasks[i].list_cap = list_cap; }
      while (!todo.empty()) {
        // every walk of this launch gets ranges of its own in a new arena
        uint64_t nn = 0, nl = 0;
        for (uint32_t i : todo) { nn += tasks[i].node_cap; nl += 3ull * tasks[i].list_cap; }
        arenas.emplace_back();
        arenas.emplace_back();
        listbufs.emplace_back();
        DevBuf<uint64_t> &an = arenas[arenas.size() - 2], &ah = arenas[arenas.size() - 1];
        if (an.alloc(nn) != hipSuccess || ah.alloc(nn) != hipSuccess || listbufs.back().alloc(nl) != hipSuccess) {
          (void)hipGetLastError();
          return fail(MCX_ERR_NOMEM, "contigs: no room for the ranges of %llu walks (%llu nodes, %llu list entries)", (unsigned long long)todo.size(),
                      (unsigned long long)nn, (unsigned long long)nl);
        }
        nn = nl = 0;
        for (uint32_t i : todo) {
          tasks[i].nodes = an.p + nn; tasks[i].hashes = ah.p + nn; tasks[i].lists = listbufs.back().p + nl;
          nn += tasks[i].node_cap; nl += 3ull * tasks[i].list_cap;
        }
        HIP_TRY(hipMemcpyAsync(d_tasks.p, tasks.data(), ni * sizeof(CgTask), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_todo.p, todo.data(), todo.size() * 4, hipMemcpyHostToDevice, st));
        CgArgs a;
        a.k = g->k; a.ncols = (uint32_t)g->ncols; a.colour = p->colour; a.flags = p->flags;
        a.links = seg->links; a.nlinks = seg->n; a.conf = d_conf.p; a.nconf = p->nconf;
        a.min_step = p->min_step_confid; a.min_cumul = p->min_cumul_confid;
        a.tasks = d_tasks.p; a.todo = d_todo.p; a.ntodo = todo.size(); a.res = d_res.p;
        GRID_LAUNCH_W(k_cg_walk, todo.size() * 4, g->t, a);
        HIP_TRY(hipMemcpyAsync(res.data(), d_res.p, ni * sizeof(CgRes), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<uint32_t> again;
        for (uint32_t i : todo) {
          if (!res[i].unfinished) continue;
          uint32_t &cap = res[i].unfinished == 1 ? tasks[i].node_cap : tasks[i].list_cap;
          if (cap >= (1u << 30)) return fail(MCX_ERR_NOMEM, "contigs: a walk needs a range of more than 2^30 entries");
          cap *= 2;
          again.push_back(i);
        }
        S.reruns += again.size();
        todo.swap(again);
      }
    }
    // which items give a contig: item i is dropped iff a kept item j < i holds its seed among its nodes
    std::vector<uint8_t> dropped(ni, 0);
    std::vector<std::vector<uint32_t>> hit_by(ni);
    if (!reseed && ni) {
      std::unordered_map<uint64_t, uint32_t> first_item;
      for (uint64_t i = 0; i < ni; i++)
        if (!first_item.emplace(tasks[i].seed, (uint32_t)i).second) dropped[i] = 1;  // a seed twice: the later one always goes
      uint64_t total_nodes = 0;
      for (uint64_t i = 0; i < ni; i++) total_nodes += 1ull + res[i].n[0] + res[i].n[1];
      DevBuf<uint64_t> d_hits;
      DevBuf<unsigned long long> d_nh;
      HIP_TRY(d_hits.alloc(std::max<uint64_t>(total_nodes, 1)));
      HIP_TRY(d_nh.alloc(1));
      HIP_TRY(hipMemsetAsync(d_nh.p, 0, 8, st));
      GRID_LAUNCH(k_cg_claim<false>, ni, (const CgTask *)d_tasks.p, ni, d_seeditem.p);
      GRID_LAUNCH(k_cg_hits, ni * 64, (const CgTask *)d_tasks.p, (const CgRes *)d_res.p, ni, (const uint32_t *)d_seeditem.p, d_hits.p, total_nodes, d_nh.p);
      GRID_LAUNCH(k_cg_claim<true>, ni, (const CgTask *)d_tasks.p, ni, d_seeditem.p);
      unsigned long long nh = 0;
      HIP_TRY(hipMemcpyAsync(&nh, d_nh.p, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      std::vector<uint64_t> hits(std::min<uint64_t>(nh, total_nodes));
      if (!hits.empty()) HIP_TRY(hipMemcpy(hits.data(), d_hits.p, hits.size() * 8, hipMemcpyDeviceToHost));
      for (uint64_t hb : hits) hit_by[(uint32_t)hb].push_back((uint32_t)(hb >> 32));
    }
    // the window in order
    std::vector<uint32_t> kept;
    std::vector<uint8_t> is_kept(ni, 0);
    for (uint64_t i = 0; i < nb; i++) {
      if (p->ncontigs && ncontigs + kept.size() >= p->ncontigs) { done = true; break; }
      const uint32_t it = item_of[i];
      if (it == kCgNoItem) { S.num_reseed_abort++; continue; }
      bool drop = dropped[it];
      for (uint32_t j : hit_by[it]) drop = drop || is_kept[j];
      if (drop) { S.num_reseed_abort++; continue; }
      is_kept[it] = 1;
      kept.push_back(it);
    }
    if (kept.empty()) return MCX_OK;
    // records, visited marks and text
    const uint64_t nkept = kept.size(), k = (uint64_t)g->k;
    std::vector<mcx_contig_rec> recs(nkept);
    std::vector<uint64_t> off(nkept + 1, 0);
    for (uint64_t c = 0; c < nkept; c++) {
      const CgRes &r = res[kept[c]];
      mcx_contig_rec &o = recs[c];
      memset(&o, 0, sizeof(o));
      for (int j = 0; j < 4; j++) o.seed_key[j] = r.seed_key[j];
      o.len_nodes = 1ull + r.n[0] + r.n[1];
      o.seq_off = seq_off + off[c];
      o.num_junc = r.num_junc;
      for (int d = 0; d < 2; d++) {
        o.paths_held[d] = r.paths_held[d]; o.paths_cntr[d] = r.paths_cntr[d]; o.max_step_gap[d] = r.max_step_gap[d]; o.gap_conf[d] = r.gap_conf[d];
        o.stop_causes[d] = r.stop_causes[d];
        S.stop_causes[r.stop_causes[d] < 9 ? r.stop_causes[d] : 0]++;
      }
      o.outdegree_rv = r.outdegree_rv; o.outdegree_fw = r.outdegree_fw;
      off[c + 1] = off[c] + o.len_nodes + k;  // len_nodes + k - 1 bases and the newline
      S.total_nodes += o.len_nodes;
      S.total_junc += r.num_junc;
      S.corrupt_links += r.corrupt;
      for (int j = 0; j < 9; j++) S.wlk_steps[j] += r.wlk_steps[j];
    }
    S.contigs += nkept;
    DevBuf<uint32_t> d_kept;
    DevBuf<uint64_t> d_off;
    DevBuf<uint8_t> d_text;
    HIP_TRY(d_kept.alloc(nkept));
    HIP_TRY(d_off.alloc(nkept + 1));
    if (seq_sink) HIP_TRY(d_text.alloc(off[nkept]));
    HIP_TRY(hipMemcpyAsync(d_kept.p, kept.data(), nkept * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), (nkept + 1) * 8, hipMemcpyHostToDevice, st));
    if (!reseed) GRID_LAUNCH(k_cg_visit, nkept * 64, (const CgTask *)d_tasks.p, (const CgRes *)d_res.p, (const uint32_t *)d_kept.p, nkept, d_visited.p);
    if (seq_sink)
      GRID_LAUNCH_W(k_cg_text, nkept * 64, g->t, g->k, (const CgTask *)d_tasks.p, (const CgRes *)d_res.p, (const uint32_t *)d_kept.p, nkept, (const uint64_t *)d_off.p,
                    d_text.p);
    HIP_TRY(hipStreamSynchronize(st));
    ncontigs += nkept;
    if (rec_sink && rec_sink(rec_ctx, recs.data(), nkept * sizeof(mcx_contig_rec)) != 0) return fail(MCX_ERR_SINK, "contigs: the sink refused the records");
    if (seq_sink && (rc2 = text_to_sink(g, d_text.p, off[nkept], seq_sink, seq_ctx, "contigs: the sink refused the sequences")) != MCX_OK) return rc2;
    seq_off += off[nkept];
    return MCX_OK;
  };
  auto run = [&]() -> int {
    int rc2 = setup();
    for (uint64_t c0 = 0; rc2 == MCX_OK && c0 < cand.size() && !done; c0 += B) {
      if (p->ncontigs && ncontigs >= p->ncontigs) break;
      rc2 = batch(c0, std::min<uint64_t>(B, cand.size() - c0));
    }
    return rc2;
  };
  rc = run();
  (void)hipStreamSynchronize(st);  // before the scratch goes
  if (rc != MCX_OK) return rc;
  if (stats) {
    uint64_t *dst = &stats->contigs;
    const uint64_t *src = &S.contigs;
    for (size_t i = 0; i < sizeof(S) / 8; i++) dst[i] += src[i];
  }
  return MCX_OK;
}
