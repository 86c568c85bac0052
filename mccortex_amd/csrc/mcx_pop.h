// mcx_pop.h -- `popbubbles` on the device (included by mcx_api.hip).
//
// pop_bubbles (src/tools/pop_bubbles.c) over the unitig decomposition that mcx_graph_unitig_stats keeps
// (mcx_clean.h): per unitig its summed coverage and its two ends, the parallel unitigs of every unitig
// (get_parallel_nodes + db_unitig_extend of mark_remove_bubbles), the order in which unitigs take their turn,
// then one keep flag per unitig for clean's prune kernels.  Steps ("popbubbles' device passes"):
//   A. k_pop_sums    per unitig: 64-bit coverage sum; the two oriented nodes that leave it (no link on that side)
//      k_pop_norm    db_unitig_normalise: the end with the lower key is the left one, a single k-mer is forward
//   B. k_pop_pairs   per unitig U: the sibling nodes of both ends (nodes0[], nodes1[]); for every left sibling,
//                    in order and with its multiplicity, the unitig V it starts; (U -> V) is a pair when V's other
//                    end is a right sibling in the same orientation.  Pairs go to a compacted list
//                    (the kernel runs twice: a counting pass sizes the list).
//      k_pop_mark    per pair: is it a "threat" -- would U, taking its turn before V, mark V visited?
//   C. k_pop_threats / k_pop_settle   rounds over the threat relation (a DAG: it leads from lower to higher E)
//      until a round decides nothing: which unitigs take their turn
//   D. k_pop_apply   every pair whose U took its turn marks its loser and counts one pop (process_bubble)
//      k_cl_prune_edges, k_cl_tombstone (mcx_clean.h) with the keep flags
// Every kernel is a grid-stride loop (the "grid" knob caps the launches).  The table is only read before D.
#pragma once
#include "mcx_clean.h"

namespace mcx {

constexpr uint32_t kPopMaxSib = 16;            // nodes[16] of mark_remove_bubbles: 4 next x 4 back (3 where the edge back exists)
constexpr uint64_t kPopIdMask = 0x7FFFFFFFull;  // a pair: U in bits 0..30, V in bits 31..61
constexpr uint64_t kPopLower = 1ull << 62;      // E(U) < E(V)
constexpr uint64_t kPopThreat = 1ull << 63;     // U's turn marks V visited
enum : uint8_t { kPopOpen = 0, kPopTurn = 1, kPopNoTurn = 2 };

// the three conditions of process_bubble on the branch that would go
__device__ __forceinline__ bool pop_pass(uint64_t mean, uint32_t len, uint32_t len_other, int32_t max_covg, int32_t max_klen,
                                         int32_t max_kdiff)
{
  const int64_t d = (int64_t)len - (int64_t)len_other;
  return (max_covg <= 0 || mean <= (uint64_t)max_covg) && (max_klen <= 0 || len <= (uint32_t)max_klen) &&
         (max_kdiff < 0 || (d < 0 ? -d : d) <= (int64_t)max_kdiff);
}

// sum[u] += coverage; ends[2u], ends[2u+1] = the oriented nodes 2 i + o of unitig u whose side o has no link, in
// the order they are met (a chain has exactly two, a closed cycle none: its entries stay kClNone)
__global__ __launch_bounds__(256) void k_pop_sums(uint64_t n, const uint32_t *uid, const uint32_t *cov, const uint8_t *lk,
                                                  unsigned long long *sum, uint32_t *ends)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const uint32_t u = uid[i];
    atomicAdd(&sum[u], (unsigned long long)cov[i]);
    for (uint32_t o = 0; o < 2; o++) {
      const uint32_t v = (uint32_t)(2 * i + o);
      if (!cl_end(lk, v)) continue;
      if (atomicCAS(&ends[2 * (uint64_t)u], kClNone, v) != kClNone) ends[2 * (uint64_t)u + 1] = v;
    }
  }
}

// ends[2u] = the node that leaves the normalised unitig to the left (the reverse of its first node),
// ends[2u+1] = its last node.  E(u) is the key of ends[2u] >> 1.
template <int W>
__global__ __launch_bounds__(256) void k_pop_norm(TableView t, uint64_t n, const uint64_t *slot_of, const uint32_t *len, uint32_t *ends)
{
  for (uint64_t u = cl_first(); u < n; u += cl_stride()) {
    if (!len[u]) continue;
    const uint32_t a = ends[2 * u], b = ends[2 * u + 1];
    if (a == kClNone) continue;  // a closed cycle
    if ((a >> 1) == (b >> 1)) {  // a single k-mer, forward: it leaves leftwards in reverse
      ends[2 * u] = a | 1u;
      ends[2 * u + 1] = a & ~1u;
    } else if (kmer_less<W>(cl_key<W>(t, slot_of[b >> 1]), cl_key<W>(t, slot_of[a >> 1]))) {
      ends[2 * u] = b;
      ends[2 * u + 1] = a;
    }
  }
}

// get_parallel_nodes: one node out of v over every edge, one node back over every other edge; the siblings
// come oriented as v is (heading into the shared neighbour).  The edge back to v is cleared if it is there
// (the reference asserts it is); a neighbour that is not in the graph is passed over.
template <int W>
__device__ uint32_t pop_parallel(const TableView &t, int k, const uint64_t *slot_of, const uint32_t *map, const uint8_t *ue,
                                 uint32_t v, uint32_t *out)
{
  const uint32_t i = v >> 1, o = v & 1u;
  const Kmer<W> key = cl_key<W>(t, slot_of[i]);
  const uint32_t nib = (ue[i] >> (4 * o)) & 15u;
  const uint32_t y = o == 0 ? 3u - kmer_first_base<W>(key, k) : (uint32_t)(key.w[W - 1] & 3u);
  uint32_t cnt = 0;
  for (uint32_t x = 0; x < 4; x++) {
    if (!((nib >> x) & 1u)) continue;
    uint32_t p = 0;
    const uint64_t s = cl_next<W>(t, key, o, x, k, p);
    if (s == kNoSlot) continue;
    const Kmer<W> kx = cl_key<W>(t, s);
    const uint32_t back = (ue[map[s]] >> (4 * (p ^ 1u))) & 15u & ~(1u << y);
    for (uint32_t z = 0; z < 4; z++) {
      if (!((back >> z) & 1u)) continue;
      uint32_t q = 0;
      const uint64_t s2 = cl_next<W>(t, kx, p ^ 1u, z, k, q);
      if (s2 != kNoSlot) out[cnt++] = 2 * map[s2] + (q ^ 1u);
    }
  }
  return cnt;
}

// mark_remove_bubbles up to the call of process_bubble.  *cursor counts every pair; those beyond cap are not
// stored (cap = 0: the counting pass).  *inside is set when a left sibling of a unitig that has right siblings too
// lies inside its unitig, which only one-sided edges allow: the reference would then walk a fragment of that unitig
// as the branch.  The flag does not wait to see whether the fragment would end at a right sibling: the call is
// refused for every such graph, also those on which the sequential rule finds no bubble there (mcx_gpu.h says so).
template <int W>
__global__ __launch_bounds__(256) void k_pop_pairs(TableView t, int k, uint64_t n, const uint64_t *slot_of, const uint32_t *map,
                                                   const uint8_t *ue, const uint32_t *uid, const uint32_t *len, const uint8_t *lk,
                                                   const uint32_t *ends, uint64_t cap, uint64_t *pairs, unsigned long long *cursor,
                                                   uint32_t *inside)
{
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += cl_stride()) {
    const uint64_t u = base + threadIdx.x;
    uint64_t mine[kPopMaxSib];
    uint32_t cnt = 0;
    if (u < n && len[u] && ends[2 * u] != kClNone) {
      uint32_t left[kPopMaxSib], right[kPopMaxSib];
      const uint32_t n1 = pop_parallel<W>(t, k, slot_of, map, ue, ends[2 * u + 1], right);
      const uint32_t n0 = n1 ? pop_parallel<W>(t, k, slot_of, map, ue, ends[2 * u], left) : 0;
      for (uint32_t a = 0; a < n0; a++) {
        const uint32_t s = left[a];
        if (!cl_end(lk, s)) { *inside = 1u; continue; }
        const uint32_t v = uid[s >> 1];
        // the branch starts at the reverse of s and runs to v's other end: ends[2v+1] when s leaves v to the left,
        // ends[2v] when s is v's last node (v is then walked backwards and ends in the reverse of its first node)
        const uint32_t last = ends[2 * (uint64_t)v] == s ? ends[2 * (uint64_t)v + 1] : ends[2 * (uint64_t)v];
        bool hit = false;
        for (uint32_t b = 0; b < n1; b++) hit |= right[b] == last;
        if (!hit) continue;
        const bool lower = kmer_less<W>(cl_key<W>(t, slot_of[ends[2 * u] >> 1]), cl_key<W>(t, slot_of[ends[2 * (uint64_t)v] >> 1]));
        mine[cnt++] = u | (uint64_t)v << 31 | (lower ? kPopLower : 0);
      }
    }
    // one reservation per wave
    uint32_t incl = cnt;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const uint32_t total = __shfl(incl, 63, 64);
    if (!total) continue;
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(cursor, (unsigned long long)total);
    at = __shfl(at, 0, 64) + incl - cnt;
    for (uint32_t a = 0; a < cnt; a++)
      if (at + a < cap) pairs[at + a] = mine[a];
  }
}

// (U -> V) is a threat when U comes first, V would be the loser (s2 goes unless mean1 < mean2) and passes -C -L -D
__global__ __launch_bounds__(256) void k_pop_mark(uint64_t np, uint64_t *pairs, const unsigned long long *sum, const uint32_t *len,
                                                  int32_t max_covg, int32_t max_klen, int32_t max_kdiff)
{
  for (uint64_t i = cl_first(); i < np; i += cl_stride()) {
    const uint64_t p = pairs[i];
    if (!(p & kPopLower)) continue;
    const uint32_t u = (uint32_t)(p & kPopIdMask), v = (uint32_t)((p >> 31) & kPopIdMask);
    const uint64_t mu = sum[u] / len[u], mv = sum[v] / len[v];
    if (mu >= mv && pop_pass(mv, len[v], len[u], max_covg, max_klen, max_kdiff)) pairs[i] = p | kPopThreat;
  }
}

// one round, first half: an undecided V is killed by a U that takes its turn, and waits for an undecided U
__global__ __launch_bounds__(256) void k_pop_threats(uint64_t np, const uint64_t *pairs, const uint8_t *state, uint8_t *kill,
                                                     uint8_t *wait)
{
  for (uint64_t i = cl_first(); i < np; i += cl_stride()) {
    const uint64_t p = pairs[i];
    if (!(p & kPopThreat)) continue;
    const uint32_t u = (uint32_t)(p & kPopIdMask), v = (uint32_t)((p >> 31) & kPopIdMask);
    if (state[v] != kPopOpen) continue;
    const uint8_t su = state[u];
    if (su == kPopTurn) kill[v] = 1;
    else if (su == kPopOpen) wait[v] = 1;
  }
}

// second half: killed -> no turn; nothing to wait for -> turn
__global__ __launch_bounds__(256) void k_pop_settle(uint64_t n, const uint32_t *len, uint8_t *state, const uint8_t *kill, uint8_t *wait,
                                                    uint32_t *changed)
{
  uint32_t ch = 0;
  for (uint64_t u = cl_first(); u < n; u += cl_stride()) {
    if (!len[u] || state[u] != kPopOpen) continue;
    if (kill[u]) { state[u] = kPopNoTurn; ch = 1; }
    else if (!wait[u]) { state[u] = kPopTurn; ch = 1; }
    wait[u] = 0;
  }
  if (ch) *changed = 1u;
}

// process_bubble for every pair whose U took its turn
__global__ __launch_bounds__(256) void k_pop_apply(uint64_t np, const uint64_t *pairs, const unsigned long long *sum, const uint32_t *len,
                                                   int32_t max_covg, int32_t max_klen, int32_t max_kdiff, const uint8_t *state,
                                                   uint8_t *keep, unsigned long long *popped)
{
  unsigned long long c = 0;
  for (uint64_t i = cl_first(); i < np; i += cl_stride()) {
    const uint64_t p = pairs[i];
    const uint32_t u = (uint32_t)(p & kPopIdMask), v = (uint32_t)((p >> 31) & kPopIdMask);
    if (state[u] != kPopTurn) continue;
    const uint64_t mu = sum[u] / len[u], mv = sum[v] / len[v];
    const bool first = mu < mv;  // remove s1, else s2
    if (!pop_pass(first ? mu : mv, first ? len[u] : len[v], first ? len[v] : len[u], max_covg, max_klen, max_kdiff)) continue;
    keep[first ? u : v] = 0;
    c++;
  }
  block_add(popped, c);
}

__global__ __launch_bounds__(256) void k_pop_count(uint64_t n, const uint32_t *len, const uint8_t *keep, unsigned long long *gone)
{
  unsigned long long c = 0;
  for (uint64_t u = cl_first(); u < n; u += cl_stride()) c += len[u] && !keep[u];
  block_add(gone, c);
}

}  // namespace mcx
