// mcx_unitigs.h -- `unitigs` on the device (included by mcx_api.hip).
//
// ctx_unitigs.c over the table: every unitig of mcx_graph_unitig_stats' decomposition (mcx_clean.h), spelled as
// FASTA, GFA or DOT text by kernels.  The text is deterministic (DESIGN.md section 7 lists the deviations):
//   * every unitig is normalised (db_unitig_normalise) in all three formats: a chain starts at the end with the
//     lower key, a closed cycle at its lowest key read forwards, a single k-mer is forward;
//   * unitigs are numbered in ascending order of the key of their first k-mer and appear in that order;
//   * an edge between unitig ends is printed by _print_edge's rule with `node < next` decided by k-mer key: when the
//     key of the end k-mer is below the neighbour's, or when the two are the same k-mer and not both sides are
//     reverse.  The lines are sorted by (source unitig, left end before right end, edge base ACGT).
// Steps ("unitigs' device passes"):
//   A. rank   k_cl_links again (the cache does not keep them), k_un_init, k_un_jump: pointer jumping in place over
//             packed (distance << 32 | next) words until every chain node holds (its end, its distance to it).
//             Nodes that never reach an end lie on closed cycles: k_un_mark lists them, k_un_cyc_* find each cycle's
//             lowest key, k_un_cut removes the link that enters it on the forward strand (and the mirror link), and
//             k_un_reinit + k_un_jump rank the listed nodes alone, now chains.
//   B. order  k_un_heads: the oriented first k-mer of every unitig; LSD radix sort of those keys, word by word;
//             k_un_number: number, length, prev / next nibbles, record length; exclusive scans give 64-bit byte
//             offsets and the position of every unitig in the base array; k_un_place: per k-mer (number, rank,
//             orientation) and its one base at bases[first + rank].
//             GFA / DOT: k_un_edges fills 8 slots per unitig (2 ends x ACGT) with the line's target and length.
//   C. emit   k_un_emit is driven by the output: a thread owns 16 consecutive bytes of the chunk buffer, finds the
//             record that holds the first of them by binary search in the offsets (narrowed per block), and walks on
//             from there; an aligned full piece is one 16-byte store.  Any byte range of the text can be produced,
//             so a chunk seam may fall anywhere in a record.
// Scratch while a call runs, beside the decomposition (MCX_CLEAN_BYTES_PER_KMER): MCX_UNITIGS_BYTES_PER_KMER per
// k-mer and MCX_UNITIGS_BYTES_PER_UNITIG per unitig (mcx_gpu.h).  The table is only read.
// Every kernel is a grid-stride loop (the "grid" knob caps the launches).
#pragma once
#include "mcx_clean.h"

namespace mcx {

enum { kUnFasta = 0, kUnGfa = 1, kUnDot = 2 };
constexpr uint32_t kUnCyc = 4u, kUnCand = 8u;  // lk bits beside the two link bits: on a closed cycle, still the lowest key

__device__ __forceinline__ uint64_t un_ld(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void un_st(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__host__ __device__ __forceinline__ uint32_t un_digits(uint32_t x)
{
  uint32_t d = 1;
  while (x >= 10) { x /= 10; d++; }
  return d;
}
// digit `at` (0 = most significant) of x, which has nd digits
__device__ __forceinline__ char un_digit(uint32_t x, uint32_t nd, uint32_t at)
{
  for (uint32_t i = at + 1; i < nd; i++) x /= 10;
  return (char)('0' + x % 10);
}
// rev_nibble_lookup: the edges of the other strand (bit x -> bit 3 - x)
__device__ __forceinline__ uint32_t un_rev_nibble(uint32_t e) { return (__brev(e) >> 28) & 15u; }
// the n-th (0-based) set bit of a nibble
__device__ __forceinline__ uint32_t un_nth_bit(uint32_t nib, uint32_t nth)
{
  for (uint32_t i = 0; i < nth; i++) nib &= nib - 1;
  return (uint32_t)__ffs(nib) - 1u;
}

// word w of the key in `slot` (the flag bits live in word 0 only)
__device__ __forceinline__ uint64_t un_keyword(const TableView &t, uint64_t slot, uint32_t w)
{
  const uint64_t x = key_ptr(t, slot)[w];
  return w ? x : (x & kKeyMask);
}

__global__ __launch_bounds__(256) void k_un_init(uint64_t n2, const uint32_t *nxt0, uint64_t *pk)
{
  for (uint64_t v = cl_first(); v < n2; v += cl_stride()) {
    const uint32_t a = nxt0[v];
    pk[v] = (uint64_t)a | ((uint64_t)(a != (uint32_t)v) << 32);
  }
}

// One round of pointer jumping, in place: pk[v] = distance << 32 | node says that `node` lies `distance` links after
// v.  A word is read and written whole, so whichever of a neighbour's old and new words a thread sees is true, and
// so is the sum.  *changed = 1 when some node reached its end this round: while a chain has an unfinished node, the
// unfinished node nearest the end points at a finished one and reaches the end in this round, so a round that sets
// nothing leaves only the nodes of closed cycles unfinished.  list == nullptr: all m nodes.
__global__ __launch_bounds__(256) void k_un_jump(uint64_t m, const uint32_t *list, const uint8_t *lk, uint64_t *pk, uint32_t *changed)
{
  uint32_t ch = 0;
  for (uint64_t t = cl_first(); t < m; t += cl_stride()) {
    const uint32_t v = list ? list[t] : (uint32_t)t;
    const uint64_t x = un_ld(&pk[v]);
    const uint32_t a = (uint32_t)x;
    if (cl_end(lk, a)) continue;  // done
    const uint64_t y = un_ld(&pk[a]);
    const uint32_t b = (uint32_t)y;
    un_st(&pk[v], ((x & ~0xFFFFFFFFull) + (y & ~0xFFFFFFFFull)) | b);
    ch |= cl_end(lk, b);
  }
  if (ch) *changed = 1u;
}

// k-mers whose forward node never reached an end lie on a closed cycle (and so does their reverse node, on the
// mirror cycle): both oriented nodes go on the list, the k-mer is a candidate for its cycle's lowest key
__global__ __launch_bounds__(256) void k_un_mark(uint64_t n, uint8_t *lk, const uint64_t *pk, uint32_t *list, unsigned long long *count)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    if (cl_end(lk, (uint32_t)pk[2 * i])) continue;
    lk[i] |= (uint8_t)(kUnCyc | kUnCand);
    const unsigned long long at = atomicAdd(count, 2ull);
    list[at] = (uint32_t)(2 * i);
    list[at + 1] = (uint32_t)(2 * i + 1);
  }
}

// The lowest key of every cycle, one key word per step, most significant first: reset, take the minimum of word w
// over the candidates, drop the candidates above it.  mk is indexed by unitig id.
__global__ __launch_bounds__(256) void k_un_cyc_reset(uint64_t m, const uint32_t *list, const uint32_t *uid, unsigned long long *mk)
{
  for (uint64_t t = cl_first(); t < m; t += cl_stride())
    if (!(list[t] & 1u)) mk[uid[list[t] >> 1]] = ~0ull;
}
__global__ __launch_bounds__(256) void k_un_cyc_min(TableView t, uint64_t m, const uint32_t *list, const uint64_t *slot_of, const uint32_t *uid,
                                                    const uint8_t *lk, uint32_t w, unsigned long long *mk)
{
  for (uint64_t j = cl_first(); j < m; j += cl_stride()) {
    const uint32_t v = list[j], i = v >> 1;
    if ((v & 1u) || !(lk[i] & kUnCand)) continue;
    atomicMin(&mk[uid[i]], (unsigned long long)un_keyword(t, slot_of[i], w));
  }
}
__global__ __launch_bounds__(256) void k_un_cyc_keep(TableView t, uint64_t m, const uint32_t *list, const uint64_t *slot_of, const uint32_t *uid,
                                                     uint8_t *lk, uint32_t w, const unsigned long long *mk)
{
  for (uint64_t j = cl_first(); j < m; j += cl_stride()) {
    const uint32_t v = list[j], i = v >> 1;
    if ((v & 1u) || !(lk[i] & kUnCand)) continue;
    if (un_keyword(t, slot_of[i], w) != mk[uid[i]]) lk[i] &= (uint8_t)~kUnCand;
  }
}

// The one candidate left per cycle is its lowest key M.  The link that enters 2M (M read forwards) comes from
// P = nxt0[2M + 1] ^ 1; P loses its out link, and so does 2M + 1 on the mirror cycle: what remains is a chain from M
// to P whose lower end key is M's.  No other thread of this launch writes these two bytes.
__global__ __launch_bounds__(256) void k_un_cut(uint64_t m, const uint32_t *list, const uint32_t *nxt0, uint8_t *lk, unsigned long long *ncycles)
{
  for (uint64_t j = cl_first(); j < m; j += cl_stride()) {
    const uint32_t v = list[j], i = v >> 1;
    if ((v & 1u) || !(lk[i] & kUnCand)) continue;
    const uint32_t p = nxt0[v + 1] ^ 1u;
    lk[i] &= (uint8_t)~2u;
    lk[p >> 1] &= (uint8_t)~(1u << (p & 1u));
    atomicAdd(ncycles, 1ull);
  }
}
__global__ __launch_bounds__(256) void k_un_reinit(uint64_t m, const uint32_t *list, const uint32_t *nxt0, const uint8_t *lk, uint64_t *pk)
{
  for (uint64_t j = cl_first(); j < m; j += cl_stride()) {
    const uint32_t v = list[j];
    pk[v] = cl_end(lk, v) ? (uint64_t)v : ((uint64_t)nxt0[v] | (1ull << 32));
  }
}

// At an end k-mer of a unitig: the two ends are A = the end behind i (read along i forwards the unitig starts there)
// and B = the end ahead.  The normalised unitig starts at the one with the lower key, read away from that end; a
// single k-mer is forward.  The start k-mer appends itself to `starts` and fills head[unitig id].
template <int W>
__global__ __launch_bounds__(256) void k_un_heads(TableView t, uint64_t n, const uint64_t *slot_of, const uint32_t *uid, const uint64_t *pk,
                                                  uint32_t *head, uint64_t *starts, unsigned long long *count)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const uint64_t x0 = pk[2 * i], x1 = pk[2 * i + 1];
    if ((x0 >> 32) && (x1 >> 32)) continue;  // inside
    const uint32_t a = (uint32_t)x1 ^ 1u, b = (uint32_t)x0;
    uint32_t h = (uint32_t)(2 * i);
    if ((a >> 1) != (b >> 1)) h = kmer_less<W>(cl_key<W>(t, slot_of[a >> 1]), cl_key<W>(t, slot_of[b >> 1])) ? a : (b ^ 1u);
    if ((h >> 1) != (uint32_t)i) continue;
    head[uid[i]] = h;
    starts[atomicAdd(count, 1ull)] = i;
  }
}

// the items of `perm` (dense ids here, compacted entries in the export) -> key word w of their k-mers (the sort's next digit)
__global__ __launch_bounds__(256) void k_un_keyword(TableView t, uint64_t nu, const uint64_t *slot_of, const uint64_t *perm, uint32_t w, uint64_t *dst)
{
  for (uint64_t j = cl_first(); j < nu; j += cl_stride()) dst[j] = un_keyword(t, slot_of[perm[j]], w);
}

__host__ __device__ __forceinline__ uint32_t un_head_len(int fmt, uint32_t num, uint32_t pn)
{
  const uint32_t d = un_digits(num);
  if (fmt == kUnFasta) return 7u + d + 6u + (uint32_t)__builtin_popcount(pn & 15u) + 6u + (uint32_t)__builtin_popcount(pn >> 4) + 1u;
  if (fmt == kUnGfa) return 6u + d + 1u;  // "S\tnode" <i> "\t"
  return 6u + d + 8u;                     // "  node" <i> " [label="
}
__host__ __device__ __forceinline__ uint32_t un_tail_len(int fmt) { return fmt == kUnDot ? 2u : 1u; }

// unitig number j (sorted[j] = dense id of its first k-mer): its oriented first and last node, length, the prev and
// next nibbles of the printed strand, and the length of its record
__global__ __launch_bounds__(256) void k_un_number(uint64_t nu, int fmt, int k, const uint64_t *sorted, const uint32_t *uid, const uint32_t *len,
                                                   const uint32_t *head, const uint64_t *pk, const uint8_t *ue, uint32_t *unum, uint32_t *ufirst,
                                                   uint32_t *ulast, uint32_t *ulen, uint8_t *upn, uint64_t *reclen)
{
  for (uint64_t j = cl_first(); j < nu; j += cl_stride()) {
    const uint32_t u = uid[sorted[j]], h = head[u], e = (uint32_t)pk[h], L = len[u];
    unum[u] = (uint32_t)j;
    ufirst[j] = h;
    ulast[j] = e;
    ulen[j] = L;
    const uint32_t prev = un_rev_nibble((ue[h >> 1] >> (4 * ((h & 1u) ^ 1u))) & 15u), next = (ue[e >> 1] >> (4 * (e & 1u))) & 15u;
    const uint32_t pn = prev | (next << 4);
    upn[j] = (uint8_t)pn;
    reclen[j] = (uint64_t)un_head_len(fmt, (uint32_t)j, pn) + (uint64_t)(k - 1) + L + un_tail_len(fmt);
  }
}

// per k-mer: unitig number, rank and orientation in the normalised unitig, and the base it adds to the sequence
template <int W>
__global__ __launch_bounds__(256) void k_un_place(TableView t, int k, uint64_t n, const uint64_t *slot_of, const uint32_t *uid, const uint32_t *head,
                                                  const uint32_t *unum, const uint64_t *pk, const uint32_t *ubase, uint32_t *kun, uint32_t *krk,
                                                  uint8_t *kori, uint8_t *bases)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const uint32_t u = uid[i], h = head[u], j = unum[u];
    const uint64_t x0 = pk[2 * i], x1 = pk[2 * i + 1];
    const uint32_t o = ((uint32_t)x1 ^ 1u) == h ? 0u : 1u;
    const uint32_t r = (uint32_t)((o ? x0 : x1) >> 32);
    kun[i] = j;
    krk[i] = r;
    kori[i] = (uint8_t)o;
    const uint64_t *key = key_ptr(t, slot_of[i]);
    const uint32_t nuc = o ? 3u - ((uint32_t)(key[0] >> (2 * k - 2 - 64 * (W - 1))) & 3u) : (uint32_t)(key[W - 1] & 3u);
    if ((uint64_t)ubase[j] + r < n) bases[(uint64_t)ubase[j] + r] = (uint8_t)"ACGT"[nuc];  // (always, when the ranks agree with the lengths)
  }
}

// The edges that leave the two ends of unitig j: slot 8 j + 4 side + x (side 0 = left end, leaving backwards) holds
// the line's target (number << 1 | reverse) and its length, 0 when there is no such edge or the rule gives the
// line to the other end.  An edge whose neighbour is absent is skipped (the reference asserts there).
template <int W>
__global__ __launch_bounds__(256) void k_un_edges(TableView t, int k, int fmt, uint64_t nu, const uint64_t *slot_of, const uint32_t *map, const uint8_t *ue,
                                                  const uint32_t *ufirst, const uint32_t *ulast, const uint32_t *kun, const uint32_t *krk,
                                                  const uint8_t *kori, uint32_t *etgt, uint8_t *elen)
{
  const uint32_t dk = un_digits((uint32_t)(k - 1));
  for (uint64_t s = cl_first(); s < 2 * nu; s += cl_stride()) {
    const uint64_t j = s >> 1;
    const uint32_t side = (uint32_t)(s & 1u);
    const uint32_t node = side ? ulast[j] : (ufirst[j] ^ 1u);
    const uint32_t nib = (ue[node >> 1] >> (4 * (node & 1u))) & 15u;
    const uint64_t slot = slot_of[node >> 1];
    Kmer<W> key;
    if (nib) key = cl_key<W>(t, slot);
    for (uint32_t x = 0; x < 4; x++) {
      uint32_t tg = 0, ln = 0;
      if ((nib >> x) & 1u) {
        uint32_t p = 0;
        const uint64_t s2 = cl_next<W>(t, key, node & 1u, x, k, p);
        if (s2 != kNoSlot) {
          const uint32_t i2 = map[s2];
          const uint32_t rev1 = (krk[i2] == 0 && p == kori[i2]) ? 0u : 1u, rev0 = side ^ 1u;
          const bool print = s2 == slot ? !(rev0 && rev1) : kmer_less<W>(key, cl_key<W>(t, s2));
          if (print) {
            const uint32_t v = kun[i2];
            tg = (v << 1) | rev1;
            ln = fmt == kUnGfa ? 18u + un_digits((uint32_t)j) + un_digits(v) + dk : 19u + un_digits((uint32_t)j) + un_digits(v);
          }
        }
      }
      etgt[8 * j + 4 * side + x] = tg;
      elen[8 * j + 4 * side + x] = (uint8_t)ln;
    }
  }
}

// ---- emit ----------------------------------------------------------------------------------------------------
struct UnUnits {  // the unitig records: off[0 .. nrec] are their byte offsets within the section
  TableView t;
  int k, fmt, W;
  uint64_t nrec, n;
  const uint64_t *off, *slot_of;
  const uint32_t *ufirst, *ubase;
  const uint8_t *upn, *bases;
};
struct UnEdges {  // the edge lines: off[0 .. nrec], nrec = 8 x unitigs
  int k, fmt;
  uint64_t nrec;
  const uint64_t *off;
  const uint32_t *etgt;
};

// base s of the sequence of unitig j whose oriented first node is h
__device__ __forceinline__ char un_seq_char(const UnUnits &a, uint64_t j, uint32_t h, uint64_t s)
{
  if (s >= (uint64_t)(a.k - 1)) {
    const uint64_t at = (uint64_t)a.ubase[j] + s - (uint64_t)(a.k - 1);
    return at < a.n ? (char)a.bases[at] : '?';
  }
  const uint32_t b = (h & 1u) ? (uint32_t)(a.k - 1) - (uint32_t)s : (uint32_t)s;  // base of the key, 0 = first
  const uint32_t bit = 2u * ((uint32_t)(a.k - 1) - b);
  const uint32_t nuc = (uint32_t)(key_ptr(a.t, a.slot_of[h >> 1])[a.W - 1 - (int)(bit >> 6)] >> (bit & 63u)) & 3u;
  return "ACGT"[(h & 1u) ? 3u - nuc : nuc];
}

// byte q of the record of unitig j (rl = its length)
__device__ char un_char(const UnUnits &a, uint64_t j, uint64_t q, uint64_t rl)
{
  const uint32_t num = (uint32_t)j, d = un_digits(num), pn = a.upn[j];
  const uint32_t hl = un_head_len(a.fmt, num, pn), tl = un_tail_len(a.fmt);
  if (q >= rl - tl) return (a.fmt == kUnDot && q == rl - 2) ? ']' : '\n';
  if (q >= hl) return un_seq_char(a, j, a.ufirst[j], q - hl);
  uint32_t c = (uint32_t)q;
  if (a.fmt == kUnFasta) {
    if (c < 7u) return ">unitig"[c];
    c -= 7u;
    if (c < d) return un_digit(num, d, c);
    c -= d;
    if (c < 6u) return " prev="[c];
    c -= 6u;
    const uint32_t np = (uint32_t)__popc(pn & 15u);
    if (c < np) return "ACGT"[un_nth_bit(pn & 15u, c)];
    c -= np;
    if (c < 6u) return " next="[c];
    c -= 6u;
    const uint32_t nn = (uint32_t)__popc(pn >> 4);
    if (c < nn) return "ACGT"[un_nth_bit(pn >> 4, c)];
    return '\n';
  }
  if (c < 6u) return a.fmt == kUnGfa ? "S\tnode"[c] : "  node"[c];
  c -= 6u;
  if (c < d) return un_digit(num, d, c);
  c -= d;
  return a.fmt == kUnGfa ? '\t' : " [label="[c];
}

// byte q of edge line e (slot 8 j + 4 side + x)
__device__ char un_char(const UnEdges &a, uint64_t e, uint64_t q, uint64_t)
{
  const uint32_t j = (uint32_t)(e >> 3), rev0 = ((uint32_t)(e >> 2) & 1u) ^ 1u, tg = a.etgt[e], v = tg >> 1, rev1 = tg & 1u;
  const uint32_t dj = un_digits(j), dv = un_digits(v);
  uint32_t c = (uint32_t)q;
  if (c < 6u) return a.fmt == kUnGfa ? "L\tnode"[c] : "  node"[c];
  c -= 6u;
  if (c < dj) return un_digit(j, dj, c);
  c -= dj;
  if (a.fmt == kUnGfa) {  // \t <o> \tnode <v> \t <o> \t <k-1> M \n
    if (c < 2u) return c == 0u ? '\t' : "+-"[rev0];
    c -= 2u;
    if (c < 5u) return "\tnode"[c];
    c -= 5u;
    if (c < dv) return un_digit(v, dv, c);
    c -= dv;
    if (c < 3u) return c == 1u ? "+-"[rev1] : '\t';
    c -= 3u;
    const uint32_t dk = un_digits((uint32_t)(a.k - 1));
    if (c < dk) return un_digit((uint32_t)(a.k - 1), dk, c);
    return c == dk ? 'M' : '\n';
  }
  if (c < 2u) return c == 0u ? ':' : "ew"[rev0];  // : <e|w> " -> node" <v> : <w|e> \n
  c -= 2u;
  if (c < 8u) return " -> node"[c];
  c -= 8u;
  if (c < dv) return un_digit(v, dv, c);
  c -= dv;
  return c == 0u ? ':' : c == 1u ? "we"[rev1] : '\n';
}

// the last record r in [lo, hi] with off[r] <= p
__device__ __forceinline__ uint64_t un_find(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t p)
{
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Bytes [p0, p0 + cnt) of a section go to dst[at .. at + cnt): a thread's window is an aligned 16-byte piece of dst,
// a tile is 256 windows; the tile's first and last record are found once per block.  cnt > 0.
template <class A>
__global__ __launch_bounds__(256) void k_un_emit(A a, uint64_t p0, uint64_t cnt, uint8_t *dst, uint64_t at)
{
  __shared__ uint64_t s_lo, s_hi;
  const uint64_t *off = a.off;
  const uint64_t w0 = at / 16, w1 = (at + cnt + 15) / 16;  // windows [w0, w1)
  for (uint64_t tile = w0 + (uint64_t)blockIdx.x * 256; tile < w1; tile += (uint64_t)gridDim.x * 256) {
    const uint64_t tb = max(tile * 16, at), te = min((tile + 256) * 16, at + cnt);  // buffer bytes of the tile
    __syncthreads();
    if (threadIdx.x == 0) s_lo = un_find(off, 0, a.nrec - 1, p0 + (tb - at));
    if (threadIdx.x == 64) s_hi = un_find(off, 0, a.nrec - 1, p0 + (te - 1 - at));
    __syncthreads();
    const uint64_t b0 = max((tile + threadIdx.x) * 16, at), b1 = min((tile + threadIdx.x + 1) * 16, at + cnt);
    if (b0 >= b1) continue;
    const uint64_t p = p0 + (b0 - at);
    uint64_t r = un_find(off, s_lo, s_hi, p), q = p - off[r], rl = off[r + 1] - off[r];
    union { uint8_t c[16]; uint4 v; } out;
    const uint32_t nb = (uint32_t)(b1 - b0);
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
      if (i < nb) {
        out.c[i] = (uint8_t)un_char(a, r, q, rl);
        if (++q == rl && i + 1 < nb) {
          do { r++; rl = off[r + 1] - off[r]; } while (rl == 0);  // (edge slots may be empty; bytes remain, so a record follows)
          q = 0;
        }
      }
    }
    if (nb == 16) *reinterpret_cast<uint4 *>(dst + b0) = out.v;
    else
      for (uint32_t i = 0; i < 16; i++)
        if (i < nb) dst[b0 + i] = out.c[i];
  }
}

// the keys of the dense ids, W words each (mcx_graph_unitigs_dev)
template <int W> __global__ __launch_bounds__(256) void k_un_keys(TableView t, uint64_t n, const uint64_t *slot_of, uint64_t *out)
{
  for (uint64_t i = cl_first(); i < n; i += cl_stride()) {
    const Kmer<W> key = cl_key<W>(t, slot_of[i]);
    for (int w = 0; w < W; w++) out[i * W + w] = key.w[w];
  }
}

__global__ __launch_bounds__(256) void k_un_narrow(uint64_t nu, const uint64_t *in, uint32_t *out)
{
  for (uint64_t j = cl_first(); j < nu; j += cl_stride()) out[j] = (uint32_t)in[j];
}
// oriented first node -> dense id of the first k-mer
__global__ __launch_bounds__(256) void k_un_first(uint64_t nu, const uint32_t *ufirst, uint32_t *out)
{
  for (uint64_t j = cl_first(); j < nu; j += cl_stride()) out[j] = ufirst[j] >> 1;
}

// a literal piece of the text (the preamble, the blank line, the closing brace)
struct UnText { char s[160]; };
__global__ void k_un_text(UnText x, uint64_t from, uint64_t cnt, uint8_t *dst)
{
  for (uint64_t i = threadIdx.x; i < cnt; i += blockDim.x) dst[i] = (uint8_t)x.s[from + i];
}

}  // namespace mcx
