// mcx_infer.h -- `inferedges` on the device (included by mcx_api.hip).
//
// infer_kmer_edges (src/tools/infer_edges.c) for a chunk of byte-packed .ctx records in HBM: for every
// record, each edge that some colour lacks (--all) or that some colour has and another lacks (--pop)
// names a neighbour k-mer; the neighbour is looked up in the (read-only) table and, where it is
// present in colour c and the record has coverage in c, the edge is OR-ed into the record's edge byte
// of c.  A record only ever changes its own edge bytes, so there are no write conflicts.
//
// Layout: a block of 256 lanes takes a tile of up to 32 records.  The tile's bytes
// are staged into LDS with aligned 16-byte loads (records are not 4-byte aligned when ncols is odd),
// then lane l works on neighbour l % 8 of record l / 8, so the up to eight probe chains of a record
// are in flight at once instead of one after the other.  Found edges are OR-ed into the LDS copy of
// the edge bytes (LDS atomics on the aligned word that holds the byte), and the edge bytes of the
// records that changed are stored back.
#pragma once
#include "mcx_kernels.h"

namespace mcx {

constexpr int kInferThreads = 256;
constexpr int kInferMaxRecs = kInferThreads / 8;  // records per tile (eight lanes each)
constexpr uint32_t kInferLdsBudget = 60u << 10;   // dynamic LDS a tile may take
constexpr uint32_t kInferPop = 1, kInferPresenceCovg = 2;  // = MCX_INFER_POP, MCX_INFER_PRESENCE_COVG

// records per tile for a record size (0: a record does not fit the LDS budget)
__host__ __device__ inline uint32_t infer_tile_recs(uint32_t rec_bytes)
{
  const uint32_t r = (kInferLdsBudget - 48u) / rec_bytes;
  return r < (uint32_t)kInferMaxRecs ? r : (uint32_t)kInferMaxRecs;
}
__host__ __device__ inline uint32_t infer_lds_bytes(uint32_t rec_bytes)
{
  return infer_tile_recs(rec_bytes) * rec_bytes + 48u;  // + the base's alignment and a 16-byte chunk at each end
}

__device__ __forceinline__ uint32_t lds_le32(const uint8_t *p)
{
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// binary_kmer_right_shift_one_base + binary_kmer_set_first_nuc: `nuc` becomes the first base
template <int W> __device__ __forceinline__ void kmer_push_front(Kmer<W> &x, uint32_t nuc, int k)
{
  for (int i = W - 1; i > 0; i--) x.w[i] = (x.w[i] >> 2) | (x.w[i - 1] << 62);
  x.w[0] >>= 2;
  const int top = 2 * k - 2 - 64 * (W - 1);  // bit of the first base in word 0
  x.w[0] = (x.w[0] & ~(3ULL << top)) | ((uint64_t)nuc << top);
}

// ctr[0] += records modified, ctr[1] += neighbour lookups made
template <int W>
__global__ __launch_bounds__(kInferThreads) void k_infer_records(TableView t, uint8_t *recs, uint64_t nrecs, uint32_t ncols,
                                                                 int k, uint32_t flags, unsigned long long *ctr)
{
  extern __shared__ uint8_t s_dyn[];
  __shared__ uint32_t s_mod[kInferMaxRecs];
  __shared__ uint32_t s_any;
  // base of the staged bytes: 16-byte aligned whatever static LDS sits in front of the dynamic region
  uint8_t *s_tile = s_dyn + ((16u - ((uint32_t)(uintptr_t)s_dyn & 15u)) & 15u);
  const uint32_t rec_bytes = 8u * W + 5u * ncols;
  const uint32_t R = infer_tile_recs(rec_bytes);
  const uint64_t ntiles = (nrecs + R - 1) / R;
  const uint64_t total = nrecs * rec_bytes;
  const uint32_t tid = threadIdx.x, r = tid >> 3, j = tid & 7u;
  const uint32_t nuc = j & 3u, orient = j >> 2, bit = 1u << j;  // nuc_orient_to_edge
  const bool pop = flags & kInferPop, by_covg = flags & kInferPresenceCovg;
  uint32_t modified = 0, lookups = 0;

  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t r0 = tile * R;
    const uint32_t nr = (uint32_t)(nrecs - r0 < R ? nrecs - r0 : R);
    const uint64_t lo = r0 * rec_bytes, hi = lo + (uint64_t)nr * rec_bytes;  // the tile's bytes [lo, hi) of recs
    // stage [lo, hi) into LDS: 16-byte chunks aligned in global memory; a chunk that reaches outside the
    // buffer is read byte by byte (never past either end of recs)
    const uintptr_t a_lo = (uintptr_t)(recs + lo), a0 = a_lo & ~(uintptr_t)15;
    const uint32_t head = (uint32_t)(a_lo - a0);  // LDS offset of byte lo
    const uint32_t nchunks = (uint32_t)((head + (hi - lo) + 15) / 16);
    for (uint32_t c = tid; c < nchunks; c += kInferThreads) {
      const uintptr_t a = a0 + 16u * (uintptr_t)c;
      uint8_t *dst = s_tile + 16u * c;
      if (a >= (uintptr_t)recs && a + 16 <= (uintptr_t)(recs + total)) {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(a);
      } else {
        for (int b = 0; b < 16; b++) {
          const uintptr_t ab = a + b;
          dst[b] = (ab >= (uintptr_t)recs && ab < (uintptr_t)(recs + total)) ? *reinterpret_cast<const uint8_t *>(ab) : 0;
        }
      }
    }
    if (tid < (uint32_t)kInferMaxRecs) s_mod[tid] = 0;
    if (tid == 0) s_any = 0;
    __syncthreads();

    if (r < nr) {
      uint8_t *p = s_tile + head + r * rec_bytes;
      const uint8_t *pc = p + 8 * W;
      uint8_t *pe = p + 8 * W + 4 * ncols;
      uint32_t uedges = 0, iedges = 0xffu;
      for (uint32_t c = 0; c < ncols; c++) { uedges |= pe[c]; iedges &= pe[c]; }
      const uint32_t add = pop ? uedges & ~iedges : ~iedges & 0xffu;
      // look up only when some colour with coverage lacks this edge: nothing else can change
      bool want = false;
      if (add & bit)
        for (uint32_t c = 0; c < ncols && !want; c++) want = !(pe[c] & bit) && lds_le32(pc + 4 * c) != 0;
      if (want) {
        Kmer<W> nb;
#pragma unroll
        for (int w = 0; w < W; w++) {
          const uint8_t *q = p + 8 * w;
          nb.w[w] = (uint64_t)lds_le32(q) | (uint64_t)lds_le32(q + 4) << 32;
        }
        if (orient == 0) kmer_push<W>(nb, nuc, k);
        else kmer_push_front<W>(nb, 3u - nuc, k);
        const Kmer<W> rc = revcomp<W>(nb, k);
        const Kmer<W> key = kmer_less<W>(nb, rc) ? nb : rc;  // binary_kmer_get_key
        uint32_t novel = 0, full = 0;
        const uint64_t slot = find_or_insert_rec<W>(t, key, true, novel, full);  // must_exist: read-only
        lookups++;
        if (slot != kNoSlot) {
          const uint32_t base = (uint32_t)(pe - s_tile);
          for (uint32_t c = 0; c < ncols; c++) {
            if ((pe[c] & bit) || lds_le32(pc + 4 * c) == 0) continue;
            const uint64_t v = *val_ptr(t, slot, c);  // (the table is not written while this runs)
            if (by_covg ? (v >> 8) == 0 : v == 0) continue;
            // OR the bit into the edge byte through the aligned LDS word that holds it (the other bytes get 0)
            const uint32_t off = base + c;
            const uint32_t sh = 8u * (off & 3u);
            const uint32_t old = atomicOr(reinterpret_cast<uint32_t *>(s_tile + (off & ~3u)), bit << sh);
            if (!((old >> sh) & bit)) { s_mod[r] = 1; s_any = 1; }
          }
        }
      }
    }
    __syncthreads();
    // store the edge bytes of the records that changed (only the tile's own bytes are written)
    if (s_any) {
      for (uint32_t i = tid; i < nr * ncols; i += kInferThreads) {
        const uint32_t rr = i / ncols, c = i - rr * ncols;
        if (!s_mod[rr]) continue;
        const uint32_t off = head + rr * rec_bytes + 8u * W + 4u * ncols + c;
        recs[lo + (uint64_t)rr * rec_bytes + 8u * W + 4u * ncols + c] = s_tile[off];
      }
      if (tid < nr) modified += s_mod[tid];
    }
    __syncthreads();  // the next tile overwrites s_tile / s_mod
  }
  block_add(&ctr[0], modified);
  block_add(&ctr[1], lookups);
}

}  // namespace mcx
