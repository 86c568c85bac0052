// mcx_coverage.h -- `coverage` on the device (included by mcx_api.hip).
//
// print_read_covg (src/commands/ctx_coverage.c) over a batch of reads: for every k-mer of a read that is a key of the
// table, the coverage and the edges stored for it in every colour, the edges turned to the read's strand
// (fetch_node_edges); zero for every other start position.  The passes ("coverage's device passes"):
//   A. k_cv_probe   rt_probe's walk (mcx_reads.h) with a sink that keeps the slots: per colour a lane gathers the value
//                   words of its 16 start positions and stores 64 bytes of coverage and 16 bytes of edges, so a wave
//                   writes 4 KB and 1 KB contiguous per colour.  Every position of every tile walked is written.
//      k_cv_place   (host entries only) a chunk's arrays, indexed by the chunk's stream position, into the batch's,
//                   indexed by base position (rt_place of mcx_reads.h): the separators drop out, a piece of a long read
//                   lands behind the one before it.
//   B. k_cv_len     the length of every line; a 64-bit exclusive scan of them gives line_off
//      k_cv_emit    a wave per line writes its text at line_off
// All are grid-stride loops (the "grid" knob caps the launches); the table is only read.
#pragma once
#include "mcx_reads.h"

namespace mcx {

// The sink of rt_probe that `coverage` uses.  covg / edges are colour-major with `pitch` positions per colour (a
// multiple of 64, so a lane's 16 positions are inside or outside as a whole); edges may be null.
struct CvGatherSink {
  static constexpr bool kSlots = true;
  TableView t;
  uint32_t ncols;
  uint64_t pitch;
  uint32_t *covg;
  uint8_t *edges;
  __device__ __forceinline__ void operator()(uint64_t P0, uint32_t hit16, const uint64_t (&slot)[16], uint32_t o16) const
  {
    if (P0 >= pitch) return;
    for (uint32_t c = 0; c < ncols; c++) {
      uint64_t v[kPosPerLane];
#pragma unroll
      for (int j = 0; j < kPosPerLane; j++) v[j] = ((hit16 >> j) & 1u) ? *val_ptr(t, slot[j], c) : 0ull;  // 16 loads in flight
      uint32_t cv[kPosPerLane], e[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < kPosPerLane; j++) {
        const uint64_t x = v[j] >> 8;
        cv[j] = x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x;  // COVG_MAX saturation, as the export clamps
        uint32_t eb = (uint32_t)v[j] & 0xffu;
        // fetch_node_edges: the read met the key's reverse complement -> the nibbles change places, their bits stay
        if ((o16 >> j) & 1u) eb = ((eb >> 4) | (eb << 4)) & 0xffu;
        e[j >> 2] |= eb << (8 * (j & 3));
      }
      uint4 *dc = reinterpret_cast<uint4 *>(covg + (uint64_t)c * pitch + P0);
#pragma unroll
      for (int q = 0; q < 4; q++) dc[q] = make_uint4(cv[4 * q], cv[4 * q + 1], cv[4 * q + 2], cv[4 * q + 3]);
      if (edges) *reinterpret_cast<uint4 *>(edges + (uint64_t)c * pitch + P0) = make_uint4(e[0], e[1], e[2], e[3]);
    }
  }
};

template <int W>
__global__ __launch_bounds__(kThreads) void k_cv_probe(StreamArgs a, TableView t, uint32_t ncols, uint64_t pitch, uint32_t *covg, uint8_t *edges,
                                                       unsigned long long *cnt)
{
  rt_probe<W>(a, t, CvGatherSink{t, ncols, pitch, covg, edges}, cnt);
}

// rt_place (mcx_reads.h) for the coverage and the edges of every colour
__global__ __launch_bounds__(256) void k_cv_place(const uint64_t *so, uint64_t n, const uint64_t *boff, uint64_t r0, uint64_t shift, uint64_t own,
                                                  uint32_t ncols, const uint32_t *scovg, const uint8_t *sedges, uint64_t spitch, uint32_t *covg,
                                                  uint8_t *edges, uint64_t pitch)
{
  rt_place(so, n, boff, r0, shift, own, spitch, pitch, [&](uint64_t p, uint64_t d) {
    for (uint32_t c = 0; c < ncols; c++) {
      covg[(uint64_t)c * pitch + d] = scovg[(uint64_t)c * spitch + p];
      if (edges) edges[(uint64_t)c * pitch + d] = sedges[(uint64_t)c * spitch + p];
    }
  });
}

// ---- the text ------------------------------------------------------------------------------------------------------
// Line (r * ncols + c) * lpc + j is line j of colour c of read r: the edges line if asked for, the degree line if asked
// for, the coverage line (lpc = 1 + the number of those asked for).  klen = max(len - k + 1, 0) values per line, taken at
// base positions boff[r] - boff[0] ...
struct CvText {
  const uint64_t *boff;
  uint64_t nreads;
  int k;
  uint32_t ncols, flags, lpc;  // flags: MCX_COVERAGE_*
  const uint32_t *covg;
  const uint8_t *edges;
  uint64_t pitch;
};
constexpr uint32_t kCvEdges = 1, kCvDegrees = 2;  // = MCX_COVERAGE_EDGES, MCX_COVERAGE_DEGREES

// characters "%2u" makes of v
__device__ __forceinline__ uint32_t cv_width(uint32_t v)
{
  uint32_t w = 2;
  for (uint64_t lim = 100; v >= lim; lim *= 10) w++;  // (ten digits at the most)
  return w;
}
__device__ __forceinline__ uint64_t cv_klen(const CvText &x, uint64_t r)
{
  const uint64_t len = x.boff[r + 1] - x.boff[r];
  return len >= (uint64_t)x.k ? len - (uint64_t)x.k + 1 : 0;
}

// len[line] for every line.  A lane takes a (read, colour); one with more than kRtLongStarts values is summed by the
// whole wave of the lane that met it, as k_rt_reads splits its reads.
__global__ __launch_bounds__(256) void k_cv_len(CvText x, uint64_t *len)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, nitems = x.nreads * x.ncols;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < nitems; base += stride) {
    const uint64_t it = base + threadIdx.x;
    uint64_t klen = 0, p0 = 0, r = 0;
    uint32_t c = 0;
    if (it < nitems) {
      r = it / x.ncols;
      c = (uint32_t)(it % x.ncols);
      klen = cv_klen(x, r);
      p0 = x.boff[r] - x.boff[0];
    }
    const bool is_long = klen > kRtLongStarts;
    const uint32_t *cv = x.covg + (uint64_t)c * x.pitch + p0;
    uint64_t sum = 0;
    if (!is_long)
      for (uint64_t i = 0; i < klen; i++) sum += cv_width(cv[i]);
    unsigned long long todo = __builtin_amdgcn_ballot_w64(is_long);  // (uniform per wave)
    while (todo) {
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint64_t lk = __shfl((unsigned long long)klen, src);
      const uint64_t lp = __shfl((unsigned long long)p0, src);
      const uint32_t lc = __shfl(c, src);
      const uint32_t *lcv = x.covg + (uint64_t)lc * x.pitch + lp;
      uint64_t part = 0;
      for (uint64_t i = lane; i < lk; i += 64) part += cv_width(lcv[i]);
      for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor((unsigned long long)part, d);
      if ((int)lane == src) sum = part;
    }
    if (it < nitems) {
      uint64_t *out = len + it * x.lpc;
      if (x.flags & kCvEdges) *out++ = klen ? 3 * klen : 1;
      if (x.flags & kCvDegrees) *out++ = klen + 1;
      *out = klen ? sum + klen : 1;  // klen - 1 separators and the newline
    }
  }
}

// One wave per line.  The coverage line goes in blocks of 64 values: a wave prefix sum of the widths places each value,
// the running offset is carried from one block to the next.
__global__ __launch_bounds__(256) void k_cv_emit(CvText x, const uint64_t *line_off, uint64_t line0, uint64_t nlines, uint8_t *text)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const char hex[] = "0123456789abcdef", sym[] = "./[\\-{]}X";
  for (uint64_t wv = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); wv < nlines; wv += nwaves) {
    const uint64_t line = line0 + wv;
    const uint64_t it = line / x.lpc;
    uint32_t j = (uint32_t)(line % x.lpc);
    const uint64_t r = it / x.ncols;
    const uint32_t c = (uint32_t)(it % x.ncols);
    // which of the three this line is: 0 edges, 1 degree, 2 coverage
    uint32_t kind = 2;
    if (x.flags & kCvEdges) { if (j == 0) kind = 0; else j--; }
    if (kind == 2 && (x.flags & kCvDegrees) && j == 0) kind = 1;
    const uint64_t klen = cv_klen(x, r), p0 = x.boff[r] - x.boff[0];
    uint8_t *out = text + (line_off[line] - line_off[line0]);
    if (kind == 0) {  // edges_to_char: the reverse nibble with its bits reversed, then the forward nibble
      const uint8_t *e = x.edges + (uint64_t)c * x.pitch + p0;
      for (uint64_t i = lane; i < klen; i += 64) {
        const uint32_t b = e[i], up = b >> 4;
        const uint32_t rv = ((up & 1u) << 3) | ((up & 2u) << 1) | ((up & 4u) >> 1) | ((up & 8u) >> 3);
        out[3 * i] = (uint8_t)hex[rv];
        out[3 * i + 1] = (uint8_t)hex[b & 15u];
        out[3 * i + 2] = i + 1 < klen ? ' ' : '\n';
      }
      if (!klen && lane == 0) out[0] = '\n';
    } else if (kind == 1) {  // symbols[min(indegree, 2)][min(outdegree, 2)]
      const uint8_t *e = x.edges + (uint64_t)c * x.pitch + p0;
      for (uint64_t i = lane; i < klen; i += 64) {
        const uint32_t b = e[i];
        const uint32_t in = (uint32_t)__popc(b >> 4), od = (uint32_t)__popc(b & 15u);
        out[i] = (uint8_t)sym[3u * (in < 2u ? in : 2u) + (od < 2u ? od : 2u)];
      }
      if (lane == 0) out[klen] = '\n';
    } else {
      const uint32_t *cv = x.covg + (uint64_t)c * x.pitch + p0;
      uint64_t carry = 0;
      for (uint64_t i0 = 0; i0 < klen; i0 += 64) {
        const uint64_t i = i0 + lane;
        uint32_t v = 0, w = 0, sep = 0;
        if (i < klen) { v = cv[i]; w = cv_width(v); sep = i ? 1u : 0u; }
        uint32_t incl = w + sep;
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t up = __shfl_up(incl, d);
          if ((int)lane >= d) incl += up;
        }
        if (i < klen) {
          uint8_t *at = out + carry + (incl - w - sep);
          if (sep) *at++ = ' ';
          for (int d = (int)w - 1; d >= 0; d--) {
            at[d] = (v || d == (int)w - 1) ? (uint8_t)('0' + v % 10u) : ' ';  // "%2u": one digit is padded to two
            v /= 10u;
          }
        }
        carry += __shfl(incl, 63);
      }
      if (lane == 0) out[carry] = '\n';
    }
  }
}

}  // namespace mcx
