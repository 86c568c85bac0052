// mcx_chunk.h -- host reads (bases, off, nreads) cut into the chunks a pinned staging buffer takes.  Plain C++17, no HIP:
// tests/chunk_check.cpp drives it on the CPU under the sanitizers.
// Two layouts, one filler (ReadChunker::fill):
//  * carry (mcx_graph_add_reads with MCX_PACKED=0, mcx_graph_subgraph_seed_reads): the chunks are consecutive windows of
//    ONE stream, read 0 '\n' read 1 '\n' ...  A chunk is kCarry bytes carried over from the chunk before (separators before
//    the first), then whole reads each followed by a separator.  A read that does not fit a chunk is cut into contiguous
//    pieces, each a chunk of its own, with no separator until the read ends.  kChunkPad separators follow the chunk, so
//    the 16-byte loads of the kernels stay inside the copy.  The buffer holds kCarry + cap + kChunkPad bytes.
//  * stand-alone (alone_chunks of mcx_api.hip: mcx_graph_reads_touch, coverage_batch, and correct_batch for `correct` and
//    `thread`): no carry, every chunk is a stream of its own.  Whole reads each followed by a separator, or ONE piece of a
//    read that does not fit, also followed by a separator; consecutive pieces overlap by k - 1 bases, so every k-mer of
//    the read starts in exactly one piece: a piece owns all its positions but the last k - 1, the last piece of a read
//    all of its own (Chunk::own).  The buffer holds cap bytes.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>

namespace mcx {

constexpr uint64_t kCarry = 128;    // context bytes carried between chunks
constexpr uint64_t kChunkPad = 64;  // separators behind a chunk of the carry layout

struct ChunkLayout {
  uint64_t prefix;     // kCarry (the carry layout) or 0 (stand-alone chunks)
  uint64_t cap;        // new bytes a chunk takes at most
  uint64_t max_reads;  // whole reads a chunk takes at most (>= 1; ~0ull: as many as fit)
  uint64_t overlap;    // bases that consecutive pieces of a read share: 0 or k - 1 (< cap - 1)
  bool piece_sep;      // every piece ends in a separator and is an entry of its own, not only the piece that ends its read
};

struct Chunk {
  uint64_t r0 = 0;  // first read of the chunk
  uint64_t n = 0;   // entries: whole reads, or 1 for a piece under piece_sep (0 for a piece of the carry layout)
  uint64_t L = 0;   // new bytes, separators included
  long long piece_of = -1;  // >= 0: the chunk is a piece, `take` bases of this read from base `shift` on; ended = they are its last
  uint64_t shift = 0, take = 0;
  bool ended = false;
  // The first `own` positions of each read in the chunk are the chunk's own: all of them (~0) for whole reads and for the
  // piece that ends its read; a piece before that leaves its last `overlap` positions to the next piece, which starts there.
  uint64_t own = ~0ull;
};

struct ReadChunker {
  const uint8_t *bases;  // (may be null when every read is empty)
  const uint64_t *off;
  uint64_t nreads;
  uint64_t r = 0, r_pos = 0;  // next read, first base of it that the next piece starts with
  uint8_t carry[kCarry];

  ReadChunker(const uint8_t *b, const uint64_t *o, uint64_t n) : bases(b), off(o), nreads(n) { memset(carry, '\n', kCarry); }
  bool done() const { return r >= nreads; }

  // The next chunk into buf; offs (or null) takes n + 1 offsets: offs[i] = prefix + where entry i starts, offs[n] =
  // prefix + L.  The caller may have placed the whole reads [r - n0, r) itself, L0 bytes of them (the threaded prefill of
  // mcx_graph_add_reads): the chunk goes on behind them.
  Chunk fill(const ChunkLayout &lay, uint8_t *buf, uint64_t *offs, uint64_t n0 = 0, uint64_t L0 = 0)
  {
    Chunk c;
    c.r0 = r - n0, c.n = n0, c.L = L0;
    uint8_t *hs = buf + lay.prefix;
    if (lay.prefix) memcpy(buf, carry, lay.prefix);
    while (r < nreads) {
      const uint64_t len = off[r + 1] - off[r];
      const bool whole = r_pos == 0 && len + 1 <= lay.cap - c.L && c.n < lay.max_reads;
      if (!whole && c.L) break;
      if (offs) offs[c.n] = lay.prefix + c.L;
      if (whole) {
        if (len) memcpy(hs + c.L, bases + off[r], len);
        c.L += len;
        hs[c.L++] = '\n';
        c.n++;
        r++;
        continue;
      }
      // a read longer than a chunk (or its tail): a piece on its own
      c.piece_of = (long long)r;
      c.shift = r_pos;
      c.take = std::min(len - r_pos, lay.cap - 1);
      c.ended = r_pos + c.take == len;
      if (!c.ended) c.own = c.take - lay.overlap;
      memcpy(hs, bases + off[r] + r_pos, c.take);
      c.L = c.take;
      if (c.ended || lay.piece_sep) hs[c.L++] = '\n';
      c.n = lay.piece_sep ? 1 : 0;
      if (c.ended) { r++; r_pos = 0; }
      else r_pos += c.own;
      break;
    }
    if (offs) offs[c.n] = lay.prefix + c.L;
    if (lay.prefix) {
      memcpy(carry, hs + c.L - lay.prefix, lay.prefix);  // (reaches back into this chunk's own prefix when L < prefix)
      memset(hs + c.L, '\n', kChunkPad);
    }
    return c;
  }
};

}  // namespace mcx
