// chunk_check.cpp -- the host read chunker (mccortex_amd/csrc/mcx_chunk.h) driven to the end of an input on the CPU.
// Built with -fsanitize=address,undefined by test_chunk_check.py; the destination buffers are heap blocks of exactly
// the size a layout allows, so a byte written past a chunk is caught.  Exits non-zero on the first violation.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "mcx_chunk.h"

using namespace mcx;

#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "%s:%d: %s failed: ", __FILE__, __LINE__, #cond);   \
      fprintf(stderr, __VA_ARGS__);                                       \
      fprintf(stderr, "\n");                                              \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

static std::string bases_of(uint64_t n, uint64_t &seed)
{
  std::string s(n, 'A');
  for (auto &ch : s) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    ch = "ACGT"[seed >> 62];
  }
  return s;
}

// One list for a layout with chunks of `cap` new bytes whose pieces advance by `stride` bases: every branch of the
// filler is reached, in this order.
static std::vector<std::string> make_reads(uint64_t k, uint64_t cap, uint64_t stride)
{
  uint64_t seed = 12345 + k + cap;
  std::vector<std::string> v;
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, k - 1, k}) v.push_back(bases_of(n, seed));
  v.push_back(bases_of(cap - 1, seed));      // fits whole, with its separator
  v.push_back(bases_of(cap, seed));          // goes in pieces
  v.push_back(bases_of(2 * cap + 5, seed));
  for (int i = 0; i < 40; i++) v.push_back(bases_of(3, seed));  // (cap = 256: the read count stops a chunk before the bytes do)
  for (uint64_t i = 0; i < cap / 16 + 8; i++) v.push_back(bases_of(3, seed));  // the same at every cap
  v.push_back(bases_of(cap - 1 + stride, seed));  // its second piece is a full one and ends the read
  v.push_back(bases_of(k + 7, seed));
  return v;
}

struct Input {
  std::vector<std::string> reads;
  std::string bases;
  std::vector<uint64_t> off;
  explicit Input(std::vector<std::string> r) : reads(std::move(r))
  {
    bases = "xx";  // (off[0] need not be 0)
    off.push_back(bases.size());
    for (const auto &s : reads) { bases += s; off.push_back(bases.size()); }
  }
  const uint8_t *data() const { return reinterpret_cast<const uint8_t *>(bases.data()); }
  uint64_t len(uint64_t r) const { return reads[r].size(); }
};

struct Seen { int count_stop = 0, full_last_piece = 0, mid_piece = 0, pieces = 0, chunks = 0; };

static void check_seen(const Seen &s, const char *what, uint64_t k, uint64_t cap)
{
  CHECK(s.count_stop && s.full_last_piece && s.mid_piece >= 3 && s.chunks > 8, "%s k=%llu cap=%llu: a branch was not reached (%d %d %d %d)", what,
        (unsigned long long)k, (unsigned long long)cap, s.count_stop, s.full_last_piece, s.mid_piece, s.chunks);
}

// carry layout; prefill: the caller places up to two whole reads itself before the filler goes on (the threaded
// prefill of mcx_graph_add_reads in small)
static void check_carry(uint64_t k, uint64_t cap, bool prefill)
{
  const Input in(make_reads(k, cap, cap - 1));
  const uint64_t nreads = in.reads.size(), max_reads = cap / 16;
  const ChunkLayout lay{kCarry, cap, max_reads, 0, false};
  std::string expect, got;
  std::vector<uint64_t> start;  // where read r starts in the stream
  for (const auto &s : in.reads) { start.push_back(expect.size()); expect += s + "\n"; }
  std::unique_ptr<uint8_t[]> buf(new uint8_t[kCarry + cap + kChunkPad]);
  std::unique_ptr<uint64_t[]> hoff(new uint64_t[max_reads + 1]);
  ReadChunker ck(in.data(), in.off.data(), nreads);
  Seen seen;
  uint64_t next = 0, piece_at = 0;  // next read, bases of it that earlier pieces took
  while (!ck.done()) {
    uint64_t n0 = 0, L0 = 0;
    if (prefill && ck.r_pos == 0)
      for (; n0 < 2 && ck.r < nreads && in.len(ck.r) + 1 <= cap - L0; n0++, ck.r++) {
        hoff[n0] = kCarry + L0;
        memcpy(buf.get() + kCarry + L0, in.reads[ck.r].data(), in.len(ck.r));
        L0 += in.len(ck.r);
        buf[kCarry + L0++] = '\n';
      }
    const Chunk c = ck.fill(lay, buf.get(), hoff.get(), n0, L0);
    seen.chunks++;
    CHECK(c.L >= 1 && c.L <= cap && c.n <= max_reads, "L=%llu n=%llu", (unsigned long long)c.L, (unsigned long long)c.n);
    const std::string before = std::string(kCarry, '\n') + got;
    CHECK(memcmp(buf.get(), before.data() + before.size() - kCarry, kCarry) == 0, "carry of chunk %d", seen.chunks);
    for (uint64_t i = 0; i < kChunkPad; i++) CHECK(buf[kCarry + c.L + i] == '\n', "pad byte %llu", (unsigned long long)i);
    CHECK(c.r0 == next, "r0=%llu next=%llu", (unsigned long long)c.r0, (unsigned long long)next);
    CHECK(hoff[c.n] == kCarry + c.L, "hoff[n]");
    if (c.piece_of >= 0) {
      seen.pieces++;
      CHECK(c.n == 0 && (uint64_t)c.piece_of == next && c.shift == piece_at, "piece of %lld at %llu", c.piece_of, (unsigned long long)c.shift);
      CHECK(piece_at > 0 || in.len(next) + 1 > cap, "a read that fits went as a piece");
      CHECK(c.ended == (c.shift + c.take == in.len(next)) && c.L == c.take + (c.ended ? 1 : 0), "piece length");
      CHECK(c.ended || c.take == cap - 1, "a piece that does not end its read is not full");
      CHECK(memcmp(buf.get() + kCarry, in.reads[next].data() + c.shift, c.take) == 0, "piece bytes");
      if (c.ended) { seen.full_last_piece += c.take == cap - 1; next++; piece_at = 0; }
      else { seen.mid_piece++; piece_at += c.take; }
    } else {
      CHECK(c.n >= 1 && piece_at == 0, "an empty chunk");
      for (uint64_t i = 0; i < c.n; i++) CHECK(hoff[i] == kCarry + start[next + i] - got.size(), "hoff[%llu]", (unsigned long long)i);
      next += c.n;
      // the chunk stopped for a reason
      const bool fits = next < nreads && in.len(next) + 1 <= cap - c.L;
      CHECK(next == nreads || c.n == max_reads || !fits, "the chunk stopped early");
      seen.count_stop += fits && c.n == max_reads;
    }
    CHECK(ck.r == next && ck.r_pos == piece_at, "cursor");
    got.append(reinterpret_cast<const char *>(buf.get()) + kCarry, c.L);
  }
  CHECK(next == nreads && got == expect, "the chunks do not add up to the stream");
  check_seen(seen, prefill ? "carry+prefill" : "carry", k, cap);
}

static void check_alone(uint64_t k, uint64_t C)
{
  const uint64_t k1 = k - 1, R = C / 16;
  const Input in(make_reads(k, C, C - 1 - k1));
  const uint64_t nreads = in.reads.size();
  const ChunkLayout lay{0, C, R, k1, true};
  std::unique_ptr<uint8_t[]> buf(new uint8_t[C]);
  std::unique_ptr<uint64_t[]> ho(new uint64_t[R + 1]);
  ReadChunker ck(in.data(), in.off.data(), nreads);
  Seen seen;
  uint64_t next = 0, owned = 0;  // next read, start positions of it that earlier pieces own
  std::vector<int> cover;        // of the read in pieces: how many pieces own each base position
  while (!ck.done()) {
    const Chunk c = ck.fill(lay, buf.get(), ho.get());
    seen.chunks++;
    CHECK(c.L >= 1 && c.L <= C && c.n >= 1 && c.n <= R, "L=%llu n=%llu", (unsigned long long)c.L, (unsigned long long)c.n);
    CHECK(ho[0] == 0 && ho[c.n] == c.L && c.r0 == next, "offsets");
    if (c.piece_of >= 0) {
      seen.pieces++;
      const uint64_t len = in.len(next);
      CHECK(c.n == 1 && (uint64_t)c.piece_of == next && c.L == c.take + 1 && buf[c.take] == '\n', "piece layout");
      CHECK(c.shift == owned, "piece starts at %llu, owned so far %llu", (unsigned long long)c.shift, (unsigned long long)owned);
      CHECK(owned > 0 || len + 1 > C, "a read that fits went as a piece");
      CHECK(c.ended == (c.shift + c.take == len), "ended");
      CHECK(c.ended || c.take == C - 1, "a piece that does not end its read is not full");
      CHECK(memcmp(buf.get(), in.reads[next].data() + c.shift, c.take) == 0, "piece bytes");
      // own: all positions but the last k - 1; the last piece owns all of its own.  [shift, shift + own) tile [0, len).
      CHECK(c.ended || c.take > k1, "a piece owns nothing");
      const uint64_t own = c.ended ? c.take : c.take - k1;
      // what the chunk says it owns, [shift, shift + min(own, take)), is that range: every base position of the read
      // falls into exactly one piece's, and the ranges come in order
      if (c.shift == 0) cover.assign(len, 0);
      CHECK(c.own == (c.ended ? ~0ull : own), "Chunk::own = %llu", (unsigned long long)c.own);
      CHECK(c.shift == owned && c.shift + std::min(c.own, c.take) <= len, "owned range");
      for (uint64_t p = c.shift; p < c.shift + std::min(c.own, c.take); p++) cover[p]++;
      if (c.ended) {
        CHECK(owned + own == len, "tiling");
        for (uint64_t p = 0; p < len; p++) CHECK(cover[p] == 1, "position %llu of read %llu is owned %d times", (unsigned long long)p, (unsigned long long)next, cover[p]);
        seen.full_last_piece += c.take == C - 1;
        next++;
        owned = 0;
      } else {
        seen.mid_piece++;
        owned += own;
      }
    } else {
      CHECK(owned == 0, "whole reads inside a read in pieces");
      CHECK(c.own == ~0ull, "whole reads own all of their own");
      for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t len = in.len(next + i);
        CHECK(ho[i + 1] == ho[i] + len + 1 && buf[ho[i + 1] - 1] == '\n', "read %llu: offsets", (unsigned long long)(next + i));
        CHECK(len == 0 || memcmp(buf.get() + ho[i], in.reads[next + i].data(), len) == 0, "read %llu: bytes", (unsigned long long)(next + i));
      }
      next += c.n;
      const bool fits = next < nreads && in.len(next) + 1 <= C - c.L;
      CHECK(next == nreads || c.n == R || !fits, "the chunk stopped early");
      seen.count_stop += fits && c.n == R;
    }
    CHECK(ck.r == next && ck.r_pos == owned, "cursor");
  }
  CHECK(next == nreads, "reads left over");
  check_seen(seen, "stand-alone", k, C);
}

// every read empty and no bases at all: nothing is read through the null pointer
static void check_empty()
{
  const uint64_t off[4] = {7, 7, 7, 7};
  uint8_t buf[256];
  uint64_t ho[17];
  ReadChunker ck(nullptr, off, 3);
  const Chunk c = ck.fill(ChunkLayout{0, 256, 16, 30, true}, buf, ho);
  CHECK(ck.done() && c.n == 3 && c.L == 3 && c.piece_of < 0 && ho[0] == 0 && ho[3] == 3 && !memcmp(buf, "\n\n\n", 3), "empty reads");
}

int main()
{
  for (uint64_t k : {31, 127}) {
    for (uint64_t C : {256, 1024}) check_alone(k, C);
    for (uint64_t cap : {848, 1024}) {
      check_carry(k, cap, false);
      check_carry(k, cap, true);
    }
  }
  check_empty();
  printf("chunk_check: ok\n");
  return 0;
}
