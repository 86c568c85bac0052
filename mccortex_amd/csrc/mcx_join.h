// mcx_join.h -- `join` on the device (included by mcx_api.hip, behind the sort helpers it uses).
//
// Merging .ctx files (src/commands/ctx_join.c, graph_writer_merge_mkhdr) without a hash table: the inputs arrive as
// records, each key at most once per file, so the engine sorts and reduces instead of probing (DESIGN.md section 4,
// "join's device passes").  There is no capacity to guess, nothing can be full and the output is key-sorted.
//   A. k_join_extract  (per mcx_join_add_records call) the uploaded records stay in HBM as they came, byte-packed with
//                      the file's own colour count; the kernel applies graph_load's keep_kmer test
//                      (graphs_load.c:121-124: coverage in some selected colour) and appends one 64-bit locator
//                      (call << 40 | record) per kept record.  HBM: the input bytes + 8 per record, whatever out_ncols is.
//   B. sort_perm_by_words over the locators, the key words fetched through them from the records (k_join_word)
//   C. k_join_heads, a scan, k_join_runs: run id of every item, first item of every run
//   D. k_join_isec     per run: is the key in every intersection source (ctx_join.c:262-306 as it behaves with
//                      --ncols 1; with more colours in memory the reference indexes covgs[node] and the edge mask with
//                      the wrong stride), the edge mask of source rank 0, is the run written; a scan places the output
//   E. k_join_reduce   a block per tile of consecutive output records: the items of the tile's runs x slices of their
//                      colour filters are dealt over the whole block (a run of hundreds of sources, or a file of hundreds
//                      of colours, is shared by all waves), summed into LDS (SAFE_ADD_COVG saturation, edge OR under the
//                      mask), packed into the byte image of the records in LDS and stored with 16-byte writes.
// The output goes out in chunks of "out_chunk" bytes; a seam may fall inside a record.
// Out of scope: inputs whose items, sort scratch or output chunk do not fit the free HBM are refused with MCX_ERR_NOMEM;
// splitting the key range into several passes is not implemented.
#pragma once

namespace mcx {

struct JoinCall {
  const uint8_t *recs;
  uint64_t nrecs;
  uint32_t rec_bytes, file_ncols;
  int32_t source;  // -1: an input graph, >= 0: intersection source of that rank
  uint32_t nmap, map_off, pad;
};
constexpr int kJoinIdxBits = 40;
constexpr uint64_t kJoinIdxMask = (1ull << kJoinIdxBits) - 1;

// 32 bits at any byte address by aligned words and a shift (the buffers are padded, so the second word is always there)
__device__ __forceinline__ uint32_t join_load32(const uint8_t *p)
{
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3u) * 8u;
  const uint32_t lo = q[0];
  if (!sh) return lo;
  return (lo >> sh) | (q[1] << (32u - sh));
}
__device__ __forceinline__ uint64_t join_load64(const uint8_t *p) { return (uint64_t)join_load32(p) | (uint64_t)join_load32(p + 4) << 32; }
// the record of a locator; *c = its call (read in place: a caller that wants only the record loads two fields of it)
__device__ __forceinline__ const uint8_t *join_rec(const JoinCall *calls, uint64_t loc, const JoinCall **c)
{
  const JoinCall *q = calls + (loc >> kJoinIdxBits);
  *c = q;
  return q->recs + (loc & kJoinIdxMask) * q->rec_bytes;
}

// A. keep_kmer and the locator of every kept record of one call
__global__ __launch_bounds__(256) void k_join_extract(const uint8_t *recs, uint64_t n, uint32_t rec_bytes, uint32_t key_bytes, const int32_t *from,
                                                      uint32_t nmap, uint64_t tag, uint64_t *loc, unsigned long long *count)
{
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {  // (whole waves: wave_append)
    const uint64_t i = base + threadIdx.x;
    uint32_t any = 0;
    if (i < n) {
      const uint8_t *pc = recs + i * rec_bytes + key_bytes;
      for (uint32_t m = 0; m < nmap; m++) any |= join_load32(pc + 4 * from[m]);
    }
    const uint64_t at = wave_append(count, any != 0);
    if (any) loc[at] = tag | i;
  }
}

// B. word w (0 = most significant) of the keys of items[i]
__global__ __launch_bounds__(256) void k_join_word(const uint64_t *items, const JoinCall *calls, uint32_t w, uint64_t *dst, uint64_t n)
{
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const JoinCall *c;
    const uint8_t *p = join_rec(calls, items[i], &c);
    dst[i] = join_load64(p + 8 * w);
  }
}

// C. head[i] = 1 where item i starts a run behind item 0 (the inclusive sum of these is the run id)
__global__ __launch_bounds__(256) void k_join_heads(const uint64_t *items, const JoinCall *calls, uint32_t W, uint64_t *head, uint64_t n)
{
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t h = 0;
    if (i) {
      const JoinCall *ca, *cb;
      const uint8_t *a = join_rec(calls, items[i - 1], &ca), *b = join_rec(calls, items[i], &cb);
      for (uint32_t w = 0; w < W; w++) h |= (uint64_t)(join_load64(a + 8 * w) != join_load64(b + 8 * w));
    }
    head[i] = h;
  }
}
// ex = exclusive scan of head -> run id in place; runstart[run] = first item, runstart[nruns] = n
__global__ __launch_bounds__(256) void k_join_runs(const uint64_t *head, uint64_t *ex, uint64_t *runstart, uint64_t n)
{
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t run = ex[i] + head[i];
    ex[i] = run;
    if (!i || head[i]) runstart[run] = i;
    if (i == n - 1) runstart[run + 1] = n;
  }
}

// D. per run: in the intersection?  written?  the edge mask of intersection source 0.  ctr: [0] keys of the
// intersection, [1] runs written without an input record.
// Limitation: one thread takes a whole run, and walks it once per 64 intersection sources.  Runs are as long as the
// number of files that hold the key, so this is a few items for most keys; a key held by hundreds of files, or a join
// with more than 64 `-i` graphs, serialises on one lane here (k_join_reduce, where the bytes are, shares such a run
// over the block).  Without `-i` the loop is not entered.  A wave per long run is the form to move to if this shows.
__global__ __launch_bounds__(256) void k_join_isec(const uint64_t *items, const uint64_t *runstart, uint64_t nruns, const JoinCall *calls,
                                                   const int32_t *from, uint32_t key_bytes, uint32_t n_isec, uint32_t keep_empty, uint8_t *runw,
                                                   uint8_t *runmask, uint64_t *wflag, unsigned long long *ctr)
{
  for (uint64_t run = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; run < nruns; run += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t mask = 0xffu, w = 1;
    if (n_isec) {
      const uint64_t s = runstart[run], e = runstart[run + 1];
      uint64_t ninput = 0;
      bool all = true;
      mask = 0;
      for (uint32_t base = 0; base < n_isec; base += 64) {
        uint64_t bits = 0;
        for (uint64_t i = s; i < e; i++) {
          const JoinCall *c;
          const uint8_t *p = join_rec(calls, items[i], &c);
          if (c->source < 0) { ninput += base == 0; continue; }
          const uint32_t src = (uint32_t)c->source;
          if (src >= base && src < base + 64) bits |= 1ull << (src - base);
          if (src == 0 && base == 0) {
            const uint8_t *pe = p + key_bytes + 4 * c->file_ncols;
            for (uint32_t m = 0; m < c->nmap; m++) mask |= pe[from[c->map_off + m]];
          }
        }
        const uint32_t need = n_isec - base < 64 ? n_isec - base : 64;
        if (bits != (need == 64 ? ~0ull : (1ull << need) - 1)) all = false;
      }
      w = all && (ninput || keep_empty);
      if (all) table_count_slow(ctr);
      if (w && !ninput) table_count_slow(ctr + 1);
    }
    runw[run] = (uint8_t)w;
    runmask[run] = (uint8_t)mask;
    wflag[run] = w;
  }
}
__global__ __launch_bounds__(256) void k_join_outrun(const uint8_t *runw, const uint64_t *outidx, uint64_t nruns, uint64_t *outrun)
{
  for (uint64_t run = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; run < nruns; run += (uint64_t)gridDim.x * blockDim.x)
    if (runw[run]) outrun[outidx[run]] = run;
}

struct JoinReduce {
  const uint64_t *items, *runid, *runstart, *outidx, *outrun;
  const uint8_t *runw, *runmask;
  const JoinCall *calls;
  const int32_t *from, *into;
  uint32_t W, ncols, rec_bytes, P, T;
  uint64_t o0, o1;  // output records of this launch
  uint8_t *dst;     // 16-byte aligned; byte 0 is byte 0 of record o0
};

__device__ __forceinline__ void join_sat_add(uint32_t *p, uint32_t cv)
{
  uint32_t old = *p;
  for (;;) {
    const uint32_t sum = old + cv, nv = sum < old ? 0xFFFFFFFFu : sum;  // SAFE_ADD_COVG
    if (nv == old) return;
    const uint32_t seen = atomicCAS(p, old, nv);
    if (seen == old) return;
    old = seen;
  }
}

// Limitation: a tile walks every item between its first and its last written run, those of unwritten runs in between
// included (they are skipped on !runw).  Without `-i` every run is written and nothing is skipped; with a sparse
// intersection -- few output keys among many input keys -- a tile's span grows with the ratio and the blocks' work is
// uneven.  The answers do not depend on it.  Not measured (tools/bench_join.py has no `-i`); compacting the kept items
// behind k_join_isec is the remedy.
// E. LDS: the byte image of the tile's records at the alignment it has in dst (T * rec_bytes + 16, rounded to 16), then
// T x ncols coverage sums and T x ceil(ncols / 4) words of edge bytes
__global__ __launch_bounds__(256) void k_join_reduce(JoinReduce a)
{
  extern __shared__ uint4 s_join[];
  uint8_t *img = reinterpret_cast<uint8_t *>(s_join);
  const uint32_t img_bytes = ((a.T * a.rec_bytes + 16u) + 15u) & ~15u, ew = (a.ncols + 3u) / 4u;
  uint32_t *accc = reinterpret_cast<uint32_t *>(img + img_bytes), *acce = accc + (size_t)a.T * a.ncols;
  const uint32_t key_bytes = 8u * a.W;
  const uint64_t nout = a.o1 - a.o0, ntiles = (nout + a.T - 1) / a.T;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t t0 = a.o0 + tile * a.T, t1 = t0 + a.T < a.o1 ? t0 + a.T : a.o1;
    const uint32_t nt = (uint32_t)(t1 - t0);
    for (uint32_t u = threadIdx.x; u < nt * (a.ncols + ew); u += blockDim.x) {
      if (u < nt * a.ncols) accc[u] = 0;
      else acce[u - nt * a.ncols] = 0;
    }
    __syncthreads();
    const uint64_t i0 = a.runstart[a.outrun[t0]], i1 = a.runstart[a.outrun[t1 - 1] + 1];
    for (uint64_t u = threadIdx.x; u < (i1 - i0) * a.P; u += blockDim.x) {
      const uint64_t i = i0 + u / a.P;
      const uint32_t slice = (uint32_t)(u % a.P);
      const uint64_t run = a.runid[i];
      if (!a.runw[run]) continue;  // a key outside the intersection
      const JoinCall *c;
      const uint8_t *p = join_rec(a.calls, a.items[i], &c);
      if (c->source >= 0) continue;  // intersection graphs are not merged into the output
      const uint32_t r = (uint32_t)(a.outidx[run] - t0), mask = a.runmask[run];
      const uint32_t nmap = c->nmap, map_off = c->map_off;
      const uint8_t *pc = p + key_bytes, *pe = pc + 4 * c->file_ncols;
      for (uint32_t m = slice; m < nmap; m += a.P) {
        const uint32_t f = (uint32_t)a.from[map_off + m], col = (uint32_t)a.into[map_off + m];
        const uint32_t cv = join_load32(pc + 4 * f), e = pe[f] & mask;
        if (cv) join_sat_add(&accc[r * a.ncols + col], cv);
        if (e) atomicOr(&acce[r * ew + (col >> 2)], e << (8u * (col & 3u)));
      }
    }
    __syncthreads();
    uint8_t *g0 = a.dst + (t0 - a.o0) * a.rec_bytes, *g1 = g0 + (uint64_t)nt * a.rec_bytes;
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(g0) & 15u);
    for (uint32_t u = threadIdx.x; u < nt * a.W; u += blockDim.x) {  // the key: that of the run's first item
      const uint32_t r = u / a.W, w = u % a.W;
      const JoinCall *c;
      const uint8_t *p = join_rec(a.calls, a.items[a.runstart[a.outrun[t0 + r]]], &c);
      const uint64_t x = join_load64(p + 8 * w);
      uint8_t *d = img + lead + r * a.rec_bytes + 8 * w;
      for (int b = 0; b < 8; b++) d[b] = (uint8_t)(x >> (8 * b));
    }
    for (uint32_t u = threadIdx.x; u < nt * a.ncols; u += blockDim.x) {
      const uint32_t r = u / a.ncols, col = u % a.ncols, cv = accc[u];
      uint8_t *d = img + lead + r * a.rec_bytes + key_bytes;
      for (int b = 0; b < 4; b++) d[4 * col + b] = (uint8_t)(cv >> (8 * b));
      d[4 * a.ncols + col] = (uint8_t)(acce[r * ew + (col >> 2)] >> (8u * (col & 3u)));
    }
    __syncthreads();
    uint8_t *m0 = g0 + ((16u - lead) & 15u), *m1 = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g1) & ~(uintptr_t)15);
    if (m0 > g1) m0 = g1;
    if (m1 < m0) m1 = m0;
    const uint8_t *simg = img + lead;  // image byte of g0
    for (uint32_t u = threadIdx.x; u < (uint32_t)(m0 - g0); u += blockDim.x) g0[u] = simg[u];
    for (uint32_t u = threadIdx.x; u < (uint32_t)(g1 - m1); u += blockDim.x) m1[u] = simg[(m1 - g0) + u];
    const uint4 *s16 = reinterpret_cast<const uint4 *>(simg + (m0 - g0));  // (lead + (m0 - g0) is a multiple of 16)
    uint4 *d16 = reinterpret_cast<uint4 *>(m0);
    for (uint32_t u = threadIdx.x; u < (uint32_t)((m1 - m0) >> 4); u += blockDim.x) d16[u] = s16[u];
    __syncthreads();
  }
}

}  // namespace mcx

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct mcx_join {
  int k = 0, W = 0, ncols = 0, n_isec = 0, device = 0, cus = 0;
  uint32_t flags = 0, grid = 0;
  uint64_t out_chunk = 64ull << 20;
  hipStream_t stream = nullptr;
  struct Call { uint8_t *d_recs; uint64_t *d_loc; uint64_t nrecs, kept; };
  std::vector<Call> dev;
  std::vector<JoinCall> calls;
  std::vector<int32_t> from, into;
  uint32_t max_nmap = 1;
  unsigned long long *d_count = nullptr;
  int32_t *d_from = nullptr;  // scratch of one call's source colours
  size_t d_from_cap = 0;
  void *h_buf = nullptr;  // mcx_join_buffer
  double ms[4] = {0, 0, 0, 0};  // mcx_join_phases
  mcx_join_stats st{};
};

static unsigned join_grid(const mcx_join *j, uint64_t items)
{
  const uint64_t cap = j->grid ? j->grid : (uint64_t)j->cus * 8;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, cap));
}

extern "C" void mcx_join_destroy(mcx_join *j)
{
  if (!j) return;
  (void)hipSetDevice(j->device);
  if (j->stream) (void)hipStreamSynchronize(j->stream);
  for (auto &c : j->dev) { if (c.d_recs) (void)hipFree(c.d_recs); if (c.d_loc) (void)hipFree(c.d_loc); }
  if (j->d_count) (void)hipFree(j->d_count);
  if (j->d_from) (void)hipFree(j->d_from);
  if (j->h_buf) (void)hipHostFree(j->h_buf);
  if (j->stream) (void)hipStreamDestroy(j->stream);
  delete j;
}

extern "C" int mcx_join_create(mcx_join **out, int kmer_size, int out_ncols, int n_isec, uint32_t flags, int device)
{
  if (!out) return fail(MCX_ERR_ARG, "null argument");
  *out = nullptr;
  if (kmer_size < 3 || kmer_size > 127 || !(kmer_size & 1)) return fail(MCX_ERR_ARG, "kmer size must be odd and within 3..127 (got %d)", kmer_size);
  if (out_ncols < 1 || out_ncols > 10000) return fail(MCX_ERR_ARG, "bad number of colours: %d", out_ncols);
  if (n_isec < 0) return fail(MCX_ERR_ARG, "bad number of intersection graphs: %d", n_isec);
  if (flags & ~(uint32_t)MCX_JOIN_KEEP_EMPTY) return fail(MCX_ERR_ARG, "unknown join flags: %u", flags);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return fail(MCX_ERR_NODEVICE, "no HIP device found"); }
  if (device < 0 || device >= ndev) return fail(MCX_ERR_NODEVICE, "no HIP device %d (%d found)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  mcx_join *j = new mcx_join();
  ScopeExit drop([&] { mcx_join_destroy(j); });
  j->k = kmer_size; j->W = words_for_k(kmer_size); j->ncols = out_ncols; j->n_isec = n_isec; j->flags = flags; j->device = device;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  j->cus = std::max(1, prop.multiProcessorCount);
  HIP_TRY(hipStreamCreateWithFlags(&j->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc((void **)&j->d_count, 4 * sizeof(unsigned long long)));
  drop.dismiss();
  *out = j;
  return MCX_OK;
}

extern "C" int mcx_join_configure(mcx_join *j, const char *key, uint64_t value)
{
  if (!j || !key) return fail(MCX_ERR_ARG, "null argument");
  if (!strcmp(key, "grid")) { j->grid = (uint32_t)std::min<uint64_t>(value, 1u << 20); return MCX_OK; }
  if (!strcmp(key, "out_chunk")) { j->out_chunk = value ? value : (64ull << 20); return MCX_OK; }
  return fail(MCX_ERR_ARG, "unknown join configuration key: %s", key);
}

extern "C" int mcx_join_get_stats(const mcx_join *j, mcx_join_stats *stats)
{
  if (!j || !stats) return fail(MCX_ERR_ARG, "null argument");
  *stats = j->st;
  return MCX_OK;
}

extern "C" int mcx_join_phases(const mcx_join *j, double *ms)
{
  if (!j || !ms) return fail(MCX_ERR_ARG, "null argument");
  for (int i = 0; i < 4; i++) ms[i] = j->ms[i];
  return MCX_OK;
}

extern "C" int mcx_join_buffer(mcx_join *j, size_t bytes, void **ptr)
{
  if (!j || !ptr || !bytes) return fail(MCX_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(j->device));
  if (j->h_buf) { (void)hipHostFree(j->h_buf); j->h_buf = nullptr; }
  HIP_TRY(hipHostMalloc(&j->h_buf, bytes, hipHostMallocDefault));
  *ptr = j->h_buf;
  return MCX_OK;
}

// Every call allocates its own two buffers and ends in a stream synchronisation (the count of kept records comes back),
// so a caller that reads a file in chunks has its reads and the uploads take turns: nothing overlaps on the loading side.
extern "C" int mcx_join_add_records(mcx_join *j, int source, const void *recs, uint64_t nrecs, int file_ncols, const int32_t *from_col,
                                    const int32_t *into_col, int nmap)
{
  if (!j) return fail(MCX_ERR_ARG, "null argument");
  if (source < -1 || source >= j->n_isec) return fail(MCX_ERR_ARG, "bad source %d (-1 or an intersection rank below %d)", source, j->n_isec);
  if (file_ncols < 1 || file_ncols > 10000) return fail(MCX_ERR_ARG, "bad number of file colours: %d", file_ncols);
  if (nmap < 1 || !from_col || (source < 0 && !into_col)) return fail(MCX_ERR_ARG, "empty colour filter");
  for (int m = 0; m < nmap; m++) {
    if (from_col[m] < 0 || from_col[m] >= file_ncols) return fail(MCX_ERR_ARG, "filter source colour %d out of range (file has %d)", from_col[m], file_ncols);
    if (source < 0 && (into_col[m] < 0 || into_col[m] >= j->ncols)) return fail(MCX_ERR_ARG, "filter target colour %d out of range (output has %d)", into_col[m], j->ncols);
  }
  if (!nrecs) return MCX_OK;
  if (!recs) return fail(MCX_ERR_ARG, "null records");
  const double t_in = now_s();
  if (nrecs > kJoinIdxMask || j->calls.size() >= (1u << (64 - kJoinIdxBits)) - 1) return fail(MCX_ERR_ARG, "too many records or calls for one join");
  HIP_TRY(hipSetDevice(j->device));
  const uint32_t rec_bytes = 8u * (uint32_t)j->W + 5u * (uint32_t)file_ncols;
  const uint64_t bytes = nrecs * rec_bytes;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bytes + 8 * nrecs + (1u << 20) > free_b)
    return fail(MCX_ERR_NOMEM, "join: the records of the inputs do not fit the free HBM (%llu MB more asked for, %llu MB free); joining in several passes is not implemented",
                (unsigned long long)((bytes + 8 * nrecs) >> 20), (unsigned long long)(free_b >> 20));
  mcx_join::Call c{nullptr, nullptr, nrecs, 0};
  HIP_TRY(hipMalloc((void **)&c.d_recs, bytes + 16));  // (+16: join_load32 reads whole aligned words)
  ScopeExit drop([&] { (void)hipFree(c.d_recs); if (c.d_loc) (void)hipFree(c.d_loc); });
  HIP_TRY(hipMalloc((void **)&c.d_loc, 8 * nrecs));
  if ((size_t)nmap > j->d_from_cap) {
    if (j->d_from) (void)hipFree(j->d_from);
    j->d_from = nullptr; j->d_from_cap = 0;
    HIP_TRY(hipMalloc((void **)&j->d_from, sizeof(int32_t) * (size_t)nmap));
    j->d_from_cap = (size_t)nmap;
  }
  hipStream_t st = j->stream;
  HIP_TRY(hipMemcpyAsync(c.d_recs, recs, bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c.d_recs + bytes, 0, 16, st));
  HIP_TRY(hipMemcpyAsync(j->d_from, from_col, sizeof(int32_t) * (size_t)nmap, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(j->d_count, 0, sizeof(unsigned long long), st));
  const uint64_t tag = (uint64_t)j->calls.size() << kJoinIdxBits;
  hipLaunchKernelGGL(k_join_extract, dim3(join_grid(j, nrecs)), dim3(256), 0, st, (const uint8_t *)c.d_recs, nrecs, rec_bytes, 8u * (uint32_t)j->W,
                     (const int32_t *)j->d_from, (uint32_t)nmap, tag, c.d_loc, j->d_count);
  HIP_TRY(hipGetLastError());
  unsigned long long kept = 0;
  HIP_TRY(hipMemcpyAsync(&kept, j->d_count, sizeof(kept), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  c.kept = kept;
  JoinCall jc{c.d_recs, nrecs, rec_bytes, (uint32_t)file_ncols, source, (uint32_t)nmap, (uint32_t)j->from.size(), 0};
  for (int m = 0; m < nmap; m++) { j->from.push_back(from_col[m]); j->into.push_back(source < 0 ? into_col[m] : 0); }
  if (source < 0) { j->st.recs_read += nrecs; j->st.recs_kept += kept; j->max_nmap = std::max(j->max_nmap, (uint32_t)nmap); }
  else { j->st.isec_recs_read += nrecs; j->st.isec_recs_kept += kept; }
  j->calls.push_back(jc);
  j->dev.push_back(c);
  drop.dismiss();
  j->ms[0] += (now_s() - t_in) * 1e3;
  return MCX_OK;
}

extern "C" int mcx_join_finish(mcx_join *j, mcx_sink_fn sink, void *ctx, mcx_join_stats *stats)
{
  if (!j || !sink) return fail(MCX_ERR_ARG, "null argument");
  HIP_TRY(hipSetDevice(j->device));
  hipStream_t st = j->stream;
  double t_ph = now_s();
  auto phase = [&](int i) { const double t = now_s(); j->ms[i] += (t - t_ph) * 1e3; t_ph = t; };
  j->st.kmers_written = j->st.kmers_intersection = j->st.kmers_written_no_covg = 0;
  uint64_t M = 0;
  for (auto &c : j->dev) M += c.kept;
  if (stats) *stats = j->st;
  if (!M) return MCX_OK;
  const int W = j->W;
  const uint32_t rb = 8u * (uint32_t)W + 5u * (uint32_t)j->ncols, ew = ((uint32_t)j->ncols + 3u) / 4u;
  // the tile of the reduce kernel: what 48 KB of LDS hold, 128 records at the most; one record where a record is wider
  const uint32_t per_rec = rb + 4u * (uint32_t)j->ncols + 4u * ew;
  const uint32_t T = std::max(1u, std::min(128u, (48u << 10) / per_rec));
  const size_t lds = (((size_t)T * rb + 16 + 15) & ~(size_t)15) + (size_t)T * (4u * (size_t)j->ncols + 4u * ew);
  if (lds > (160u << 10) - 1024) return fail(MCX_ERR_ARG, "join: a record of %d colours does not fit the LDS", j->ncols);
  if (lds > (64u << 10)) allow_lds(k_join_reduce, lds);
  const uint64_t chunk = std::max<uint64_t>(j->out_chunk, 1);
  size_t tmp_bytes = 0;
  int rc = sort_perm_scratch(st, M, &tmp_bytes);
  if (rc != MCX_OK) return rc;
  {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // per kept record 32 bytes of sort arrays + 10 of run tables, and rocprim's scratch (it keeps a second copy of keys
    // and values: about 16 more); cmd_join.c's estimate before anything is read books the same per record of the files
    const uint64_t need = 8 * (4 * M + 2) + tmp_bytes + 10 * M + std::min<uint64_t>(chunk, M * rb) + 2 * (uint64_t)rb + (1u << 20);
    if (need > free_b)
      return fail(MCX_ERR_NOMEM, "join: the sort of %llu records needs %llu MB of HBM beside the records, %llu MB are free; joining in several passes is not implemented",
                  (unsigned long long)M, (unsigned long long)(need >> 20), (unsigned long long)(free_b >> 20));
  }
  DevBuf<uint64_t> d_p0, d_p1, d_k0, d_k1, d_outidx;
  DevBuf<uint8_t> d_tmp, d_runw, d_runmask, d_out;
  DevBuf<JoinCall> d_calls;
  DevBuf<int32_t> d_from, d_into;
  HIP_TRY(d_p0.alloc(M + 1));
  HIP_TRY(d_p1.alloc(M + 1));
  HIP_TRY(d_k0.alloc(M));
  HIP_TRY(d_k1.alloc(M));
  HIP_TRY(d_tmp.alloc(tmp_bytes ? tmp_bytes : 16));
  HIP_TRY(d_calls.alloc(j->calls.size()));
  HIP_TRY(d_from.alloc(j->from.size()));
  HIP_TRY(d_into.alloc(j->into.size()));
  HIP_TRY(hipMemcpyAsync(d_calls.p, j->calls.data(), sizeof(JoinCall) * j->calls.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_from.p, j->from.data(), sizeof(int32_t) * j->from.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_into.p, j->into.data(), sizeof(int32_t) * j->into.size(), hipMemcpyHostToDevice, st));
  {
    uint64_t at = 0;
    for (auto &c : j->dev) {
      if (c.kept) HIP_TRY(hipMemcpyAsync(d_p0.p + at, c.d_loc, 8 * c.kept, hipMemcpyDeviceToDevice, st));
      at += c.kept;
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (auto &c : j->dev) { (void)hipFree(c.d_loc); c.d_loc = nullptr; c.kept = 0; }  // (a second finish finds nothing)
  }
  const unsigned gm = join_grid(j, M);
  auto word = [&](int w, bool, const uint64_t *through, uint64_t *dst, const uint64_t **) -> int {
    hipLaunchKernelGGL(k_join_word, dim3(gm), dim3(256), 0, st, through, (const JoinCall *)d_calls.p, (uint32_t)w, dst, M);
    HIP_TRY(hipGetLastError());
    return MCX_OK;
  };
  uint64_t *const keys[2] = {d_k0.p, d_k1.p}, *const perms[2] = {d_p0.p, d_p1.p}, *items = nullptr;
  if ((rc = sort_perm_by_words(st, M, W, 64, keys, perms, d_tmp.p, tmp_bytes, nullptr, word, &items)) != MCX_OK) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  phase(1);
  uint64_t *runstart = items == d_p0.p ? d_p1.p : d_p0.p, *head = d_k0.p, *runid = d_k1.p;
  hipLaunchKernelGGL(k_join_heads, dim3(gm), dim3(256), 0, st, (const uint64_t *)items, (const JoinCall *)d_calls.p, (uint32_t)W, head, M);
  HIP_TRY(hipGetLastError());
  if ((rc = device_scan(st, (const uint64_t *)head, runid, M)) != MCX_OK) return rc;
  hipLaunchKernelGGL(k_join_runs, dim3(gm), dim3(256), 0, st, (const uint64_t *)head, runid, runstart, M);
  HIP_TRY(hipGetLastError());
  uint64_t R = 0;
  HIP_TRY(hipMemcpyAsync(&R, runid + (M - 1), 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  R += 1;
  d_tmp.release();
  HIP_TRY(d_runw.alloc(R));
  HIP_TRY(d_runmask.alloc(R));
  HIP_TRY(d_outidx.alloc(R));
  uint64_t *wflag = d_k0.p;  // (the head flags are spent)
  HIP_TRY(hipMemsetAsync(j->d_count, 0, 4 * sizeof(unsigned long long), st));
  const unsigned gr = join_grid(j, R);
  hipLaunchKernelGGL(k_join_isec, dim3(gr), dim3(256), 0, st, (const uint64_t *)items, (const uint64_t *)runstart, R, (const JoinCall *)d_calls.p,
                     (const int32_t *)d_from.p, 8u * (uint32_t)W, (uint32_t)j->n_isec, (uint32_t)((j->flags & MCX_JOIN_KEEP_EMPTY) != 0), d_runw.p,
                     d_runmask.p, wflag, j->d_count);
  HIP_TRY(hipGetLastError());
  if ((rc = device_scan(st, (const uint64_t *)wflag, d_outidx.p, R)) != MCX_OK) return rc;
  uint64_t last[2] = {0, 0};
  unsigned long long ctr[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&last[0], d_outidx.p + (R - 1), 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&last[1], wflag + (R - 1), 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ctr, j->d_count, sizeof(ctr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t nout = last[0] + last[1];
  uint64_t *outrun = d_k0.p;  // (and so are the write flags: d_runw holds them)
  hipLaunchKernelGGL(k_join_outrun, dim3(gr), dim3(256), 0, st, (const uint8_t *)d_runw.p, (const uint64_t *)d_outidx.p, R, outrun);
  HIP_TRY(hipGetLastError());
  j->st.kmers_written = nout;
  j->st.kmers_intersection = ctr[0];
  j->st.kmers_written_no_covg = ctr[1];
  if (stats) *stats = j->st;
  HIP_TRY(hipStreamSynchronize(st));
  phase(2);
  if (!nout) return MCX_OK;

  const uint64_t total = nout * rb, cbytes = std::min(chunk, total);
  HostBuf<uint8_t> h_out;
  HIP_TRY(d_out.alloc(cbytes + 2 * (uint64_t)rb + 32));
  HIP_TRY(h_out.alloc(cbytes));
  JoinReduce a;
  a.items = items; a.runid = runid; a.runstart = runstart; a.outidx = d_outidx.p; a.outrun = outrun;
  a.runw = d_runw.p; a.runmask = d_runmask.p; a.calls = d_calls.p; a.from = d_from.p; a.into = d_into.p;
  a.W = (uint32_t)W; a.ncols = (uint32_t)j->ncols; a.rec_bytes = rb; a.T = T; a.dst = d_out.p;
  // slices of a call's colour filter that a thread takes: one while the filters are short
  a.P = 1;
  while (a.P < 64 && a.P * 4 < j->max_nmap) a.P *= 2;
  const uint64_t cap_blocks = j->grid ? j->grid : (uint64_t)j->cus * 8;
  for (uint64_t b0 = 0; b0 < total; b0 += cbytes) {
    const uint64_t b1 = std::min(total, b0 + cbytes);
    a.o0 = b0 / rb;
    a.o1 = (b1 + rb - 1) / rb;  // (at most cbytes / rb + 2 records: d_out holds them)
    const uint64_t ntiles = (a.o1 - a.o0 + T - 1) / T;
    hipLaunchKernelGGL(k_join_reduce, dim3((unsigned)std::min(ntiles, cap_blocks)), dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_out.p, d_out.p + (b0 - a.o0 * rb), b1 - b0, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (sink(ctx, h_out.p, (size_t)(b1 - b0)) != 0) return fail(MCX_ERR_SINK, "join: the sink refused the records");
  }
  phase(3);
  return MCX_OK;
}
