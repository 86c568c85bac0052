/*
 * mcx_gpu.h -- C ABI of the MI355X (gfx950) backend for McCortex `build`.
 *
 * The reference has no plugin/FFI layer: `ctx_build` (src/commands/ctx_build.c:245)
 * calls statically linked C functions.  This header is the set of entry points
 * a C host (the reference's own `ctx_build`, or our `mccortex<K> build`) binds
 * instead of those functions; every entry names the reference call it replaces
 * (paths relative to the reference root).  Plain pointers and sizes only.
 *
 * Conventions: every function returns MCX_OK (0) or a negative mcx_status and
 * sets a thread-local message readable with mcx_last_error().  No callbacks
 * into the host except the export sink.  A handle is NOT thread-safe: one
 * submitting host thread per handle (kernels run asynchronously on the
 * handle's HIP stream).  The library never falls back to a CPU path: without
 * a gfx950 device mcx_graph_create() fails with MCX_ERR_NODEVICE.
 */
#ifndef MCX_GPU_H_
#define MCX_GPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MCX_OK = 0,
  MCX_ERR_ARG = -1,       /* bad argument (even k, k out of range, colour >= ncols ...) */
  MCX_ERR_NODEVICE = -2,  /* no usable HIP device */
  MCX_ERR_NOMEM = -3,     /* device/host allocation failed */
  MCX_ERR_FULL = -4,      /* "Hash table is full" (src/graph/hash_table.c:119-123) */
  MCX_ERR_HIP = -5,       /* HIP runtime error, see mcx_last_error() */
  MCX_ERR_SINK = -6,      /* export sink returned non-zero */
  MCX_ERR_INVAL = -7      /* malformed input text (mcx_links_add_text; see mcx_links_error) */
} mcx_status;

/* Subset of SeqLoadingStats (src/basic/seq_loading_stats.h:5-14) that the
 * build path fills (src/tools/build_graph.c:173-188,209-213). */
typedef struct {
  uint64_t num_se_reads;
  uint64_t num_good_reads;      /* reads with >= 1 contig */
  uint64_t num_bad_reads;       /* reads with no contig   */
  uint64_t total_bases_read;
  uint64_t total_bases_loaded;  /* sum of contig lengths  */
  uint64_t contigs_parsed;
  uint64_t num_kmers_loaded;    /* k-mer occurrences inserted */
  uint64_t num_kmers_novel;     /* occurrences that created a new node */
  /* --remove-pcr only (mcx_graph_add_reads_pcr) */
  uint64_t num_pe_reads;        /* reads loaded as mates of a pair */
  uint64_t num_dup_se_reads;    /* single reads dropped as PCR duplicates */
  uint64_t num_dup_pe_pairs;    /* pairs dropped as PCR duplicates */
} mcx_load_stats;

typedef struct mcx_graph mcx_graph;

const char *mcx_last_error(void);
const char *mcx_version(void);
int mcx_device_count(void);
/* Free / total HBM of a device in bytes (the build command checks -m/-n against
 * HBM where the reference checks host RAM, src/graph/cmd_mem.c:133-151). */
int mcx_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* Replaces db_graph_alloc (src/graph/db_graph.c:23) + hash_table_alloc
 * (src/graph/hash_table.c:16-52) for the build path.
 *   kmer_size       odd, 3..127 (W = 1 word for k<=31, 2 words for 33..63, 3 for
 *                   65..95, 4 for 97..127: the reference's MAXK = 31 / 63 / 95 / 127
 *                   builds, src/graph/binary_kmer.h:10-18, Makefile:33-48).  k > 63
 *                   builds on one device with the fused insert kernel (one HBM
 *                   atomic per occurrence); the partitioned insert, the exchange
 *                   formats and mcx_graph_create_multi are for k <= 63.
 *   ncols           colours (>=1); coverage and edges are kept per colour
 *   capacity_kmers  minimum number of k-mer slots (the reference's -n); the
 *                   slot layout, probe sequence and seed are free because
 *                   parity is on the sorted record set
 *   device          HIP device ordinal */
int mcx_graph_create(mcx_graph **g, int kmer_size, int ncols,
                     uint64_t capacity_kmers, int device);
/* One shard of a graph whose table is split over `nparts` GPUs (a power of two, <= 32) by hash
 * prefix: the key's owner is the top bits of the quotient-hash region index (mcx_graph_key_owner).
 * mcx_graph_create == nparts 1.  Every shard must be created with the same k / ncols / capacity. */
int mcx_graph_create_shard(mcx_graph **g, int kmer_size, int ncols, uint64_t capacity_kmers,
                           int device, int nparts, int part);
void mcx_graph_destroy(mcx_graph *g);

/* Empty the table and zero the statistics (graph stays allocated). */
int mcx_graph_reset(mcx_graph *g);

/* Tuning knobs (no reference equivalent).  Keys:
 *   "defer"        1 (default): k-mer occurrences are radix-partitioned by table region into
 *                  HBM bins and applied one sub-table at a time from LDS when the bins fill
 *                  up or the graph is read (sync / nkmers / stats / export); 0: every
 *                  occurrence is inserted straight into the HBM table with device atomics.
 *                  Both give the same graph.
 *   "defer_tuples" occurrences buffered per flush (sizes the bin workspace in HBM); default: 64 per
 *                  table slot within 30 % of the HBM free after the table was allocated.  A graph with
 *                  several colours shares this workspace between its colours (a pool of bin sets, each
 *                  bound to the colour that first writes to it): colours may alternate from call to
 *                  call without a flush, and a flush makes one pass over the table per colour.
 *                  Reads handed over in host memory while the device is idle are flushed in the
 *                  background, one group of table regions at a time (MCX_IDLE_FLUSH=0: off).
 *   "flush_regions" table regions split + applied per step of a flush (0 = automatic: 16 K sub-tables
 *                  per step); bounds the sub-table bin workspace to that share of the table
 *   "place_bins"   1 (default) .. 32: the sub-table bin workspace is the best of up to n allocations -- each half of the
 *                  flush overlap chosen by itself -- by a probe that writes the split kernel's pattern (16 K fronts,
 *                  128-byte runs) into them: where 8 GB of bins happen to lie in HBM decides 13 % of that kernel
 *                  (37.9-38.6 against 43.8-44.3 ms per 12 G occurrences at C2).  Costs n allocations and ~3 ms of probes
 *                  each at the first use of the workspace; candidates are held while HBM has room for them, and the search ends
 *                  as soon as one is 30 % faster than the slowest seen (about one place in five is).
 *   "intersect"    1: `build --intersect` (ctx_build.c:341-363,384-413).  The graph must have been
 *                  created with ONE colour more than the output: the last colour becomes hidden (not
 *                  exported, not scanned) and holds the union of the intersection graphs' edges,
 *                  loaded with mcx_graph_add_records(... into = that colour).  Implies "defer" 0.
 *   "must_exist"   1: mcx_graph_add_reads only updates k-mers that are already in the graph and adds
 *                  an edge only between consecutive k-mers that were both found
 *                  (BuildGraphTask.prefs.must_exist_in_graph, src/tools/build_graph.c:99-150)
 *   "prepare"      allocate now what the first mcx_graph_add_reads otherwise allocates (pinned staging
 *                  buffers, the partition workspace): lets a host that parses with other threads hide
 *                  ~0.1 s behind the parse of its first batch
 *   "profile"      1: time every kernel launch with HIP events (see mcx_graph_profile)
 * Test and experiment knobs (launch geometry only: no allocation depends on them, so they may be set at any
 * time and take effect from the next launch; the answers must not change with them):
 *   "grid"         n >= 1: at most n blocks for the grid-stride launches that otherwise take CUs x 8 (the stream
 *                  k-merisers k_stream / k_stream_bin / k_stream_superk, k_insert_tuples, k_infer_records, the
 *                  table scans, the export compaction) and 4 n for the split, the LDS insert and k_superk_bin
 *                  unless "grid_split" / "grid_insert" are set; 0 restores CUs x 8.  Small grids make every
 *                  block walk several tiles, which the byte-exact tests use to reach the kernels' loops.
 *   "grid_stream"  n >= 1: blocks of k_stream_bin (0: "grid"; MCX_GRID_STREAM at creation)
 *   "grid_split"   n >= 1: blocks of the split k_tuples_bin (0: 4 x "grid", halved / quartered for its 512- /
 *                  1024-thread forms; MCX_GRID_SPLIT)
 *   "grid_insert"  n >= 1: blocks of k_lds_insert (0: 4 x "grid"; MCX_GRID_INSERT) */
int mcx_graph_configure(mcx_graph *g, const char *key, uint64_t value);
/* "kernel calls total_ms" per line for the launches recorded since "profile" was set. */
int mcx_graph_profile(mcx_graph *g, char *buf, size_t buflen);

/* One table over several GPUs of a node, driven by one host process: what the reference's batch
 * loop (src/commands/ctx_build.c:384-407) becomes when the hash table it feeds is split across
 * `ndevices` devices (a power of two <= 32; a device may be named more than once): by the hash of a
 * k-mer's canonical minimizer for odd k in 29..63 (exchange format v3: reads travel as super-k-mer
 * records, every device holds an ordinary table), by hash prefix otherwise (format v2: occurrences
 * travel; MCX_MULTI_EXCHANGE=v2 forces it).  mcx_graph_key_owner tells which device holds a key.
 * SURVEY.md 8(b) sketched this as the devices / ndevices arguments of mcx_graph_create.  The handle
 * that comes back is used like any other: mcx_graph_add_reads (the batch is dealt out to the
 * shards, each k-merises its piece and sends every other shard its occurrences with peer copies
 * over xGMI), mcx_graph_add_reads_pcr, mcx_graph_add_records, sync / statistics / scans / checksum,
 * mcx_graph_export (sorted: one device sort merges the shards).  mcx_graph_add_stream_dev takes a
 * stream on any of the devices.  Intersect / must-exist mode works as on one device (records are
 * dealt with by the shard that owns their key; reads are walked by every shard, which exchange what
 * they found before any of them updates a node: an edge needs both of its k-mers).  Hot k-mers and
 * low-complexity input (poly-G reads, satellite repeats) do not overflow the exchange: what fits neither
 * its segment nor the owner's overflow bin is spilled on the sender and routed by the host.  Format v2's
 * spill area holds a whole piece, so nothing can be lost; format v3 has room for 3 records per 16
 * positions in the segments (random reads make 2.3, low-complexity input fewer: long runs) and its spill
 * area holds one record per start position of a piece -- a record is a run of >= 1 k-mers, so no input
 * can overflow it.  Start-up runs a peer self-test: for every ordered pair of distinct devices one copy
 * kernel writes a pattern into the other device's memory through the peer mapping and the result is read
 * back; a pair that fails switches the group to hipMemcpyPeerAsync copies (what MCX_MULTI_COPY=memcpy
 * selects by hand) with one line on stderr.  Not available on such a handle: the
 * device-pointer exchange calls below (those take a single shard).  ndevices == 1 is mcx_graph_create. */
int mcx_graph_create_multi(mcx_graph **out, int kmer_size, int ncols, uint64_t capacity_kmers,
                           const int *devices, int ndevices);
/* HBM per device that the exchange buffers of such a table take on first use (send / receive sets of
 * one piece, spill areas), for the caller's memory check next to the table itself: the build command
 * adds it when it checks -m / -n against the free HBM (src/graph/cmd_mem.c:133-151).  0 for one device.
 * When the buffers do not fit after all, the library halves the piece instead of failing. */
int mcx_multi_exchange_bytes(int kmer_size, int ndevices, uint64_t capacity_kmers, uint64_t *bytes_per_device);
/* Devices the handle spans (1 for an ordinary graph). */
int mcx_graph_ndevices(const mcx_graph *g);

/* Slots actually allocated (>= capacity_kmers) and bytes of HBM held. */
int mcx_graph_capacity(const mcx_graph *g, uint64_t *slots, uint64_t *bytes);

/* Replaces build_graph_from_reads_mt (src/tools/build_graph.c:192-231, SE path
 * without --remove-pcr) for a whole batch of reads held in host memory:
 * contig split (src/basic/seq_reader.c:61-172), rolling k-mers, canonical key,
 * find-or-insert, coverage +1, edge OR (src/tools/build_graph.c:122-150).
 *   bases          concatenated read bases (ASCII, any case), no separators
 *   quals          NULL, or quality bytes in the same layout.  They decide under a
 *                  cutoff; without one only a byte >= 128 does (a negative `char`
 *                  ends a contig in seq_contig_end2 whatever the cutoff,
 *                  seq_reader.c:148-149): the batch is scanned for one
 *   read_offsets   nreads+1 offsets into bases/quals
 *   fq_cutoff_abs  prefs.fq_cutoff + FASTQ offset, 0 = off (build_graph.c:203-206)
 *   hp_cutoff      homopolymer cutoff, 0 = off
 *   stats_accum    optional; num_se_reads and total_bases_read are added here.
 *                  Contig / k-mer / good-read counters live on the device: read
 *                  them with mcx_graph_device_stats() (the host takes the delta
 *                  around each input file, as graph_info_update_stats needs
 *                  per-file totals, src/tools/build_graph.c:294-298).
 * The call returns once the batch is staged; use mcx_graph_sync() to drain. */
int mcx_graph_add_reads(mcx_graph *g, int colour,
                        const uint8_t *bases, const uint8_t *quals,
                        const uint64_t *read_offsets, uint64_t nreads,
                        uint8_t fq_cutoff_abs, uint8_t hp_cutoff,
                        mcx_load_stats *stats_accum);

/* The same step with prefs.remove_pcr_dups (`build --remove-pcr`): replaces
 * build_graph_from_reads_mt (src/tools/build_graph.c:192-231) + seq_reads_are_novel (:28-92).
 *   paired         != 0: reads 2i and 2i + 1 are the two mates of pair i (a --seq2 / --seqi
 *                  task); 0: single reads (--seq)
 *   matedir        0 FF, 1 FR, 2 RF, 3 RR (cortex_types.h:18-25): mates are turned to FF and
 *                  loaded that way (seq_reader_orient_mp_FF, src/basic/seq_reader.c:506-510);
 *                  a single read is reverse-complemented for RF / RR
 *   fq_cutoff_abs1/2  the cutoff of the first / second mate's file (single reads: the first)
 * A read (pair) is dropped when the first k-mer of (each of) its read(s) is the start, in the same
 * orientation, of a read (pair) loaded before it -- earlier in this batch or in an earlier call.
 * The reference's outcome depends on the order in which its worker threads reach the reads; this
 * gives the outcome of walking the reads in input order on one thread.  The start k-mers of
 * dropped reads stay in the graph, as in the reference.  num_pe_reads / num_se_reads,
 * total_bases_read and the duplicate counts are added to stats_accum; the call returns when the
 * filter has run (it is synchronous).  Costs 8 bytes of HBM per table slot while in use. */
int mcx_graph_add_reads_pcr(mcx_graph *g, int colour,
                            const uint8_t *bases, const uint8_t *quals,
                            const uint64_t *read_offsets, uint64_t nreads,
                            uint8_t fq_cutoff_abs1, uint8_t fq_cutoff_abs2, uint8_t hp_cutoff,
                            int paired, int matedir, mcx_load_stats *stats_accum);
/* Forget all read starts: the reference wipes dBGraph.readstrt whenever the colour being loaded
 * changes (src/commands/ctx_build.c:392-395). */
int mcx_graph_pcr_reset(mcx_graph *g);

/* Device-resident variant of the same step: `d_stream` is a byte stream in HBM
 * in which reads are separated by at least one byte that is not one of
 * ACGTacgt (e.g. '\n'); every maximal ACGT run of length >= k is one contig
 * (what seq_contig_start/end yield with -Q/-H off).  Must be 16-byte aligned.
 * Asynchronous on the handle's stream. */
int mcx_graph_add_stream_dev(mcx_graph *g, int colour,
                             const void *d_stream, uint64_t nbytes);

/* The same stream in packed form: per 16 positions one code word (2 bits per base, A=0 C=1 G=2 T=3,
 * first base on top) and 16 invalid flags (first base = bit 15; set for every position that does
 * not hold one of ACGTacgt, and for positions >= npos of the last word) -- 3 bits per position
 * instead of 8.  This is what mcx_graph_add_reads stages over PCIe (mcx_pack_bases on the host);
 * mcx_pack_stream_dev converts an ASCII stream that is already in HBM (d_code: (npos + 15) / 16
 * u32, d_inv: as many u16; asynchronous on `hip_stream`, a hipStream_t or NULL). */
int mcx_pack_stream_dev(const void *d_stream, uint64_t nbytes, void *d_code, void *d_inv, void *hip_stream);
int mcx_graph_add_packed_dev(mcx_graph *g, int colour, const void *d_code, const void *d_inv, uint64_t npos);

/* Sharded build.  Step 1 on every rank: k-merise a device
 * stream and bin the per-occurrence tuples (canonical key words, edge byte) by
 * owner = (second result word of lookup3(key) * nparts) >> 32 (= mcx_key_owner()).  d_keys holds nparts bins of
 * bin_capacity tuples, W words each; d_edges likewise one byte per tuple;
 * d_counts[nparts] (uint64) receives the fill of every bin (must be zeroed by
 * the caller).  Overflowing a bin sets MCX_ERR_FULL at the next sync. */
int mcx_graph_partition_stream_dev(mcx_graph *g, const void *d_stream, uint64_t nbytes,
                                   int nparts, uint64_t bin_capacity,
                                   void *d_keys, void *d_edges, void *d_counts);
/* Step 2 on the owner, after the exchange: insert n tuples -- for each, coverage[key][colour] += 1 and
 * edges[key][colour] |= edge byte.  The keys are taken as given (W words each, most significant first): nothing is
 * canonicalised -- a key and its reverse complement are two keys -- and the bits above 2k are not checked (they must
 * be zero for a key that a read could yield; the small integers of `hashtest` are stored as they are).  k <= 63 with
 * the deferred path on: split into pieces of one set of region bins each; otherwise one direct-insert launch.  On a
 * shard of a split table the keys of other shards are inserted too (mcx_insert_stats::foreign_inserts counts them). */
int mcx_graph_insert_tuples_dev(mcx_graph *g, int colour, const void *d_keys,
                                const void *d_edges, uint64_t n);
/* Owner of a canonical key in the exchange above (host-side helper for tests). */
uint32_t mcx_key_owner(const uint64_t *key_words, int kmer_size, int nparts);

/* `mccortex<K> hashtest` (src/commands/ctx_exp_hashtest.c:40-69: `bkmer.b[0] = i; hash_table_find_or_insert(...)`):
 * find-or-insert of the n BinaryKmers whose most significant word is i, i in [first, first + n), all other words 0 --
 * generated on the device, no edges, colour 0.  Ends with the table drained (mcx_graph_sync); MCX_ERR_FULL when the
 * table cannot hold them.  The keys go through mcx_graph_insert_tuples_dev as they are: not canonicalised, and where
 * the integers pass the key bits of the top word (k = 33, 65: two bits) they are stored whole, as the reference does. */
int mcx_graph_hashtest(mcx_graph *g, uint64_t first, uint64_t n);
/* The command's -F mode (hash function only, nothing stored): the reference splits [0, n) into `nparts` ranges
 * (one per thread: range i starts at i * (n / nparts), the last one ends at n), XORs binary_kmer_hash(bkmer, 0) =
 * bklk3_hashlittle over each range and ADDS the ranges' results (ctx_exp_hashtest.c:61-66,160-175). */
int mcx_hashtest_func(int device, int kmer_size, uint64_t n, uint32_t nparts, uint64_t *hash_out);

/* Diagnostics (tools/exp_hbm_map.py): the split kernel's write pattern -- nregions x spb fronts `cap_words` apart,
 * 128-byte runs, `iters` x 64 runs per front -- on any device buffer, timed (the second of two runs, ms). */
int mcx_debug_probe(void *d_buf, uint64_t cap_words, uint32_t nregions, uint32_t spb, uint32_t iters, uint32_t jit_mask, float *ms_out);

/* Like mcx_graph_insert_tuples_dev for tuples that sit in `nseg` segments of `seg_cap` slots with
 * the fills in device memory (d_counts[nseg], u64; a fill above seg_cap is read as seg_cap), so the
 * caller needs no host round trip to learn how many arrived: the overflow bins of the sharded
 * exchange are consumed this way.  Keys as given, as above: not canonicalised, bits above 2k not checked.
 * The whole call goes into ONE set of region bins, booked as min(nseg * seg_cap, tuples per set): when the fills
 * exceed that, the tuples that find their (region, replica) segment full take the direct insert into the table
 * (mcx_insert_stats::fallback_inserts) -- the graph is the same, the call slower.
 * Needs the deferred path (k <= 63, a table of at least 64 sub-tables, "defer" not 0): otherwise MCX_ERR_ARG, before
 * anything is allocated.  nseg == 0 or seg_cap == 0: MCX_OK, nothing happens. */
int mcx_graph_insert_tuple_segments_dev(mcx_graph *g, int colour, const void *d_keys, const void *d_edges,
                                        const void *d_counts, uint32_t nseg, uint64_t seg_cap);

/* Sharded build, compact exchange: the sender bins packed occurrences (one 64-bit word per key
 * word) by (owner, region) of the sharded table, so every owner's block is one fixed-size message
 * and the receiver consumes it without re-binning.
 *   mcx_graph_shard_layout      segments per owner, tuples per segment and overflow capacity for
 *                               calls of at most `tuples_per_call` occurrences
 *   mcx_graph_shard_bins_dev    k-merise a stream into d_keys[nparts][segs][seg_cap][W] with fills
 *                               d_counts[nparts][segs] (zeroed by the caller); occurrences beyond a
 *                               segment go to the owner's overflow bin (full keys + edge bytes,
 *                               d_ov_counts[nparts] zeroed by the caller), beyond that: MCX_ERR_FULL
 *   mcx_graph_add_segments_dev  owner side: split received blocks (nseg segments of packed tuples
 *                               of THIS shard, `ntuples` in total) by sub-table; applied at the
 *                               next flush.  Overflow bins go through mcx_graph_insert_tuples_dev.
 *   mcx_graph_key_owner         owner of a canonical key under this graph's geometry */
int mcx_graph_shard_layout(mcx_graph *g, uint64_t tuples_per_call, uint32_t *segs_per_owner,
                           uint64_t *seg_cap, uint64_t *ov_cap);
int mcx_graph_shard_bins_dev(mcx_graph *g, const void *d_stream, uint64_t nbytes, void *d_keys,
                             void *d_counts, uint64_t seg_cap, void *d_ov_keys, void *d_ov_edges,
                             void *d_ov_counts, uint64_t ov_cap);
int mcx_graph_add_segments_dev(mcx_graph *g, int colour, const void *d_keys, const void *d_counts,
                               uint32_t nseg, uint64_t seg_cap, uint64_t ntuples);
uint32_t mcx_graph_key_owner(const mcx_graph *g, const uint64_t *key_words);

/* Bulk load of `.ctx` records: what graph_load() does for `build --graph <in.ctx>`
 * (src/graph/graphs_load.c:86-214, reader src/graph/graph_file_reader.c:347-420).
 * `recs` = nrecs records in the .ctx body layout (W x u64 key, file_ncols x u32 coverage,
 * file_ncols x u8 edges, byte-packed, host memory).  The colour filter is the reference's list of
 * (from, into) pairs (src/basic/file_filter.c): file colour from_col[i] is added to colour
 * into_col[i] of this graph (coverage +=, saturating at 2^32-1 on export; edges |=; targets and
 * sources may repeat).  Records whose loaded colours all have zero coverage are skipped.  MCX_RECORDS_MUST_EXIST: only update k-mers already in the graph
 * (GraphLoadingPrefs.must_exist_in_graph).  The per-record checks of graph_file_read_raw are
 * reported through the stats: index (counted from the first record ever passed with this stats
 * object) of the first record with zero coverage in every file colour / with edges but no coverage
 * in some colour (the reference warns once for each), or -1; an oversized k-mer fails the call
 * with MCX_ERR_ARG (the reference dies).  Synchronous. */
enum { MCX_RECORDS_MUST_EXIST = 1, MCX_RECORDS_MASK_EDGES = 2 };
typedef struct {
  uint64_t nkmers_read, nkmers_loaded, nkmers_novel;
  int64_t first_oversized, first_zero_covg, first_edges_no_covg; /* initialise to -1 */
} mcx_records_stats;
/* MCX_RECORDS_MASK_EDGES (intersect mode): only OR in edges that the hidden colour has for that
 * k-mer (GraphLoadingPrefs.must_exist_in_edges, graphs_load.c:166-167). */
int mcx_graph_add_records(mcx_graph *g, const void *recs, uint64_t nrecs, int file_ncols,
                          const int32_t *from_col, const int32_t *into_col, int nmap, uint32_t flags,
                          mcx_records_stats *stats_accum);

/* End of an intersect build: remove k-mers with no coverage in any visible colour and AND every
 * colour's edges with the intersection graphs' edges (db_graph_remove_no_covg_kmers +
 * db_graph_intersect_edges, src/graph/db_graph.c:630-673).  *removed = k-mers dropped. */
int mcx_graph_intersect_finish(mcx_graph *g, uint64_t *removed);

/* `clean` (src/commands/ctx_clean.c, src/tools/clean_graph.c) in two calls, so that the host can pick
 * the threshold from the "before" histogram in between.  Both flush pending inserts first and refuse
 * (MCX_ERR_ARG) a graph split over devices or in intersect mode, and graphs of 2^31 k-mers or more.
 * mcx_graph_unitig_stats splits the graph into unitigs (db_unitig.c: maximal chains over the union of
 *   the colours' edges, each k-mer in exactly one) on the device and keeps the decomposition for
 *   mcx_graph_clean.  before (NULL: not wanted) = 3 x MCX_CLEAN_NBINS counts: k-mer coverage (summed
 *   over colours, saturating), unitig median coverage, unitig length, each clipped to the last bin.
 *   Scratch: MCX_CLEAN_BYTES_PER_KMER per k-mer + MCX_CLEAN_BYTES_PER_SLOT per table slot + the radix
 *   sort's temporary while the call runs; MCX_ERR_NOMEM when the free HBM cannot hold it.  Kept on the handle
 *   until the next prune (mcx_graph_clean, mcx_graph_pop_bubbles) or the next call that finds it stale: 27 bytes
 *   per k-mer (slot, coverage, unitig id, length, median, union edges, end degrees, and the link bits that
 *   mcx_graph_pop_bubbles finds the unitig ends with) + MCX_CLEAN_BYTES_PER_SLOT per slot.
 * mcx_graph_clean removes every unitig whose median coverage is < covg_threshold or that is a tip
 *   (length < min_keep_tip and indeg(first) + outdeg(last) <= 1); 0 switches that test off.  Kept
 *   k-mers lose, in every colour, the edges to removed (or absent) k-mers; removed k-mers leave the
 *   table.  The decisions are made once, on the graph as mcx_graph_unitig_stats saw it (which runs
 *   first if it has not, or if the k-mer count has changed since).  after = the same three histograms
 *   over the kept unitigs. */
#define MCX_CLEAN_NBINS 1000
#define MCX_CLEAN_BYTES_PER_KMER 64
#define MCX_CLEAN_BYTES_PER_SLOT 4
typedef struct {
  uint64_t num_tips, num_tip_kmers;                            /* UnitigCleanerStats, clean_graph.c */
  uint64_t num_low_covg_unitigs, num_low_covg_unitig_kmers;
  uint64_t num_tip_and_low_unitigs, num_tip_and_low_unitig_kmers;
  uint64_t nkmers_before, nkmers_removed;
} mcx_clean_stats;
int mcx_graph_unitig_stats(mcx_graph *g, uint64_t *before);
int mcx_graph_clean(mcx_graph *g, uint32_t covg_threshold, uint32_t min_keep_tip, mcx_clean_stats *stats, uint64_t *after);

/* `popbubbles` (src/commands/ctx_pop_bubbles.c; pop_bubbles, mark_remove_bubbles, get_parallel_nodes and
 * process_bubble of src/tools/pop_bubbles.c; prune_nodes_lacking_flag of src/graph/prune_nodes.c) on the
 * decomposition of mcx_graph_unitig_stats, which is reused when it still describes the table and made
 * otherwise.  All colours count as one: edges are their union, coverage is db_node_sum_covg.  Two unitigs are
 * parallel when, one node out and one node back over every other edge, a start of one is found at each end of
 * the other; of such a pair the branch with the lower mean coverage (sum / length, rounded down) loses, on
 * equal means the alternative.  The loser goes if its mean is <= max_covg and its length <= max_klen (each
 * ignored when <= 0) and the lengths differ by <= max_kdiff (ignored when < 0).  Kept k-mers lose, in every
 * colour, the edges to removed k-mers; removed k-mers leave the table.
 * The reference's result depends on the order in which its threads reach the unitigs (a losing alternative is
 * marked visited and never takes its own turn).  Here the result is that of pop_bubbles() on one thread when
 * every unitig is taken in its normal form (db_unitig_normalise: the end with the lower key first, a single
 * k-mer forward) and the unitigs take their turn in ascending order of E(U), the smaller of the keys of U's two
 * end k-mers: a function of the graph alone, not of the table's size or load or the "grid" knob.
 * The same refusals as `clean` (MCX_ERR_ARG).  One more: when a unitig has siblings at both ends and one of its
 * left siblings lies inside a unitig -- only one-sided edges allow that -- the call is refused (MCX_ERR_ARG; the
 * table is left as it was), because the reference would walk a fragment of that unitig as the branch.  This is
 * decided at the sibling, before it is known whether the fragment would end at a right sibling, so it also
 * refuses graphs on which the sequential rule finds no bubble there.  `inferedges` makes the edges two-sided.
 * Scratch beside the decomposition: MCX_POP_BYTES_PER_KMER per k-mer and MCX_POP_BYTES_PER_PAIR per parallel
 * pair found (at most MCX_POP_BYTES_PER_UNITIG per unitig, far fewer in practice).  The pairs are counted by a
 * first pass and the list has exactly that size; MCX_ERR_NOMEM when the free HBM cannot hold it. */
#define MCX_POP_BYTES_PER_KMER 20
#define MCX_POP_BYTES_PER_PAIR 8
#define MCX_POP_BYTES_PER_UNITIG (16 * MCX_POP_BYTES_PER_PAIR)
typedef struct {
  uint64_t num_popped;        /* bubbles popped */
  uint64_t num_pairs;         /* parallel pairs examined */
  uint64_t nkmers_before;
  uint64_t nkmers_removed;
  uint64_t num_unitigs_removed;
  uint32_t rounds;            /* rounds of the order resolution */
} mcx_pop_stats;
int mcx_graph_pop_bubbles(mcx_graph *g, int32_t max_covg, int32_t max_klen, int32_t max_kdiff, mcx_pop_stats *stats);

/* `subgraph` (src/commands/ctx_subgraph.c; subgraph_from_reads, mark_bkmer, mark_unitig, store_node_neighbours and
 * extend of src/tools/subgraph.c; prune_nodes_lacking_flag of src/graph/prune_nodes.c): keep the k-mers within
 * `dist` edges of the seed k-mers.  All colours count as one: the neighbours of a k-mer come from the union of the
 * colours' edges, on both sides.  The result is a set -- a function of the graph, the seeds, dist and the flags
 * alone, not of the table's size or load, the "grid" knob or the "subgraph_narrow" knob.
 *   mcx_graph_subgraph_begin    flushes pending inserts and sets up the state on the handle: dense k-mer ids (the
 *       decomposition of mcx_graph_unitig_stats when it still describes the table -- it is taken over and goes with
 *       the state; otherwise a scan of the table), a mark bit per k-mer and one queue of as many 32-bit ids as there
 *       are k-mers.  A k-mer enters the queue once, when its bit is set, so the queue cannot overflow: the
 *       reference's "Please increase <mem> size" has no counterpart.  With MCX_SUBGRAPH_UNITIGS the decomposition
 *       is made if it is not there.  The same refusals as `clean` (MCX_ERR_ARG): a graph split over devices or in
 *       intersect mode, 2^31 k-mers or more.  Scratch: MCX_SUBGRAPH_BYTES_PER_KMER per k-mer, and where the ids
 *       come from a scan MCX_SUBGRAPH_IDS_BYTES_PER_KMER per k-mer + MCX_CLEAN_BYTES_PER_SLOT per table slot;
 *       MCX_ERR_NOMEM when the free HBM cannot hold it.  A second begin, mcx_graph_reset and mcx_graph_destroy
 *       free the state.  The graph must not be modified between begin and finish: no inserts, and no
 *       mcx_graph_clean or mcx_graph_pop_bubbles, which change edges the ids were made from without changing the k-mer
 *       count that finish checks.
 *   mcx_graph_subgraph_seed_reads / _seed_stream_dev    (READ_TO_BKMERS with no quality or homopolymer cutoff,
 *       mark_bkmer / mark_unitig) may be called any number of times: every k-mer of the seeds that is in the graph
 *       is marked; with MCX_SUBGRAPH_UNITIGS, its whole unitig (db_unitig_fetch).  Lower case counts as upper case,
 *       any other byte ends a contig.  seed_reads takes the layout of mcx_graph_add_reads (read r is
 *       bases[off[r] .. off[r + 1])) and goes through the pinned staging buffers as ASCII, in chunks bounded by what a
 *       buffer holds (a read longer than a chunk goes in pieces); seed_stream_dev takes the layout
 *       of mcx_graph_add_stream_dev (ASCII in HBM, 16-byte aligned, any non-base byte separates reads).
 *   mcx_graph_subgraph_finish   extends the marked set by `dist` breadth-first levels (extend), complements it with
 *       MCX_SUBGRAPH_INVERT, then prunes: unmarked k-mers leave the table, kept k-mers lose in every colour the
 *       edges to removed k-mers -- and to k-mers that are not in the graph, which the extension passes over too
 *       (the reference asserts).  Frees the state.  MCX_SUBGRAPH_UNITIGS must be given as it was to begin.
 * A seed call or a finish without a begin returns MCX_ERR_ARG.
 * The levels run on the device: a frontier of up to "subgraph_narrow" k-mers (mcx_graph_configure; maximum
 * 256, default 0 = never, until the kernel has been timed against chained launches) is expanded by one workgroup that runs level after level in one launch; a larger one by
 * one launch per level, 8 levels chained between two reads of the frontier size. */
enum { MCX_SUBGRAPH_UNITIGS = 1, MCX_SUBGRAPH_INVERT = 2 };
#define MCX_SUBGRAPH_BYTES_PER_KMER 6      /* queue 4, unitig flag 1, mark bit */
#define MCX_SUBGRAPH_IDS_BYTES_PER_KMER 13 /* slot 8, summed coverage 4, union edges 1 */
typedef struct {
  uint64_t num_seed_kmers;   /* k-mer occurrences in the seeds (stats.num_kmers_loaded), in the graph or not */
  uint64_t num_seed_found;   /* distinct k-mers marked before the extension (after the unitig grab) */
  uint64_t nkmers_before, nkmers_kept, nkmers_removed;
  uint32_t levels;           /* breadth-first levels that added k-mers */
  uint32_t narrow_launches;  /* launches of the one-workgroup kernel */
  uint64_t max_frontier;     /* largest frontier, the seeds' included */
} mcx_subgraph_stats;
int mcx_graph_subgraph_begin(mcx_graph *g, uint32_t flags);
int mcx_graph_subgraph_seed_reads(mcx_graph *g, const uint8_t *bases, const uint64_t *read_offsets, uint64_t nreads);
int mcx_graph_subgraph_seed_stream_dev(mcx_graph *g, const void *d_stream, uint64_t nbytes);
int mcx_graph_subgraph_finish(mcx_graph *g, uint32_t dist, uint32_t flags, mcx_subgraph_stats *stats);

/* `reads` (src/commands/ctx_reads.c; read_touches_graph, with READ_TO_BKMERS and no quality or homopolymer cutoff):
 * which reads share a k-mer with the graph.  A read touches the graph iff some k-mer of it is a key of the table;
 * its k-mers are those of every maximal run of ACGTacgt that is at least k long, lower case counts as upper case and
 * any other byte ends a run; the lookup is by canonical key and colours do not matter.  The answer is a function of
 * the table's key set and the reads alone, not of the table's size or load, the chunking or the "grid" knob.  The
 * reference stops at a read's first hit; here every k-mer is looked up (one pass marks a bit per stream position, a
 * second ORs the bits of each read), so the two k-mer counts are exact.  The table is only read.
 *   mcx_graph_reads_touch   takes the layout of mcx_graph_add_reads (read r is bases[off[r] .. off[r + 1])) and writes
 *       hit[r] = 1 or 0.  Flushes pending inserts first.  Synchronous: hit is valid on return.  The reads go through
 *       the pinned staging buffers as ASCII, in chunks bounded by what a buffer holds ("reads_chunk" of
 *       mcx_graph_configure lowers the bound: a test knob); a read longer than a chunk goes in pieces that overlap by
 *       k - 1 bases and its byte is the OR of its pieces'.  stats_accum, if given, is added to.  nreads == 0 is MCX_OK.
 *   mcx_graph_reads_touch_stream_dev   the same over a stream in HBM: ASCII, 16-byte aligned, read i at positions
 *       [d_stream_off[i], d_stream_off[i + 1] - 1) with one separator byte (any non-base byte) behind it, so
 *       d_stream_off holds nreads + 1 64-bit offsets and d_stream_off[nreads] <= nbytes; d_hit takes nreads bytes.
 *       Asynchronous on the handle's stream; the masks (1 bit per stream position) are kept on the handle.
 * Refusals (MCX_ERR_ARG): a graph split over devices, a handle in intersect mode. */
typedef struct {
  uint64_t num_reads, num_reads_hit;
  uint64_t num_kmers;        /* k-mer occurrences in the reads, in the graph or not */
  uint64_t num_kmers_found;  /* occurrences whose k-mer is in the graph */
} mcx_touch_stats;
int mcx_graph_reads_touch(mcx_graph *g, const uint8_t *bases, const uint64_t *read_offsets, uint64_t nreads,
                          uint8_t *hit /* nreads bytes, 0/1 */, mcx_touch_stats *stats_accum /* optional, += */);
int mcx_graph_reads_touch_stream_dev(mcx_graph *g, const void *d_stream, uint64_t nbytes,
                                     const void *d_stream_off /* nreads+1 u64 */, uint64_t nreads, void *d_hit);

/* `coverage` (src/commands/ctx_coverage.c; print_read_covg): what the table stores for the k-mers of reads.  The k-mers
 * of a read are those of `reads` above (maximal runs of ACGTacgt of at least k bases, looked up by canonical key).  For
 * a k-mer that is a key, colour c gives its coverage (clamped to 2^32 - 1, as the export clamps it) and its edge byte
 * turned to the read's strand as fetch_node_edges turns it: where the read holds the reverse complement of the key the
 * two nibbles change places and the bits inside a nibble stay.  Every other start position -- an absent k-mer, a window
 * over an N or a separator, the last k - 1 positions of a read -- gives 0.  The answer is a function of the table's
 * contents and the reads alone, not of the table's size or load, the chunking or the "grid" knob.  The table is only
 * read.
 *   mcx_graph_coverage   takes the layout of mcx_graph_add_reads.  covg is [ncols][nbases] and edges, if not NULL, the
 *       same shape, with nbases = read_offsets[nreads]: index p of a colour holds the k-mer that starts at bases[p] (the
 *       stream's separators do not appear).  Flushes pending inserts first.  Synchronous.  The reads go through the
 *       pinned staging buffers as ASCII in chunks ("reads_chunk" of mcx_graph_configure lowers their size, as for
 *       mcx_graph_reads_touch: a test knob); a read longer than a chunk is probed in pieces that overlap by k - 1
 *       bases, so every k-mer starts in exactly one piece.  The batch's arrays are held in HBM until they are copied
 *       out: 4 (+ 1 with edges) bytes per colour and base; MCX_ERR_NOMEM when that does not fit.  stats, if given, is
 *       added to.  nreads == 0 is MCX_OK.
 *   mcx_graph_coverage_stream_dev   the same over a stream in HBM with the layout of mcx_graph_add_stream_dev (ASCII,
 *       16-byte aligned, any non-base byte separates reads).  d_covg is [ncols][pitch] 32-bit words and d_edges, if not
 *       NULL, [ncols][pitch] bytes, both 16-byte aligned and indexed by stream position; pitch is a multiple of 64 and
 *       at least nbytes.  Positions [0, nbytes) of every colour are written, zeros included (and some of the padding
 *       behind them), so nothing needs clearing between calls.  Asynchronous on the handle's stream; counts nothing.
 *   mcx_graph_coverage_text   the value lines of the command, written on the device after all pieces of the batch have
 *       been probed (a line is never cut by a chunk seam).  For every read in input order and every colour in ascending
 *       order: the edges line with MCX_COVERAGE_EDGES (two lower-case hex characters per k-mer, edges_to_char, separated
 *       by one space), the degree line with MCX_COVERAGE_DEGREES (one of "./[\-{]}X" per k-mer, by min(indegree, 2) and
 *       min(outdegree, 2)), then the coverage line ("%2u" of the first value, " %2u" of every further one).  A line has
 *       klen = max(len - k + 1, 0) values and ends in '\n'; klen = 0 gives a bare '\n'.  The text reaches `sink` in
 *       consecutive byte ranges, like mcx_graph_export's records; line_off, if not NULL, receives
 *       nreads * ncols * lines-per-colour + 1 offsets into it.  HBM: 5 * ncols bytes per base of the batch plus the
 *       text, which is sized by a scan of the line lengths; MCX_ERR_NOMEM when that does not fit.
 * Refusals (MCX_ERR_ARG): a graph split over devices, a handle in intersect mode, unknown flags, edge or degree lines
 * asked of a call that gathered no edges. */
/* the sink of the calls that hand out bytes in consecutive ranges (this one, mcx_graph_export, mcx_graph_unitigs); != 0 stops the call */
typedef int (*mcx_sink_fn)(void *ctx, const void *records, size_t nbytes);
typedef struct { uint64_t num_reads, num_kmers, num_kmers_found; } mcx_coverage_stats;
enum { MCX_COVERAGE_EDGES = 1, MCX_COVERAGE_DEGREES = 2 };
int mcx_graph_coverage(mcx_graph *g, const uint8_t *bases, const uint64_t *read_offsets, uint64_t nreads,
                       uint32_t *covg /* [ncols][nbases] */, uint8_t *edges /* same shape, or NULL */,
                       mcx_coverage_stats *stats_accum /* optional, += */);
int mcx_graph_coverage_stream_dev(mcx_graph *g, const void *d_stream, uint64_t nbytes, void *d_covg /* [ncols][pitch] u32 */,
                                  void *d_edges /* [ncols][pitch] u8, or NULL */, uint64_t pitch);
int mcx_graph_coverage_text(mcx_graph *g, const uint8_t *bases, const uint64_t *read_offsets, uint64_t nreads, uint32_t flags,
                            mcx_sink_fn sink, void *ctx, uint64_t *line_off, mcx_coverage_stats *stats_accum /* optional, += */);

/* `correct` (src/commands/ctx_correct.c; correct_aln_read, handle_read2) without link files: reads corrected against the
 * graph.  The k-mers of a read are those of `reads` above.  Graph view (ctx_correct.c:116-121, 187): every key of the
 * table is walked, a k-mer's edges are the OR of its edge bytes over all colours, and a k-mer is in the sample iff its
 * value word in `colour` is non-zero (coverage or edges, the presence rule of `inferedges` below).
 *   Alignment (db_alignment_from_read): a k-mer aligns iff it is a key and in the sample.  Aligned k-mers at consecutive
 *       positions stay in one segment while the union edges of the earlier hold the edge to the later; a missing edge
 *       ends the contig with no traversal (db_alignment_next_gap, correct_alignment_nxt:390).
 *   Walker step (graph_walker_choose:385-433 with no paths held): the successors over the union edges in nucleotide order;
 *       none: stop; one: take it, POPFWD if it is not in the sample; several: those in the sample, exactly one: take it,
 *       otherwise stop.  The reference asserts that an edge never names an absent k-mer; here such an edge counts as no
 *       edge.  A walk enters an oriented node twice at the most, the third entry stops it (repeat_walker.h:18-50 with
 *       graph_walker_hash64 of (node, orient) alone); every walk starts clean: the visited bits the reference leaves
 *       behind after a POPFWD stop and the false positives of its 22-bit Bloom filter are not reproduced.
 *   Gaps (correct_alignment_nxt:402-438): gap_est = the distance of the two positions, wiggle = (long)(gap_est *
 *       gap_variance + gap_wiggle) in float arithmetic, gap_min = max(0, est - wiggle), gap_max = est + wiggle.  One way
 *       (traverse_one_way2): forward from the node before the gap for gap_max + 1 nodes at the most, stopping on a POPFWD
 *       step, done on reaching the node behind the gap with gap_len >= gap_min; on failure the same from the reverse of
 *       the node behind the gap.  MCX_CORRECT_TWO_WAY (traverse_two_way2:208-236): two walkers step in turn.  A failed
 *       gap ends the contig.
 *   Ends (correct_aln_read:570-639): the left end is extended by at most the first position, the right end by at most
 *       len - (last position + k) steps; POPFWD steps are accepted.  Reads that align perfectly and reads with no aligned
 *       k-mer skip gaps and ends.
 *   Record (handle_read2): uncorrectable stretches in lower case, aligned k-mers and filled bases in upper case (the
 *       nprint rule of correct_reads.c:170-194 says how many filled bases a gap prints), then, if quals is not NULL, as
 *       many quality bytes: the read's own for its bases, fq_zero (0: '.') for filled ones.  Record r is bytes
 *       [out_off[r], out_off[r + 1]) of what reaches `sink` in consecutive ranges, in input order.
 * mcx_graph_correct takes the layout of mcx_graph_add_reads; quals, if given, has a byte per base.  Flushes pending
 * inserts first.  Synchronous.  The reads go through the pinned staging buffers in the chunks of mcx_graph_coverage
 * ("reads_chunk"), and a read in pieces is whole on the device before its walks are made.  Every gap walk and every end
 * extension is an independent task of four lanes.  HBM: 9 (+ 1 with qualities) bytes per base of the batch, 9 bytes per
 * path entry of the tasks (gap_max + 2 per gap, the limit per end) and the records; MCX_ERR_NOMEM when that does not
 * fit.  The result is a function of the table's contents, the reads and the parameters alone, not of the table's size
 * or load, the chunking or the "grid" knob.  The table is only read.  nreads == 0 is MCX_OK.
 * mcx_graph_correct_stream_dev runs the probe, the tasks and the walks over a stream in HBM with the layout of
 * mcx_graph_reads_touch_stream_dev (for the benchmark tool): d_node is scratch of `pitch` 64-bit words, 16-byte aligned,
 * pitch a multiple of 64 and at least nbytes; d_len receives the nreads record lengths.  It hands out no records and
 * returns when the walks are done (their scratch is sized by two totals read back from the device).
 * Stats: gaps = gaps_filled + gaps_too_short + gaps_too_long_or_stopped, each gap by the walk that decided it (too
 * short: gap_len < gap_min).  stops_* count over the walks of every kind what made a walker's last step fail: several
 * successors and not exactly one in the sample, a POPFWD step inside a gap, a third entry.  missing_edges counts, as
 * the reference does, only the first of a perfectly aligned read.  bases_filled = bytes written with fq_zero quality.
 * Refusals (MCX_ERR_ARG): a graph split over devices, a handle in intersect mode, colour >= ncols, unknown flags, a
 * negative or non-finite gap_variance / gap_wiggle. */
enum { MCX_CORRECT_TWO_WAY = 1 };
typedef struct { uint32_t colour, flags; float gap_variance /* D, 0.1 */, gap_wiggle /* d, 5 */; char fq_zero; } mcx_correct_params;
typedef struct {
  uint64_t num_reads, num_kmers, num_kmers_found, num_perfect, num_no_kmers;
  uint64_t gaps, gaps_filled, gaps_filled_backward, gaps_too_short, gaps_too_long_or_stopped;
  uint64_t stops_fork, stops_colour, stops_repeat, missing_edges;
  uint64_t end_gaps, end_gaps_extended, bases_filled;
} mcx_correct_stats;
int mcx_graph_correct(mcx_graph *g, const uint8_t *bases, const uint8_t *quals /* or NULL */, const uint64_t *read_offsets,
                      uint64_t nreads, const mcx_correct_params *p, mcx_sink_fn sink, void *ctx,
                      uint64_t *out_off /* nreads + 1, or NULL */, mcx_correct_stats *stats_accum /* optional, += */);
int mcx_graph_correct_stream_dev(mcx_graph *g, const void *d_stream, uint64_t nbytes, const void *d_stream_off /* nreads+1 u64 */,
                                 uint64_t nreads, const mcx_correct_params *p, void *d_node /* pitch u64 */, uint64_t pitch,
                                 void *d_len /* nreads u64 */, mcx_correct_stats *stats_accum /* optional, += */);
/* walker steps (one per lookup round of a walker) of the last of the two calls on this handle: what the benchmark tool
 * divides by k_cr_walk's time */
uint64_t mcx_graph_correct_walk_steps(const mcx_graph *g);

/* `thread` (src/commands/ctx_thread.c without -p and -u; src/tools/generate_paths.c): reads are laid over a graph of ONE
 * colour and the links of their contigs are generated, counted and kept on the handle.  The walkers hold no paths, so
 * the links are a function of the graph and the reads alone.  A k-mer is in the sample iff its value word is non-zero;
 * an edge that names an absent k-mer counts as no edge, so a degree counts the edges whose k-mer is a key.
 *   Contigs (correct_alignment_nxt:361-510): alignment, segments, gaps and their bounds are those of mcx_graph_correct.
 *       A contig is a run of segments joined by filled gaps with the walked nodes in between; a missing edge ends it
 *       without a walk, a failed gap ends it and the next starts behind the gap.  There are no end extensions.  A
 *       perfectly aligned read is a contig like any other.  Every contig adds nodes + k - 1 to the contig histogram.
 *   Junctions (worker_contig_to_junctions): forward at i if i + 1 < N and outdegree(n[i]) > 1, its base the last of
 *       n[i + 1]; reverse at i if i > 0 and indegree(n[i]) > 1, its base the first of n[i - 1].  A contig without a
 *       junction of each kind adds nothing.
 *   Links (_juncs_to_paths): per reverse junction at i, if a forward junction lies at i or behind it, a link on n[i - 1]
 *       with the bases of the forward junctions from i - 1 on; per forward junction at i, if a reverse junction lies at i
 *       or before it, a link on reverse(n[i + 1]) with the complements of the reverse bases from i + 1 downwards.  A link
 *       is cut to its first max_juncs bases (0: 32767, GPATH_MAX_JUNCS); every generated link counts once, a count stays
 *       at 255.  Links are equal iff k-mer, orientation, length and bases are.
 * mcx_graph_thread takes the layout of mcx_graph_add_reads, flushes pending inserts first and is synchronous; the reads
 * go through the "reads_chunk" pieces of mcx_graph_correct.  MCX_ERR_NOMEM when a batch does not fit.  The links kept
 * depend on the table's contents, the reads and the parameters alone, not on the table's size, the chunking, the "grid"
 * knob or how the reads are split over calls.  nreads == 0 is MCX_OK.  Stats: `aln` as mcx_graph_correct counts it
 * without the end extensions (end_gaps, end_gaps_extended and bases_filled stay 0, stops_* count the gap walks);
 * contig_kmers = nodes of all contigs; juncs_* = junctions of all contigs; links_added = links generated, equal ones
 * counted every time.
 * mcx_graph_links_text writes the .ctp body (gpath_save_sbuf) to `sink` in consecutive ranges: per k-mer `<kmer>
 * <nlinks>`, then its links in gpath_cmp order (F before R, bases in ACGT order, a prefix before the longer link) as
 * `<F|R> <njuncs> <nseen> <juncs>` and, with MCX_LINKS_SEQ, ` seq=<bases> juncpos=<i,j,..>` from a walk of gpath_fetch
 * over the table as it is now.  THE K-MERS COME IN KEY ORDER (the reference writes them in hash-table order).
 * mcx_graph_links_info: the three totals of the header (path_bytes = sum of (njuncs + 3) / 4).
 * mcx_graph_links_contig_hist: *n = the distinct contig lengths, the first `cap` of them (ascending) with their counts.
 * mcx_graph_links_reset forgets links and histogram; mcx_graph_reset does the same.
 * Refusals (MCX_ERR_ARG): ncols != 1, a graph split over devices, a handle in intersect mode, unknown flags, a negative
 * or non-finite gap_variance / gap_wiggle, max_juncs > 32767. */
enum { MCX_THREAD_TWO_WAY = 1 };
typedef struct { uint32_t flags; float gap_variance /* D, 0.1 */, gap_wiggle /* d, 5 */; uint32_t max_juncs /* 0: 32767 */; } mcx_thread_params;
typedef struct {
  mcx_correct_stats aln; /* the fields that apply; the end_* fields and bases_filled stay 0 */
  uint64_t contigs, contig_kmers, juncs_fw, juncs_rv, links_added;
} mcx_thread_stats;
int mcx_graph_thread(mcx_graph *g, const uint8_t *bases, const uint64_t *read_offsets, uint64_t nreads, const mcx_thread_params *p,
                     mcx_thread_stats *stats_accum /* optional, += */);
typedef struct { uint64_t num_kmers_with_paths, num_paths, path_bytes; } mcx_links_info;
int mcx_graph_links_info(mcx_graph *g, mcx_links_info *out);
int mcx_graph_links_contig_hist(mcx_graph *g, uint64_t *lengths, uint64_t *counts, uint64_t cap, uint64_t *n);
enum { MCX_LINKS_SEQ = 1 }; /* add seq= and juncpos= */
int mcx_graph_links_text(mcx_graph *g, uint32_t flags, mcx_sink_fn sink, void *ctx);
int mcx_graph_links_reset(mcx_graph *g);

/* mcx_graph_links_load_text puts the links of a .ctp onto the handle: `text` is whole k-mer blocks of a version-4,
 * one-colour .ctp body (what mcx_links_add_text takes, cut by ctp_pieces_*).  The links join the handle's store, merged
 * with what is there by the sort and reduce of `thread`: equal links add their counts, a count stays at 255.  A k-mer
 * line is looked up by its canonical key (a line that holds the reverse complement turns its links round).  The
 * reference dies on a k-mer that is not in the table (GPATH_DIE_MISSING_KMERS); here *nmissing counts them, none of the
 * piece's links are stored and the call is MCX_ERR_INVAL.  A malformed line is MCX_ERR_INVAL too; seq= and juncpos= are
 * optional and ignored.  *nlinks = the link lines stored.  For a handle whose links came from mcx_graph_thread,
 * links_text, links_reset, links_load_text of those bytes gives the same links_text and the same links_info.
 * Refusals: those of mcx_graph_thread without the one on ncols (the links are then those of the colour assembled). */
int mcx_graph_links_load_text(mcx_graph *g, const void *text, uint64_t nbytes, uint64_t *nlinks /* or NULL */, uint64_t *nmissing /* or NULL */);

/* `contigs` (src/commands/ctx_contigs.c, src/tools/assemble_contigs.c, src/graph/graph_walker.c): every seed k-mer is
 * walked both ways by a walker that uses the links on the handle.  The graph view is that of mcx_graph_correct: union
 * edges, in the sample iff the value word of `colour` is non-zero, an edge that names an absent k-mer counts as no edge.
 *   Walker state: the oriented node; the held links, oldest first, as (link, pos, age); the counter links likewise; the
 *       segments, newest first, as (in_fork, out_fork, num_nodes) (_gw_gseg_init, _gw_gseg_update, graph_walker.c:97-147:
 *       a step at a fork, or onto a node with another previous node in the sample, opens a segment, every link ages by
 *       one, the segments older than the oldest link go; the step adds a node to the newest).
 *   Start (graph_walker_start): one segment of one node, then the pick-up at the start node.
 *   Pick up (pickup_paths:151-210): only at a node in the sample; every stored link of the node with its orientation, in
 *       store order (gpath_cmp), with pos 0 and age 0.  Counter pick-up at a previous node whose out-degree in the sample
 *       is above 1: only links whose first base is that of the step, with pos 1, and only if they are longer than 1.
 *   Choose (graph_walker_choose:371-515): successors over the union edges in ACGT order.  None: NOCOVG.  One: COLFWD, or
 *       POPFWD when it is not in the sample.  Several: those in the sample; one: POPFRK_COLFWD; none: NOCOLCOVG.  Several
 *       in the sample: no held link, or the oldest has age 0: NOLINKS; the first held link that names another base than
 *       the oldest has the oldest's age: SPLIT_LINKS; choice_age = that link's age (0 if all agree), choice_seg = the
 *       first segment from choice_age on with in_fork, path_gap = the nodes of the segments up to it (:474-496); with the
 *       missing-information check, fewer bases named by held and counter links than successors: MISSING_LINKS; else
 *       USELINKS towards the oldest link's base.  Where a held or counter link names a base that is no successor in the
 *       sample the reference aborts (_corrupt_paths), and where no segment up to the oldest link's has in_fork it would
 *       read past its list: HERE THE WALK STOPS WITH StopUnknown and stats.corrupt_links counts it.
 *   Step (_graph_walker_force_jump:525-629): at a fork (POPFRK_COLFWD, USELINKS) held links that name the base taken
 *       advance and go when they end, the others go; counter links advance while pos + 1 < len, else go; fork_count += 1.
 *       If the new node is in the sample, its previous nodes over the union edges other than the one come from, in the
 *       sample (db_graph_prev_nodes_with_mask), are the counter pick-ups (only with the check on); rv_fork iff there is
 *       one.  Then the segment update, then the pick-up at the new node.
 *   Assembly (_assemble_contig without a seed link): the buffer is the seed key forward; for dir 0, 1 (the buffer turned
 *       round for dir 1) a clean walker starts at the buffer's last node; per step the node is appended and
 *       wlk_steps[status] counted; on USELINKS gap_length = path_gap + k + 1, confid = conf[gap_length] (0.0 beyond the
 *       table), max_step_gap and gap_conf[dir] *= confid are updated in that order, then StopLowStepConfidence if confid <
 *       min_step_confid, StopLowCumulativeConfidence if gap_conf < min_cumul_confid; then the repeat rule.  Per dir
 *       paths_held, paths_cntr and the stop cause (graphstep2assem); num_junc = the forks of both directions.
 *   Repeat rule (repeat_walker.h:18-50): the first entry of an oriented node by a step passes (the start node is no
 *       entry); a later one passes iff no earlier non-first entry of that node in this direction had an equal state, else
 *       StopHitLoop and the node stays.  States are compared by a 64-bit hash of both lists: h = mix(count), then per link
 *       mix(h ^ id), mix(h ^ (pos | len << 32)), mix(h ^ age), held then counter, mix = the finaliser of splitmix64, id =
 *       the link's index in the store.  The reference's Bloom false positives are not reproduced.
 *   Seeding: seeds in order -- without seed reads every key in the sample in ascending key order; with them (layout of
 *       mcx_graph_add_reads) the reads in input order, each k bases of ACGT (else MCX_ERR_INVAL); a read that is no key
 *       adds to seeds_not_found, one not in the sample is skipped.  MCX_CONTIGS_RESEED: every seed gives a contig.
 *       Default: seed i gives a contig iff its k-mer is not among the nodes of a contig kept from a seed before it, else
 *       num_reseed_abort += 1.  Only the first `ncontigs` kept contigs exist (0: no limit); later seeds add to nothing.
 *       THE CONTIGS COME IN THAT ORDER (the reference walks its hash table with racing threads).
 * Records go to rec_sink in contig order (whole mcx_contig_rec per call), `<bases>\n` per contig to seq_sink in the same
 * order in consecutive ranges (len_nodes + k - 1 bases, db_nodes_print); either may be NULL.  seq_off = the contig's
 * offset in that text.  The doubles are multiplied on the device in step order.  Nothing depends on the knobs
 * "contigs_batch" (seeds walked per launch), "contigs_held" and "contigs_nodes" (first capacities of a walk's list and
 * node ranges; a walk that fills one is run again with twice as much, stats.reruns counts those, MCX_ERR_NOMEM when that
 * no longer fits), on "grid" or on the table's size.  A walk whose state never repeats on a fork-free cycle (links that no
 * `thread` over this graph makes: one stored on a node of such a cycle is picked up again every round) grows until the
 * call ends with MCX_ERR_NOMEM; the reference spins there.  Refusals (MCX_ERR_ARG): a graph split over devices, intersect
 * mode, colour >= ncols, unknown flags, NaN bounds, nconf without conf. */
enum { MCX_CONTIGS_RESEED = 1, MCX_CONTIGS_NO_MISSING_CHECK = 2 };
typedef struct {
  uint32_t colour, flags;
  uint64_t ncontigs;
  double min_step_confid, min_cumul_confid; /* < 0: off */
  const double *conf;
  uint64_t nconf;
} mcx_contigs_params;
typedef struct {
  uint64_t seed_key[4];
  uint64_t len_nodes, seq_off;
  uint32_t num_junc, paths_held[2], paths_cntr[2];
  uint64_t max_step_gap[2];
  double gap_conf[2];
  uint8_t stop_causes[2], outdegree_rv, outdegree_fw;
} mcx_contig_rec;
typedef struct {
  uint64_t contigs, num_reseed_abort, seeds_not_found;
  uint64_t stop_causes[9]; /* ASSEM_STOP_*: Unknown, NoCovg, PopForkNoColCovg, ForkNoPaths, ForkInPaths, MissingPaths, HitLoop, LowStep, LowCumul */
  uint64_t wlk_steps[9];   /* GRPHWLK_*: the steps taken, by status */
  uint64_t total_nodes, total_junc, corrupt_links, reruns;
} mcx_contigs_stats;
int mcx_graph_contigs(mcx_graph *g, const uint8_t *seed_bases, const uint64_t *seed_offsets /* NULL: every key */, uint64_t nseeds,
                      const mcx_contigs_params *p, mcx_sink_fn rec_sink, void *rec_ctx, mcx_sink_fn seq_sink, void *seq_ctx,
                      mcx_contigs_stats *stats_accum /* optional, += */);

/* `bubbles` (src/commands/ctx_bubbles.c, src/tools/bubble_caller.c, src/graph/graph_crawler.c, src/graph/graph_cache.c)
 * WITHOUT LINK FILES: where the colours of a joined graph differ.  The graph view is that of mcx_graph_correct: union
 * edges, a k-mer is in a sample iff its value word in that colour is non-zero, an edge that names an absent k-mer counts
 * as no edge.  Unitigs are those of mcx_graph_unitig_stats, normalised as mcx_graph_unitigs prints them.
 *   Forks (bubble_caller_node): an oriented node with more than one successor that is a key.  FORKS ARE TAKEN IN
 *       ASCENDING KEY ORDER, FORWARD BEFORE REVERSE, and the ids `call<id>` count up from 0 in output order (the
 *       reference walks its hash table with racing threads).
 *   Paths (find_bubbles, graph_crawler_load_path_limit): colours ascending that hold the fork node; per colour every
 *       successor in ACGT order that is in the colour starts a path.  A path is a list of steps (unitig, orientation:
 *       FORWARD iff entered at the normalised unitig's first node).  After a step the unitig's k-mers are added to the
 *       path's total; at or above max_allele the path ends (the step stays).  Else the successors of the unitig's far
 *       end (graph_walker_choose without links): none: NOCOVG; one: go, in the colour or not (POPFWD); several of which
 *       one is in the colour: go there (POPFRK_COLFWD); none in the colour: NOCOLCOVG; several in the colour: NOLINKS.
 *       Repeat rule (repeat_walker.h:18-50; the state never changes without links): the first and second entry of an
 *       oriented node by a step of the path pass (the path's first node is no entry), the third ends the path without
 *       a step.  The reference's Bloom false positives are not reproduced.
 *   Cache (graph_cache_new_step): per fork the unitigs get local ids in the order they are first stepped on, over the
 *       paths in the order above; the steps on a unitig form a list, newest first.
 *   Candidates (write_bubbles_to_file, find_bubbles_ending_with): the local unitigs in id order; for each its FORWARD
 *       steps, then its REVERSE steps.  stats.candidates counts the lists of two steps or more.
 *   Filters (filter_bubbles), in order: graph_cache_is_3p_flank (the paths' first steps not all equal, the steps before
 *       the candidate not all equal, a missing one differs); graph_cache_remove_dupes (sorted by graph_cache_steps_cmp
 *       over the words local id << 1 | orientation up to and including the step, then the length; one step per equal
 *       run; fewer than 2: no call); remove_haploid_paths (the swap-with-last loop; a path is in haploid colour r when
 *       every k-mer of every unitig up to and including the end step is; fewer than 2: haploid_dropped += 1); unless
 *       MCX_BUBBLES_KEEP_SERIAL paths_all_share_unitig (the words of the steps before the end step are counted over all
 *       paths, a word met twice counts twice; a count equal to the number of paths: serial_dropped += 1, no call).
 *   Text (print_bubble): `>bubble.call<id>.5pflank kmers=<n>\n<first k-mer, then a base per further k-mer>\n`
 *       `>bubble.call<id>.3pflank kmers=<n>\n<a base per k-mer>\n` then per branch i `>bubble.call<id>.branch.<i>
 *       kmers=<n>\n<a base per k-mer>\n` and a blank line.  5' flank: db_unitig_extend from the reversed fork node, at
 *       most max_flank k-mers, turned round (it ends at the fork node).  3' flank: the whole unitig of the end step in
 *       the step's orientation.  Branch i: the nodes of path i before the end step, in the order the filters left.
 * One mcx_bubble_rec per call goes to rec_sink in output order, the text to text_sink in consecutive pieces of at most
 * "bubbles_chunk" bytes (a seam may fall anywhere); either may be NULL.  text_off = the call's offset in that text;
 * fork_key holds the key's words, most significant first.  Nothing in the records, the text or the stats depends on the
 * knobs "bubbles_batch" (fork k-mers per launch round), "bubbles_chunk", "grid" or on the table's size.
 * Refusals (MCX_ERR_ARG): a graph split over devices, intersect mode, max_allele == 0 or max_flank == 0, a haploid
 * colour >= ncols, more than 64 haploid colours, unknown flags, 4 x ncols x max_allele >= 2^31.  The decomposition is
 * reused when it still describes the table and made otherwise (the refusals of mcx_graph_clean). */
enum { MCX_BUBBLES_KEEP_SERIAL = 1 };
typedef struct {
  uint32_t max_allele, max_flank, flags, nhaploid;
  const uint32_t *haploid;
} mcx_bubbles_params;
typedef struct {
  uint64_t fork_key[4];
  uint64_t text_off, text_len;
  uint32_t fork_orient, num_branches, flank5p_kmers, flank3p_kmers;
} mcx_bubble_rec;
typedef struct {
  uint64_t forks, paths, steps;
  uint64_t stop_limit, stop_nocovg, stop_nocolcovg, stop_nolinks, stop_repeat;
  uint64_t candidates, bubbles, branches, haploid_dropped, serial_dropped;
} mcx_bubbles_stats;
int mcx_graph_bubbles(mcx_graph *g, const mcx_bubbles_params *p, mcx_sink_fn rec_sink, void *rec_ctx, mcx_sink_fn text_sink, void *text_ctx,
                      mcx_bubbles_stats *stats_accum /* optional, += */);

/* `breakpoints` (src/commands/ctx_breakpoints.c, src/tools/breakpoint_caller.c, src/graph/kmer_occur.{c,h},
 * src/graph/graph_crawler.c) WITHOUT LINK FILES: where the samples differ from an assembled reference genome, with
 * reference coordinates.  The graph view is that of mcx_graph_bubbles.  The reference colour is the handle's last
 * colour, ncols - 1; chromosome c is ref_bases[ref_offsets[c] .. ref_offsets[c + 1]) (ASCII, any case) and prints as
 * names[name_off[c] .. name_off[c + 1]) (already cleaned by the caller).
 *   Reference (kograph_create with add_missing_kmers, add_ref_seq_to_graph_mt): every maximal ACGT run of at least k
 *       bases goes into the last colour through mcx_graph_add_reads: coverage + 1 per occurrence, the edges between
 *       consecutive k-mers.  MCX_BREAKPOINTS_NO_REF_EDGES (breakpoint_caller.c:625-626): coverage only, no edge bits.
 *       MCX_BREAKPOINTS_REF_LOADED skips this: a second call on the same handle with other limits.
 *       MCX_BREAKPOINTS_LOAD_ONLY does this and returns (stats: ref_added alone): a host that has to print the k-mer count
 *       with the genome in ahead of the calls loads first and calls with REF_LOADED then (not both flags in one call).
 *   Occurrences (KOGraph): per key its (chrom, offset, orient of the key relative to the genome) for every start position
 *       of the genome whose k-mer is a key, ordered by (chrom, offset); offsets run on across non-ACGT bytes.
 *   Breaks (breakpoint_caller_node, follow_break): an oriented node whose key occurs in the genome, with one of its
 *       successors (keys only) that does not.  BREAKS ARE TAKEN IN ASCENDING KEY ORDER, FORWARD BEFORE REVERSE,
 *       SUCCESSORS IN ACGT ORDER, and the ids `call<id>` count up from 0 in output order (difference 1: the reference
 *       walks its hash table with racing threads).
 *   Walks (graph_crawler_load_path without links): the walker and the repeat rule of mcx_graph_bubbles; a step is the
 *       unitig that db_unitig_extend makes forward from the entered node.  After every step the run set is extended
 *       over the step's nodes in path orientation (kograph_filter_extend, korun_extend): the sorted active runs are
 *       scanned against the k-mer's occurrences with the reference's two pointers; strand = + iff the occurrence's
 *       orient equals the node's; a run continues iff last + 1 (strand +) or last - 1 (strand -) == offset, the sign
 *       taken from the occurrence; an occurrence that extends no run starts one at the node's index; an unextended run
 *       of MORE THAN min_ref k-mers moves to the ended set, a shorter one is dropped.  The walk goes on iff
 *       min qoffset(active) <= min qoffset(ended) and (max_ref == 0 or the longest run < max_ref) and, for a 5' flank,
 *       the active set is not empty (gcrawler_stop_at_ref_covg).  DIFFERENCE 3: the lengths of ended runs are taken
 *       from the ended runs (the reference reads koruns->b[i] while it loops over koruns_ended).  At the end the
 *       path's runs are the ended ones and the active ones of AT LEAST min_ref k-mers (gcrawler_finish_ref_covg).
 *   Per break: the 5' flank is walked from the reversed fork node in every colour (the reference colour included) that
 *       holds both nodes; walks that are node-for-node equal merge (graph_crawler_fetch).  A merged flank is reversed
 *       (koruns_reverse, nodes reverse-complemented), its runs sorted by (qoffset, chrom, first, last); without a run it
 *       is dropped.  Otherwise the allele is walked forward from the non-reference successor in each colour of the
 *       flank's set and merged likewise; a merged allele without a run is no call (process_contig).  DIFFERENCE 2: MERGED
 *       FLANKS AND MERGED ALLELES ARE ORDERED BY THEIR SMALLEST COLOUR, colours ascending inside a set (the reference
 *       orders them by cache-local unitig ids).
 *   Text (process_contig): flank3pidx = the qoffset of the allele's first sorted run, extra = min(k - 1, flank3pidx),
 *       path_kmers = flank3pidx - extra, kmer3poffset = k - 1 - extra;
 *       `>brkpnt.call<id>.5pflank chr=<runs>\n<first k-mer, then a base per further k-mer>\n`
 *       `>brkpnt.call<id>.3pflank chr=<runs>\n<a base per node from path_kmers on>\n`
 *       `>brkpnt.call<id>.path cols=<c0,c1,..>\n<a base per node before path_kmers>\n\n`; a run prints as korun_gzprint
 *       does: name:start-end:strand:offset, 1-based, with (first_kmer_idx, kmer_offset) = (0, 0) for the 5' flank and
 *       (flank3pidx, kmer3poffset) for the 3' flank.
 *   (Difference 4 is the command's: its header gives the real -R as max_ref_flank_kmers.)
 * One mcx_breakpoint_rec per call goes to rec_sink in output order, the text to text_sink in consecutive pieces of at
 * most "breakpoints_chunk" bytes (a seam may fall anywhere); either may be NULL.  Nothing in the records, the text or
 * the stats (but `reruns`) depends on the knobs "breakpoints_batch" (break k-mers per launch round), "breakpoints_chunk",
 * "breakpoints_runs" (runs a walk holds at a time before the batch is walked again with twice the room: reruns counts
 * the walks that outgrew theirs), "grid" or on the table's size.  stop_bound counts walks that reached the hard cap of
 * 4 n + 4 nodes for n k-mers, which the repeat rule keeps them from: always 0.
 * Refusals (MCX_ERR_ARG): a graph split over devices, intersect mode, ncols < 2, nchroms == 0 or > 2^30, a chromosome
 * longer than 2^32, min_ref == 0, max_ref != 0 && min_ref > max_ref, unknown flags; the refusals of mcx_graph_clean. */
enum { MCX_BREAKPOINTS_NO_REF_EDGES = 1, MCX_BREAKPOINTS_REF_LOADED = 2, MCX_BREAKPOINTS_LOAD_ONLY = 4 };
typedef struct {
  uint32_t min_ref, max_ref /* 0: no limit */, flags;
} mcx_breakpoints_params;
typedef struct {
  uint64_t fork_key[4];
  uint64_t text_off, text_len;
  uint32_t fork_orient, succ_base, num_cols, path_kmers;
  uint32_t flank5p_kmers, flank3p_kmers, flank5p_runs, flank3p_runs;
} mcx_breakpoint_rec;
typedef struct {
  uint64_t occurrences, ref_keys, ref_added;
  uint64_t breaks, flank_walks, flanks, flanks_norun, allele_walks, alleles, alleles_norun, calls;
  uint64_t steps, runs_started, runs_ended;
  uint64_t stop_runs, stop_maxref, stop_flank, stop_nocovg, stop_nocolcovg, stop_nolinks, stop_repeat, stop_bound;
  uint64_t reruns;
} mcx_breakpoints_stats;
int mcx_graph_breakpoints(mcx_graph *g, const uint8_t *ref_bases, const uint64_t *ref_offsets, uint64_t nchroms, const char *names,
                          const uint64_t *name_off, const mcx_breakpoints_params *p, mcx_sink_fn rec_sink, void *rec_ctx,
                          mcx_sink_fn text_sink, void *text_ctx, mcx_breakpoints_stats *stats_accum /* optional, += */);

/* `inferedges`: infer_kmer_edges (src/tools/infer_edges.c) for every record of `recs` (.ctx body
 * layout, ncols == the graph's colours) against the k-mers loaded into the graph.  Each edge that some
 * colour lacks (default, --all) or that some colour has and another lacks (MCX_INFER_POP, --pop)
 * names a neighbour k-mer; where the neighbour is in the graph and present in colour c, and the
 * record has coverage in c, the edge is added to colour c of the record.  Present means a non-zero
 * value in c (coverage or edges: node_in_cols of a file, graphs_load.c:151-154), or coverage > 0 with
 * MCX_INFER_PRESENCE_COVG (a stream, infer_edges.c:_add_edge_to_colours).  The records' edge bytes
 * are updated in place; *nmodified = records whose edges changed.  The table is only read.  Not for
 * a graph split over devices or in intersect mode.
 * mcx_graph_infer_edges streams host records through two device buffers (copies overlap the
 * kernel; MCX_INFER_CHUNK=<records> caps the chunk); mcx_graph_infer_edges_dev takes records in HBM. */
enum { MCX_INFER_POP = 1, MCX_INFER_PRESENCE_COVG = 2 };
int mcx_graph_infer_edges(mcx_graph *g, void *recs, uint64_t nrecs, int ncols, uint32_t flags, uint64_t *nmodified);
int mcx_graph_infer_edges_dev(mcx_graph *g, void *d_recs, uint64_t nrecs, int ncols, uint32_t flags, uint64_t *nmodified);

/* Table scans (imply a sync).
 * mcx_graph_kmer_covg       db_graph_get_kmer_covg (src/graph/db_graph.c:490-534): per colour, the
 *                           number of k-mers with coverage and their summed coverage (ncols entries)
 * mcx_graph_covg_histogram  the k-mer coverage histogram of `clean`'s first pass
 *                           (src/tools/clean_graph.c:365-377): hist[min(c, nbins-1)]++ for every
 *                           k-mer, c = its coverage summed over colours (saturating, db_node.h:302) */
int mcx_graph_kmer_covg(mcx_graph *g, uint64_t *nkmers, uint64_t *sumcov);
int mcx_graph_covg_histogram(mcx_graph *g, uint64_t *hist, uint32_t nbins);

/* Order-independent checksum of the graph: the sum, over its k-mers, of a 64-bit mix of the
 * exported record (key words, coverages clamped to 2^32-1, edges).  mcx_records_checksum computes
 * the same sum on the host from `.ctx` body records, so that two builds -- or a build and a file --
 * can be compared at sizes where byte-wise comparison of sorted exports is impractical. */
int mcx_graph_checksum(mcx_graph *g, uint64_t *checksum, uint64_t *nkmers);
uint64_t mcx_records_checksum(const void *recs, uint64_t nrecs, int kmer_size, int ncols);

/* The two ceilings of the device the build's roofline figures are quoted against ("to be
 * measured on the box by an in-repo microbenchmark and quoted next to the nominal figure"; the reference
 * times its table and the competitor in one script as well, results/hash_table_benchmark/benchmark-tables.sh:14-59).
 * mcx_ubench_stream      streaming rates in GB/s over two buffers of `bytes` each (far beyond the 256 MiB Infinity
 *                        Cache): copy (read + write bytes counted), read only, write only; 16-byte accesses
 * mcx_ubench_random_rmw  random 64-byte-sector rates per second over a `table_bytes` working set of 16-byte
 *                        records: agent-scope atomic add (what an occurrence costs the direct insert), 16-byte
 *                        load, load + atomic.  Any out pointer may be NULL. */
int mcx_ubench_stream(int device, uint64_t bytes, double *copy_gbs, double *read_gbs, double *write_gbs);
int mcx_ubench_random_rmw(int device, uint64_t table_bytes, uint64_t nupdates, double *rmw_per_s,
                          double *load16_per_s, double *load_rmw_per_s);

/* `.ctx` records on the device without a graph handle (host buffers, .ctx body layout).
 * mcx_sort_records    sort in place by k-mer, most significant word first -- what `sort` does with
 *                     qsort (src/commands/ctx_sort.c:133-152; binary_kmers_qcmp_unaligned_ptrs)
 * mcx_records_sorted  *first_unsorted = index of the first record whose k-mer is not greater than
 *                     its predecessor's, or -1 (the check `index` makes, src/commands/ctx_index.c:136) */
int mcx_sort_records(void *recs, uint64_t nrecs, int kmer_size, int ncols, int device);
int mcx_records_sorted(const void *recs, uint64_t nrecs, int kmer_size, int ncols, int device,
                       int64_t *first_unsorted);

/* `join` (src/commands/ctx_join.c; graph_writer_merge_mkhdr of src/graph/graph_writer.c; graph_load of
 * src/graph/graphs_load.c): merge .ctx files by a device sort and a segmented reduce -- no graph handle, no hash table,
 * so there is no capacity to guess and nothing that can be full, and the output is always sorted by key.
 *   mcx_join_create       out_ncols colours in the output; n_isec intersection graphs (`-i`, 0 = none).
 *       MCX_JOIN_KEEP_EMPTY: a key of the intersection that no input graph supplies is written as an all-zero record
 *       (graph_write_empty plus the update); without the flag it is not written.
 *   mcx_join_configure    test knobs, the answers must not change with them: "grid" (at most n blocks per launch, 0 =
 *       CUs x 8) and "out_chunk" (bytes of output per sink call, 0 = 64 MiB; a seam may fall inside a record).
 * Three entries serve one caller each and are kept small on purpose: get_stats (the command's per-file "[GReader]
 * Loaded" line), buffer (the command's pinned read buffer: a C host has no other way to pinned memory) and phases
 * (tools/bench_join.py).
 *   mcx_join_get_stats    the counts so far (the records read and kept; the rest is filled by finish)
 *   mcx_join_phases       host-clock milliseconds so far of the four phases (tools/bench_join.py): upload + key
 *       extraction (the add_records calls), sort, runs + intersection, reduce + write-out (the sink's time included)
 *   mcx_join_buffer       pinned host memory of `bytes` bytes owned by the handle (one at a time; freed by the next call
 *       and by destroy): a reader fills it from the file and hands it to mcx_join_add_records.
 *   mcx_join_add_records  host records in .ctx body layout (W x u64 key, file_ncols x u32 coverage, file_ncols x u8
 *       edges, byte-packed), any number of calls per file.  source = -1: an input graph, whose file colour from_col[i]
 *       goes to output colour into_col[i] (pairs may repeat sources and targets); source = 0 .. n_isec - 1: the
 *       intersection graph of that rank, every selected colour flattened into one (into_col is not read); rank 0
 *       supplies the edge mask.  A record whose coverage is zero in all the colours the filter selects is dropped here
 *       (keep_kmer, graphs_load.c:121-124), edges or not.  The records stay in HBM as uploaded, with one 64-bit locator
 *       per kept record: the cost is that of the input bytes, not records x out_ncols.  Synchronous.
 *   mcx_join_finish       sorts the locators by key (all W words), reduces every run of equal keys to one record and
 *       hands the records to `sink` in ascending key order, in consecutive byte ranges of at most "out_chunk" bytes.
 *       covg[into] is the sum, saturating at 2^32 - 1 (SAFE_ADD_COVG), and edges[into] the OR over every (record of the
 *       run, filter pair of its call); colours nobody loads stay zero.  A key that a file repeats, or a file given
 *       twice, is summed like any other.  With intersection graphs (ctx_join.c:262-306 as it behaves with --ncols 1):
 *       a key is kept iff it survives the drop rule in EVERY intersection source -- presence per source, where the
 *       reference counts loaded records, which differs only for a file that repeats a key; records of other keys are
 *       dropped; every output colour's edges are ANDed with the OR, over the selected colours, of the edges that
 *       source 0 has for the key.  The handle is spent afterwards (a second finish writes nothing).
 *       MCX_ERR_NOMEM (from add_records or finish) when the records, the sort scratch or the output chunk do not fit
 *       the free HBM: splitting the key range into several passes is out of scope. */
typedef struct mcx_join mcx_join;
enum { MCX_JOIN_KEEP_EMPTY = 1 };
typedef struct {
  uint64_t recs_read, recs_kept;            /* input graphs */
  uint64_t isec_recs_read, isec_recs_kept;  /* intersection graphs */
  uint64_t kmers_written;
  uint64_t kmers_intersection;              /* keys present in every intersection source (0 without any) */
  uint64_t kmers_written_no_covg;           /* all-zero records written under MCX_JOIN_KEEP_EMPTY */
} mcx_join_stats;
int mcx_join_create(mcx_join **j, int kmer_size, int out_ncols, int n_isec, uint32_t flags, int device);
int mcx_join_configure(mcx_join *j, const char *key, uint64_t value);
int mcx_join_get_stats(const mcx_join *j, mcx_join_stats *stats);
int mcx_join_phases(const mcx_join *j, double *ms /* [4] */);
int mcx_join_buffer(mcx_join *j, size_t bytes, void **ptr);
int mcx_join_add_records(mcx_join *j, int source, const void *recs, uint64_t nrecs, int file_ncols,
                         const int32_t *from_col, const int32_t *into_col, int nmap);
int mcx_join_finish(mcx_join *j, mcx_sink_fn sink, void *ctx, mcx_join_stats *stats);
void mcx_join_destroy(mcx_join *j);

/* `links` (src/commands/ctx_links.c, src/paths/link_tree.c): clean, list and count the links of a version-4 .ctp body,
 * one colour.  No graph handle and no table: a k-mer is its ordinal within a piece, the per-k-mer trie of junction
 * strings is a sorted list with longest-common-prefix values (mcx_links.h).
 *   mcx_links_create      kmer_size: the k of the file (odd, any size: k-mers stay text).
 *   mcx_links_configure   test knobs, the answers must not change with them: "grid" (at most n blocks per launch, 0 =
 *       CUs x 8) and "out_chunk" (bytes of text per sink call, 0 = 64 MiB; a seam may fall inside a line).
 *   mcx_links_buffer      pinned host memory of `bytes` bytes owned by the handle (one at a time; freed by the next call
 *       and by destroy), which the reader fills.
 *   mcx_links_add_text    `text`: whole k-mer blocks of the body (`<kmer> <n>` lines, each followed by its link lines
 *       `<F|R> <njuncs> <count> <juncs> seq=<..> juncpos=<..>`); begins at a line start and ends behind a newline; `#`
 *       comment lines and empty lines anywhere.  flags: MCX_LINKS_CLEAN (tree links with a count below `cutoff` go),
 *       MCX_LINKS_HIST (every tree link with dist < distsize adds one to hist[dist][min(count, covgsize - 1)], before
 *       cleaning).  max_kmers: the k-mers of this piece beyond that many are ignored with their lines (0 = no limit).
 *       ctp_sink gets the .ctp lines of the written links in file order of the k-mers (a link is written iff no other
 *       input link of its k-mer and orientation extends it and its summed count is at least the cut-off; the `<kmer>
 *       <n>` line is left out with the block when n is 0), list_sink the rows `<k + dist + 1>,<count>` of the tree
 *       links that survive; either may be NULL.  Statistics are gathered either way.  Synchronous.  MCX_ERR_INVAL for a
 *       malformed line: nothing of the piece is counted or delivered.
 *   mcx_links_get_stats   the totals so far.
 *   mcx_links_hist        distsize x covgsize counters, accumulated over the calls (the sizes of the first
 *       MCX_LINKS_HIST call hold for the handle).
 *   mcx_links_error       after MCX_ERR_INVAL: the refusal (MCX_LINKS_BAD_*) and the byte offset, within the text of that
 *       call, of the first bad line in file order.
 *   mcx_links_phases      host-clock milliseconds so far of the eight phases (tools/bench_links.py): upload, lines,
 *       parse, sort, reduce + lcp, tree links (histogram, list), what is written, .ctp text. */
typedef struct mcx_links mcx_links;
enum { MCX_LINKS_CLEAN = 1, MCX_LINKS_HIST = 2 };
enum {
  MCX_LINKS_BAD_KMER_LINE = 1,    /* k-mer line not ACGT{k} <int> */
  MCX_LINKS_BAD_ORIENT = 2,       /* first column not a lone F or R */
  MCX_LINKS_BAD_NUMBER = 3,       /* njuncs or count not a number */
  MCX_LINKS_MULTI_COLOUR = 4,     /* a comma in the count column: "Can only clean a single colour" */
  MCX_LINKS_BAD_JUNCTION = 5,     /* non-ACGT junctions */
  MCX_LINKS_NJUNCS_RANGE = 6,     /* njuncs of 0 or above 32767 */
  MCX_LINKS_NJUNCS_LENGTH = 7,    /* njuncs != length of the junction string */
  MCX_LINKS_NO_SEQ = 8,           /* no seq= tag */
  MCX_LINKS_NO_JUNCPOS = 9,       /* no juncpos= tag */
  MCX_LINKS_JUNCPOS_COUNT = 10,   /* juncpos is no list of njuncs numbers */
  MCX_LINKS_SEQ_LENGTH = 11,      /* strlen(seq) != k + juncpos[last] + 1 */
  MCX_LINKS_SEQ_BASE = 12,        /* seq[k + juncpos[i]] != juncs[i] */
  MCX_LINKS_LINK_BEFORE_KMER = 13,/* a link line before any k-mer line */
  MCX_LINKS_COUNT_COLUMNS = 14    /* mcx_pjoin_add_text: the count column has not as many numbers as the file has colours */
};
typedef struct { uint32_t flags, distsize, covgsize, reserved; uint64_t cutoff, max_kmers; } mcx_links_params;
typedef struct { uint64_t kmers_read, kmers_with_links, links, link_bytes, tree_links, links_in; } mcx_links_stats;
int mcx_links_create(mcx_links **l, int kmer_size, int device);
int mcx_links_configure(mcx_links *l, const char *key, uint64_t value);
int mcx_links_buffer(mcx_links *l, size_t bytes, void **ptr);
int mcx_links_add_text(mcx_links *l, const void *text, uint64_t nbytes, const mcx_links_params *p, mcx_sink_fn ctp_sink, void *ctp_ctx,
                       mcx_sink_fn list_sink, void *list_ctx);
int mcx_links_get_stats(const mcx_links *l, mcx_links_stats *stats);
int mcx_links_hist(mcx_links *l, uint64_t *out);
int mcx_links_error(const mcx_links *l, int *code, uint64_t *byte_offset);
int mcx_links_phases(const mcx_links *l, double *ms /* [8] */);
void mcx_links_destroy(mcx_links *l);

/* `pjoin` (src/commands/ctx_pjoin.c, src/graph_paths/gpath_reader.c, src/paths/gpath_subset.c): the bodies of version-4
 * .ctp files merged into one, a colour per file or several files into one colour.  No graph handle and no hash table:
 * the links of all files are sorted by (k-mer as written, orientation, junction string) and every run of equal links is
 * reduced to one link whose count per colour is min(255, the sum over its lines) (mcx_pjoin.h).  A prefix and its
 * extension are different links; seq= and juncpos= are not read.
 *   mcx_pjoin_create      kmer_size: the k of the files (odd, 3..127); out_ncols: colours of the output.
 *   mcx_pjoin_configure   test knobs, the answers must not change with them: "grid" (at most n blocks per launch, 0 =
 *       8 per compute unit), "out_chunk" (bytes of text per sink call, 0 = 64 MiB), "compact" (1 = the store is reduced to
 *       its unique links after every add), "max_bytes" (the ceiling of the store's records, junction words and counts,
 *       0 = what the device has free; a full store compacts once before an add answers MCX_ERR_NOMEM).
 *   mcx_pjoin_buffer      pinned host memory of `bytes` bytes owned by the handle (one at a time; freed by the next call
 *       and by destroy).
 *   mcx_pjoin_add_text    `text`: lines of the body of a file with src_ncols colours (`<kmer> <n>` lines, each followed by
 *       its `<F|R> <njuncs> <c0,..> <juncs> [tags]` lines; comment and empty lines anywhere), ending with a newline, less
 *       than 2 GB.  filter: nfilter pairs (from, into): into[into] += count[from]; from >= src_ncols or into >= out_ncols
 *       is MCX_ERR_ARG.  A line whose mapped counts are all zero is dropped.  piece_stats (or NULL): the lines of this
 *       piece.  A malformed line is MCX_ERR_INVAL (mcx_pjoin_error: the refusal of mcx_graph_links_load_text, or
 *       MCX_LINKS_COUNT_COLUMNS, and the byte offset of the first bad line); nothing of a refused piece is stored, and
 *       nothing of a piece that met MCX_ERR_NOMEM.  Synchronous.
 *   mcx_pjoin_finish      the merged body to the sink (or NULL: totals only): per k-mer, in ascending order of the k-mer
 *       text, `<kmer> <nlinks>` and its links `<F|R> <njuncs> <c0,..,cN-1> <juncs>`, F before R, junction strings in text
 *       order, a prefix before its extensions.  stats (or NULL): as mcx_pjoin_get_stats.  The store is kept.
 *   mcx_pjoin_phases      host-clock milliseconds so far of the six phases (tools/bench_pjoin.py): upload, lines,
 *       parse + store, sort, reduce, text. */
typedef struct mcx_pjoin mcx_pjoin;
typedef struct { uint64_t kmer_lines, link_lines, links_kept, kmers_n_mismatch /* `<kmer> <n>` with n != the link lines that follow */; } mcx_pjoin_piece_stats;
typedef struct {
  uint64_t kmer_lines, link_lines, links_kept, kmers_n_mismatch; /* summed over the accepted pieces */
  uint64_t kmers, links, path_bytes;                             /* of the merged output (mcx_pjoin_finish; path_bytes as mcx_links_info) */
  uint64_t compactions, store_bytes, peak_store_bytes;           /* the store: times compacted, bytes held now and at most (after an add) */
} mcx_pjoin_stats;
int mcx_pjoin_create(mcx_pjoin **h, int kmer_size, int out_ncols, int device);
int mcx_pjoin_configure(mcx_pjoin *h, const char *key, uint64_t value);
int mcx_pjoin_buffer(mcx_pjoin *h, size_t bytes, void **ptr);
int mcx_pjoin_add_text(mcx_pjoin *h, const void *text, uint64_t nbytes, int src_ncols, const int32_t *filter /* nfilter x (from, into) */, int nfilter,
                       mcx_pjoin_piece_stats *piece_stats /* or NULL */);
int mcx_pjoin_finish(mcx_pjoin *h, mcx_sink_fn sink, void *ctx, mcx_pjoin_stats *stats /* or NULL */);
int mcx_pjoin_get_stats(const mcx_pjoin *h, mcx_pjoin_stats *stats);
int mcx_pjoin_error(const mcx_pjoin *h, int *code, uint64_t *byte_offset);
int mcx_pjoin_phases(const mcx_pjoin *h, double *ms /* [6] */);
void mcx_pjoin_destroy(mcx_pjoin *h);

/* Sharded build, exchange format v3 ("reads travel, not occurrences"; odd k in 29..63,
 * mcx_superk_supported(); records are mcx_superk_record_bytes(k) = 16 bytes for one-word keys, 32
 * for two-word keys: an 80-base window).  The owner of a k-mer is a function of its canonical minimizer
 * (smallest hashed canonical 13-mer), so consecutive k-mers of a read mostly share an owner and
 * are sent as one 16-byte record: the 48-base window of 16 consecutive positions plus the start and
 * length of the run -- about 2.3 bytes per occurrence instead of 8.5.  Every rank holds an ordinary
 * (unsharded) table with the k-mers it owns.
 *   mcx_superk_owner           owner of a canonical key (host; tests)
 *   mcx_graph_superk_layout    records per (owner, replica) segment for calls of at most
 *                              `positions_per_call` stream bytes; segs_per_owner replicas per owner
 *   mcx_graph_superk_bins_dev  sender: d_recs[nparts][segs][seg_cap] 16-byte records with fills
 *                              d_counts[segs][nparts] (u64, replica-major, zeroed by the caller); a
 *                              full segment drops records and raises MCX_ERR_FULL at the next sync
 *   mcx_graph_add_superk_dev   owner: k-merise nseg received segments d_recs[nseg][seg_cap] (fills
 *                              d_counts[nseg] in device memory) into the region bins; applied at the
 *                              next flush */
int mcx_superk_supported(int kmer_size);
int mcx_superk_record_bytes(int kmer_size);
uint32_t mcx_superk_owner(const uint64_t *key_words, int kmer_size, int nparts);
int mcx_graph_superk_layout(mcx_graph *g, int nparts, uint64_t positions_per_call, uint32_t *segs_per_owner,
                            uint64_t *seg_cap);
int mcx_graph_superk_bins_dev(mcx_graph *g, const void *d_stream, uint64_t nbytes, int nparts, void *d_recs,
                              void *d_counts, uint64_t seg_cap);
int mcx_graph_add_superk_dev(mcx_graph *g, int colour, const void *d_recs, const void *d_counts, uint32_t nseg,
                             uint64_t seg_cap, uint64_t kmers_upper_bound);

/* Host-side packer of the staging path of mcx_graph_add_reads, exported for its test: n (a
 * multiple of 32) ASCII characters -> n / 16 code words (2 bits per base, A=0 C=1 G=2 T=3 as
 * src/basic/dna.c:8-25, first base on top) and n / 16 x 16 invalid flags (first base = bit 15; set
 * for every character that is not one of ACGTacgt). */
void mcx_pack_bases(const uint8_t *src, uint64_t n, uint32_t *code, uint16_t *inv);

/* The one-pass packer of the same staging path (round 4), exported for its test: the reads
 * bases[off[i] .. off[i+1]) as the stream "128 separators, read 0, separator, read 1, separator, ...,
 * separators up to a multiple of 64 positions" -> code[p / 16], inv[p / 16]; returns the number of
 * positions (0: cap_pos too small, or fused != 0 on a host without AVX-512).  fused == 0 assembles
 * the ASCII stream and packs it with mcx_pack_bases: both must give the same words.  Replaces the
 * per-read copy of the reference's workers (src/basic/async_read_io.c:283-310 hands whole reads over). */
uint64_t mcx_pack_reads_host(const uint8_t *bases, const uint64_t *off, uint64_t nreads, uint32_t *code,
                             uint16_t *inv, uint64_t cap_pos, int fused);

/* Wait for all submitted work; reports MCX_ERR_FULL if any insert ran out of
 * slots (the reference dies with "Hash table is full"). */
int mcx_graph_sync(mcx_graph *g);

/* hash_table_nkmers (src/graph/hash_table.h:37). Implies a sync. */
int mcx_graph_nkmers(mcx_graph *g, uint64_t *n);
/* Contig/k-mer counters accumulated by the device since create/reset. */
int mcx_graph_device_stats(mcx_graph *g, mcx_load_stats *out);

/* How the inserts went: the slow-but-correct paths ("cliffs") of the partitioned build, made visible.  The
 * reference prints its own insert diagnostics, the collision histogram of hash_table_print_stats
 * (src/graph/hash_table.c:301-333); these are the ones this table has.  All zero on well-spread input (bench
 * C2: asserted in tests/test_gpu_fullsize.py); printed by `mccortex<K> build` under MCX_TIMING=1.
 *   fallback_inserts  occurrences that did not fit their partition bin (hot k-mers, an owner far above its share)
 *                     and took the per-occurrence lock-free insert in HBM instead of the LDS insert
 *   foreign_inserts   occurrences whose key another shard owns, handed to this shard through an entry that does
 *                     not route (mcx_graph_add_reads on a shard handle): inserted on the spot
 *   spilled           multi-GPU table: occurrences (exchange v2) / super-k-mer records (v3) that did not fit a
 *                     send segment and went through the sender's spill area, routed by the host
 *   flushes           passes over the table made by the partitioned insert (per colour with buffered tuples)
 * Implies a sync; a multi-GPU handle reports sums over its shards. */
typedef struct {
  uint64_t fallback_inserts;
  uint64_t foreign_inserts;
  uint64_t spilled;
  uint64_t flushes;
} mcx_insert_stats;
int mcx_graph_insert_stats(mcx_graph *g, mcx_insert_stats *out);

/* HIP stream the handle submits on (hipStream_t as void*), so callers can
 * bracket it with their own events. */
void *mcx_graph_stream(mcx_graph *g);

/* Replaces graph_write_all_kmers_direct (src/graph/graph_writer.c:182-268):
 * streams the records in .ctx v6 body layout (W x u64 key, ncols x u32 covg,
 * ncols x u8 edges; src/graph/graph_writer.c:116-127) to `sink` in chunks.
 * sorted != 0 orders records by key (hash_table_sorted, hash_table.c:362-374),
 * which is the only order in which the reference output is reproducible. */
int mcx_graph_export(mcx_graph *g, int sorted, mcx_sink_fn sink, void *ctx);

/* `unitigs` (src/commands/ctx_unitigs.c): every unitig of the decomposition above as text, written by kernels
 * and handed to `sink` in consecutive byte ranges (like mcx_graph_export's).  The decomposition of
 * mcx_graph_unitig_stats is reused when it still describes the table, and made otherwise.  Coverage is not
 * used; edges are the union over the colours.  The same refusals as `clean`; the table is only read.
 * The text depends on the graph alone (not on the table's size or load, the "grid" knob or the chunk size):
 *   - every unitig is normalised in all three formats: a chain starts at the end with the lower key, a closed
 *     cycle at its lowest key read forwards, a single k-mer is forward;
 *   - unitigs are numbered 0, 1, ... in ascending order of the key of their first k-mer, and appear so;
 *   - FASTA: ">unitig<i> prev=<P> next=<N>\n<seq>\n".  GFA: "H\tVN:Z:1.0", the S lines, then the L lines.
 *     DOT: three preamble lines, the node lines, a blank line, the edge lines, "}";
 *   - an L / DOT edge line is printed for an edge that leaves a unitig end when the key of that end k-mer is
 *     below the key of the neighbour k-mer, or when the two are the same k-mer and not both sides are reverse
 *     (_print_edge with `node < next` decided by key); the lines are sorted by (source unitig, left end
 *     before right end, edge base ACGT).
 * Scratch while the call runs, beside the decomposition: MCX_UNITIGS_BYTES_PER_KMER per k-mer and
 * MCX_UNITIGS_BYTES_PER_UNITIG per unitig (GFA / DOT; FASTA needs 104 less), plus the radix sort's temporary.
 * mcx_graph_configure(g, "unitigs_chunk", bytes) caps the chunk (tests of the chunk seams).
 * mcx_graph_unitigs_dev writes no text: it fills caller-allocated device arrays (NULL: not wanted), the
 * per-k-mer ones in dense order with nkmers entries -- keys (W words each, most significant first), unitig
 * number, rank in the normalised unitig, orientation there (1 = reverse complement) -- and the per-unitig ones
 * by unitig number (at most nkmers entries): index of the first k-mer in the per-k-mer arrays, length. */
enum { MCX_UNITIGS_FASTA = 0, MCX_UNITIGS_GFA = 1, MCX_UNITIGS_DOT = 2 };
enum { MCX_UNITIGS_POINTS = 1 }; /* DOT: print unitigs as points (-P) */
#define MCX_UNITIGS_BYTES_PER_KMER 65
#define MCX_UNITIGS_BYTES_PER_UNITIG 170
typedef struct { uint64_t num_unitigs, num_kmers, num_bytes, num_cycles; } mcx_unitigs_stats;
typedef struct {
  uint64_t *keys;
  uint32_t *unitig, *rank;
  uint8_t *orient;
  uint32_t *first, *length;
} mcx_unitigs_arrays;
int mcx_graph_unitigs(mcx_graph *g, int format, uint32_t flags, mcx_sink_fn sink, void *ctx, mcx_unitigs_stats *stats);
int mcx_graph_unitigs_dev(mcx_graph *g, const mcx_unitigs_arrays *out, mcx_unitigs_stats *stats);

/* Host-side primitives exported for parity tests of rows A-C (no device). */
void mcx_kmer_from_str(const char *seq, int kmer_size, uint64_t *words_out);
void mcx_kmer_canonical(const uint64_t *words_in, int kmer_size, uint64_t *key_out, int *orient_out);
uint32_t mcx_kmer_hash(const uint64_t *key_words, int kmer_size, uint32_t initval);

#ifdef __cplusplus
}
#endif
#endif /* MCX_GPU_H_ */
