/* host.h -- C host side of the `mccortex<K>` commands over the MI355X backend (include/mcx_gpu.h).
 * Mirrors the reference's command surface: src/main/mccortex.c (dispatcher), src/commands/ctx_*.c (options, messages,
 * flow), src/basic/cmd.c and src/graph/cmd_mem.c (shared option handling), src/graph/graph_writer.c (.ctx v6). */
#ifndef MCX_HOST_H_
#define MCX_HOST_H_

#include <pthread.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifndef MAX_KMER_SIZE
#define MAX_KMER_SIZE 31
#endif
/* MIN_KMER_SIZE = MAXK - 30, and 3 for MAXK = 31 (reference Makefile:33-48); literals, because the usage texts print them */
#if MAX_KMER_SIZE == 31
#define MIN_KMER_SIZE 3
#elif MAX_KMER_SIZE == 63
#define MIN_KMER_SIZE 33
#elif MAX_KMER_SIZE == 95
#define MIN_KMER_SIZE 65
#elif MAX_KMER_SIZE == 127
#define MIN_KMER_SIZE 97
#else
#error "MAX_KMER_SIZE must be 31, 63, 95 or 127 (three- and four-word keys are the widest the backend builds)"
#endif
#define MCX_STR_(x) #x
#define MCX_STR(x) MCX_STR_(x)
#define CMD_NAME "mccortex" MCX_STR(MAX_KMER_SIZE)

/* ---- logging (src/global/ctx_output.h:14-34) ---- */
extern FILE *msg_out; /* NULL = quiet */
extern int host_fast_exit_ok; /* set by a `build` that finished and saw its device idle: main() may _exit */
void status(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void warn(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void die(const char *fmt, ...) __attribute__((format(printf, 1, 2), noreturn));
void print_usage(const char *usage, const char *errfmt, ...) __attribute__((noreturn));
void host_set_cmdline(int argc, char **argv);

/* ---- number parsing / formatting (src/global/util.c:108-117,206-222,251-264,343) ---- */
bool parse_entire_size(const char *s, size_t *out);
bool parse_entire_uint(const char *s, unsigned *out);
bool mem_to_integer(const char *s, size_t *bytes);
char *ulong_to_str(unsigned long n, char *out);
char *bytes_to_str(unsigned long n, int decimals, char *out);
/* binary_kmer_to_str (binary_kmer.c:190-210) for the key of a .ctx record: word 0 (most significant) first */
void kmer_words_to_str(const unsigned char *rec, unsigned kmer_size, char *out);

/* ---- table sizing: entry counts and memory figures of -n / -m as the reference computes them
 * (src/basic/hash_mem.c:5-51, src/graph/cmd_mem.c:38-130) ---- */
typedef struct { uint64_t nbuckets, bucket_size, capacity; size_t bytes; } table_plan;
table_plan table_plan_for_kmers(uint64_t nkmers, size_t entry_bits);
table_plan table_plan_for_memory(size_t mem, size_t entry_bits);
const char *table_plan_for_build(size_t mem_to_use, bool mem_set, size_t num_kmers, bool nkmers_set, size_t entry_bits,
                                 int64_t max_kmers, table_plan *out, char *errbuf, size_t errlen);

/* ---- sequence input (replaces seq_file + src/basic/async_read_io.c for FASTA/FASTQ/plain, .gz) ---- */
typedef enum { SEQ_FMT_UNKNOWN = 0, SEQ_FMT_FASTA, SEQ_FMT_FASTQ, SEQ_FMT_PLAIN, SEQ_FMT_SAM } seq_fmt;
typedef struct seq_in seq_in;
seq_in *seq_in_open(const char *path); /* "-" = stdin; NULL on failure */
void seq_in_close(seq_in *s);
seq_fmt seq_in_format(seq_in *s);
const char *seq_in_path(const seq_in *s);
/* Appends reads to the batch until >= max_bases are held or EOF.  Returns reads appended,
 * 0 at EOF.  bases/quals are concatenated, offsets has nreads+1 entries. */
typedef struct {
  uint8_t *bases, *quals;
  uint64_t *offsets;
  size_t nreads, nbases, cap_bases, cap_reads;
  bool want_quals;
  /* names, kept only after read_batch_keep_names(): read i is names[name_off[i] .. name_off[i + 1]), the header line
   * behind '>' or '@' with its comment and without a trailing '\r'; plain input gives empty names */
  bool want_names;
  char *names;
  uint64_t *name_off;
  size_t names_len, cap_names, cap_name_reads;
} read_batch;
void read_batch_init(read_batch *b, bool want_quals);
void read_batch_keep_names(read_batch *b);
/* whether two read names belong to mates (seq_read_names_cmp): how --seqi of `reads` pairs consecutive reads */
bool seq_names_match(const char *a, size_t alen, const char *b, size_t blen);
void read_batch_clear(read_batch *b);
void read_batch_free(read_batch *b);
size_t seq_in_fill(seq_in *s, read_batch *b, size_t max_bases);
void read_batch_append(read_batch *dst, const read_batch *src, size_t i); /* read i of src */
/* FASTQ offset guess from the qualities seen so far (33 or 64); 0 if no qualities */
int seq_in_guess_fq_offset(const seq_in *s);
int fq_offset_from_range(int qmin, int qmax);
/* the offset of a file from its first 1000 records; 0 = no qualities, -1 = stdin (cannot look ahead) */
int fq_offset_probe(const char *path);

/* Multi-threaded parse of an uncompressed regular file (par_ingest.c): `submit` is called on the
 * calling thread for every batch; `started` (may be NULL) once, on the calling thread, after the
 * parser threads have been started and before the first batch is waited for.  Returns 0 = done,
 * 1 = not suitable (nothing submitted: use the sequential parser), 2 = irregular record met after
 * submission began. */
int par_ingest(const char *path, seq_fmt fmt, int nthreads, bool want_quals, size_t batch_bases,
               void (*submit)(void *arg, read_batch *b, int fq_offset_guess), void (*started)(void *arg), void *arg);

/* ---- .ctx header: GraphInfo arithmetic, writer, reader
 * (src/basic/graph_info.c, src/graph/graph_writer.c:11-110, src/graph/graph_file_reader.c:78-340,
 *  colour filters src/basic/file_filter.c) ---- */
typedef struct { /* ErrorCleaning, graph_info.h */
  uint8_t cleaned_tips, cleaned_unitigs, cleaned_kmers, is_graph_intersection;
  uint32_t clean_unitigs_thresh, clean_kmers_thresh;
  char *intersection_name;
} err_cleaning;
typedef struct { /* GraphInfo */
  uint32_t mean_read_length;
  uint64_t total_sequence;
  long double seq_err;
  char *name;
  err_cleaning cleaning;
} col_info;
void col_info_init(col_info *c);
void col_info_free(col_info *c);
void col_info_set_name(col_info *c, const char *name);
void col_info_update(col_info *c, uint64_t bases_loaded, uint64_t contigs);
void col_info_merge(col_info *dst, const col_info *src); /* graph_info_merge */
size_t ctx_write_header(FILE *fh, uint32_t kmer_size, uint32_t ncols, const col_info *cols);

typedef struct { uint32_t from, into; } col_filter;
typedef struct {
  char *input, *path;        /* "0,1:in.ctx:2-3" and "in.ctx" */
  FILE *fh;
  uint32_t version, kmer_size, num_words, num_cols;
  col_info *ginfo;           /* [num_cols] */
  size_t hdr_size;
  long long file_size, num_kmers; /* -1 when reading a stream */
  col_filter *filter;        /* sorted by `into` */
  size_t nfilter, into_ncols;
} ctx_reader;
/* graph_file_open2: parse "<into>:path:<from>", read and check the header; dies on error */
void ctx_reader_open(ctx_reader *r, const char *input, size_t into_offset, size_t min_k, size_t max_k);
void ctx_reader_open_mode(ctx_reader *r, const char *input, const char *mode, size_t into_offset, size_t min_k, size_t max_k);
bool ctx_reader_from_direct(const ctx_reader *r); /* file_filter_from_direct: no colour filter in the path */
/* graph_write_header (graph_writer.c:62-110): the parsed header as it is, no merging */
size_t ctx_write_header_raw(FILE *fh, const ctx_reader *r);
void ctx_reader_close(ctx_reader *r);
/* the same argument syntax for a file that is no .ctx (`pjoin`'s .ctp inputs): the path between the colour lists (to be
 * freed), and, once the file's colour count is known, the filter as ctx_reader_open sets it (*filter to be freed);
 * dies with "Invalid filter path" as ctx_reader_open does */
char *ctx_arg_path(const char *input);
void ctx_arg_filter(const char *input, uint32_t num_cols, size_t into_offset, col_filter **filter, size_t *nfilter, size_t *into_ncols);

/* cleaning_pick_kmer_threshold (src/tools/clean_graph.c): the unitig cleaning threshold from the k-mer coverage
 * histogram (arrlen bins), or -1; the outputs may be NULL (clean_thresh.c) */
int cleaning_pick_kmer_threshold(const uint64_t *kmer_covg, size_t arrlen, double *alpha_est, double *beta_est,
                                 double *false_pos, double *false_neg);

/* ---- shared by the commands (cmd_common.c; calls into libmcxgpu, so not part of libmcxhost.so) ---- */
struct option;
struct mcx_graph;
#define DEFAULT_MEM (1UL << 29) /* cmd.h:13 */
/* cmd_get_longopt_str: "-x, --name" for c < 256, "--name" for a long-only option, "-x, --Unknown" without a match */
void cmd_optname(const struct option *opts, int c, char *out);
void mcx_check(int rc, const char *what); /* dies with "Hash table is full" or "<what>: <mcx_last_error()>" */
int write_sink(void *ctx, const void *data, size_t nbytes); /* export sink: fwrite to the FILE * in ctx */
const char *plural(uint64_t n);
const char *outpath(const char *p); /* "-" reads STDOUT */
/* -m / -n / -t (cmd_mem_args_set_memory, cmd_mem_args_set_nkmers; cmd_uint32_nonzero after cmd_check(!nthreads)) */
typedef struct { size_t mem_to_use, num_kmers; bool mem_set, nkmers_set; } cmd_mem_args;
#define CMD_MEM_ARGS_INIT {DEFAULT_MEM, 0, false, false}
void cmd_mem_set_memory(cmd_mem_args *m, const char *usage, const char *arg);
void cmd_mem_set_nkmers(cmd_mem_args *m, const char *usage, const char *arg);
void cmd_threads_arg(unsigned *nthreads, const char *usage, const char *cmd, const char *arg);
/* graph_files_open: the input graphs, each at the running colour offset; ncols = colours they load into */
typedef struct { ctx_reader *files; size_t n, ncols, max_kmers, sum_kmers; } graph_files;
void graph_files_open(char **paths, size_t n, const char *usage, graph_files *set);
void graph_files_flatten(graph_files *set); /* every colour of every file into colour 0 */
void graph_files_close(graph_files *set);
col_info *graph_files_merge_headers(const graph_files *set, size_t ncols); /* col_info[ncols]: the output header */
void col_infos_free(col_info *cols, size_t ncols);
/* the table in HBM: size it from -m / -n (NULL, or why it cannot be: the caller dies, after any cleaning up of its
 * own), report it, create it (NULL, or the refusal of a machine without a device), report what was allocated */
const char *table_plan_for_args(const cmd_mem_args *m, size_t bits_per_kmer, int64_t nkmers, table_plan *plan);
void table_plan_status(const table_plan *plan); /* "[memory] graph: ..." */
const char *graph_table_create(struct mcx_graph **g, const table_plan *plan, size_t kmer_size, size_t ncols, unsigned device);
void hasht_status(struct mcx_graph *g); /* "[hasht] Allocated table in HBM ..." */
/* graph_load: the records of an opened file into the table, colour filter[i].from into filter[i].into; dies on a short
 * tail or an oversized k-mer, warns when the header's k-mer count is off, ends with "[GReader] Loaded ..." */
typedef struct {
  int into_all;       /* >= 0: every colour goes into this one, whatever the filter says */
  uint32_t rec_flags; /* MCX_RECORDS_* */
  bool warn_covg;     /* warn once each about a k-mer without coverage and one with edges but no coverage */
  unsigned char *buf; /* the caller's chunk buffer of buf_bytes; NULL: 64 MiB of the loader's own */
  size_t buf_bytes;
} graph_load_opts;
void graph_load(struct mcx_graph *g, ctx_reader *r, const graph_load_opts *opts); /* opts NULL: {-1, 0, false, NULL, 0} */
void ctx_load_graph_file(struct mcx_graph *g, ctx_reader *r); /* "[GReader] N kmers, S filesize", then graph_load */
/* header, every record of the table, the "Dumped ..." line; "-" is stdout */
void ctx_write_graph(struct mcx_graph *g, const char *out_path, size_t kmer_size, size_t ncols, const col_info *cols, bool sort_kmers);
void ctx_dumped_status(uint64_t nkmers, size_t kmer_size, size_t ncols, size_t hdr_bytes, const char *out_path);

/* ---- the JSON header of a .ctp file as text, and its body in pieces of whole k-mer blocks (ctp_hdr.c) ---- */
struct gzFile_s;
void ctp_put_str(struct gzFile_s *gz, const char *s); /* a JSON string with its quotes */
void ctp_hex_key(char *out, size_t n);                /* hex_rand_str: n hex digits and a NUL */
typedef struct { char *b; size_t len, cap; } ctp_str; /* a growing string, {NULL, 0, 0} to begin with */
void ctp_str_add(ctp_str *s, const char *p, size_t n);
size_t ctp_hdr_span(const char *buf, size_t n); /* bytes of the leading object; 0: not ended yet; (size_t)-1: no object */
bool ctp_json_member(const char *obj, const char *obj_end, const char *key, const char **vbeg, const char **vend);
bool ctp_hdr_number(const char *hdr, size_t n, const char *k1, const char *k2, uint64_t *out);
void ctp_hdr_command(ctp_str *s, const char *cmd_key, int argc, char **argv, const char *out_path, const char *file_key, const char *prev_key);
bool ctp_hdr_first_command_key(const char *hdr, size_t n, char *key, size_t keylen);
char *ctp_hdr_edit(const char *hdr, size_t n, const char *file_key, const char *command, uint64_t nkmers, uint64_t npaths, uint64_t nbytes,
                   size_t *out_len, const char **why);
size_t ctp_cut(const char *buf, size_t n);
/* ---- the header `pjoin` writes, merged from its inputs' headers as text (ctp_merge.c) ---- */
bool ctp_hdr_sample(const char *hdr, size_t n, size_t colour, const char **b, const char **e); /* the JSON string as it stands */
typedef struct { uint64_t *len, *cnt; size_t n, cap; } ctp_hist; /* ascending lengths, {NULL, NULL, 0, 0} to begin with */
void ctp_hist_add(ctp_hist *h, uint64_t len, uint64_t count);
void ctp_hist_free(ctp_hist *h);
bool ctp_hdr_hist_add(const char *hdr, size_t n, size_t colour, ctp_hist *h);
bool ctp_hdr_command_at(const char *hdr, size_t n, size_t i, const char **b, const char **e, const char **kb, const char **ke);
typedef struct { const char *hdr; size_t len; const col_filter *filter; size_t nfilter; const char *path; } ctp_merge_input;
const char *ctp_merge_header(ctp_str *out, const ctp_merge_input *in, size_t nin, size_t kmer_size, size_t out_ncols, const char *file_key, const char *command,
                             uint64_t nkmers, uint64_t npaths, uint64_t nbytes, char *err, size_t errlen);
typedef int (*ctp_read_fn)(void *ctx, void *dst, unsigned n); /* as gzread: bytes read, 0 at the end, < 0 on failure */
typedef char *(*ctp_grow_fn)(void *ctx, size_t bytes);        /* a new buffer of `bytes`; the old one is gone */
typedef struct {
  char *buf;
  size_t cap, fill, taken;
  bool eof;
  ctp_read_fn rd;
  ctp_grow_fn grow;
  void *rd_ctx, *grow_ctx;
} ctp_pieces;
void ctp_pieces_init(ctp_pieces *p, char *buf, size_t cap, ctp_read_fn rd, void *rd_ctx, ctp_grow_fn grow, void *grow_ctx);
void ctp_pieces_preload(ctp_pieces *p, const char *data, size_t n);
long long ctp_pieces_next(ctp_pieces *p);

/* ---- commands ---- */
int ctx_build(int argc, char **argv);
int ctx_sort(int argc, char **argv);
int ctx_index(int argc, char **argv);
int ctx_infer_edges(int argc, char **argv); /* src/commands/ctx_infer_edges.c */
int ctx_clean(int argc, char **argv);       /* src/commands/ctx_clean.c */
int ctx_pop_bubbles(int argc, char **argv); /* src/commands/ctx_pop_bubbles.c */
int ctx_subgraph(int argc, char **argv);    /* src/commands/ctx_subgraph.c */
int ctx_unitigs(int argc, char **argv);     /* src/commands/ctx_unitigs.c */
int ctx_reads(int argc, char **argv);       /* src/commands/ctx_reads.c */
int ctx_coverage(int argc, char **argv);    /* src/commands/ctx_coverage.c */
int ctx_correct(int argc, char **argv);     /* src/commands/ctx_correct.c */
int ctx_thread(int argc, char **argv);      /* src/commands/ctx_thread.c */
int ctx_join(int argc, char **argv);        /* src/commands/ctx_join.c */
int ctx_links(int argc, char **argv);       /* src/commands/ctx_links.c */
int ctx_pjoin(int argc, char **argv);       /* src/commands/ctx_pjoin.c */
int ctx_contigs(int argc, char **argv);     /* src/commands/ctx_contigs.c */
int ctx_bubbles(int argc, char **argv);     /* src/commands/ctx_bubbles.c */
int ctx_breakpoints(int argc, char **argv); /* src/commands/ctx_breakpoints.c */
int ctx_hashtest(int argc, char **argv);    /* src/commands/ctx_exp_hashtest.c */

/* ---- sequence output of `reads` (src/basic/seqout.{h,c}): <O>.fq.gz / .fa.gz / .txt.gz, for a paired task also
 * <O>.1.* and <O>.2.*; files are created with O_EXCL unless `force`, directories as needed (seq_out.c) ---- */
typedef struct seq_out seq_out;
/* NULL on failure, after "Output file already exists: <path>" or "Cannot create file: ..." and with nothing of it left */
seq_out *seq_out_open(const char *out_base, seq_fmt fmt, bool is_pe, bool force);
/* read i of the batch into the unpaired file (which = 0) or into <O>.1 / <O>.2 (which = 1 / 2) */
void seq_out_print(seq_out *o, int which, const read_batch *b, size_t i);
/* the same from parts: the name with `extra` (or NULL) behind it, a sequence of n bases, its qualities (or NULL); a
 * quality byte of 0, and every one of a sequence without qualities, is written as fq_zero */
void seq_out_print_parts(seq_out *o, int which, const char *name, size_t nlen, const char *extra, size_t elen, const uint8_t *seq, size_t n,
                         const uint8_t *qual, char fq_zero);
void seq_out_close(seq_out *o, bool rm); /* rm: delete the files as well */

/* ---- the batch loop of the commands that take --seq / --seq2 / --seqi tasks (cmd_reads.c): the reads of every task in
 * order, batch by batch with the pairs marked, handed to `process` in input order; with more than one thread a reader
 * parses batch n + 1 while batch n is processed (AsyncIOInput + asyncio_run_pool) ---- */
typedef struct {
  int kind; /* '1', '2' or 'i' */
  seq_in *f1, *f2;
  char *out_base;
  seq_out *out;
  size_t printed;
} reads_task;
typedef struct {
  read_batch b;
  uint8_t *mate; /* [nreads]: 1 = read i and read i + 1 are a pair */
  size_t task;
} reads_work;
typedef struct reads_run reads_run;
struct reads_run {
  reads_task *tasks;
  size_t ntasks;
  bool want_quals;
  void (*process)(reads_run *R, reads_work *w); /* the consumer; the batch is freed behind it */
  void *user;
  /* queue of one batch between the two threads */
  bool threaded, done;
  pthread_mutex_t mu;
  pthread_cond_t cv;
  reads_work *slot;
};
/* asyncio_task_parse: <in>:<O> or <in1>:<in2>:<O>; opens the inputs, dies on a failure */
void reads_task_parse(reads_task *t, int c, const char *arg);
void reads_run_tasks(reads_run *R, unsigned nthreads);

#endif
