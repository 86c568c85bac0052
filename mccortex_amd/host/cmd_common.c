/* cmd_common.c -- what the commands share: option names and the -m/-n/-t cases (src/basic/cmd.c, src/graph/cmd_mem.c),
 * opening the input graphs (graph_files_open), sizing and creating the table in HBM, loading .ctx records into it
 * (src/graph/graphs_load.c) and writing it out (src/graph/graph_writer.c).  Calls into libmcxgpu, so it is part of the
 * mccortex<K> programs only, not of libmcxhost.so. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mcx_gpu.h"

/* cmd_get_longopt_str (cmd.c:66-84): "-k, --kmer", or "--device" for an option without a letter */
void cmd_optname(const struct option *opts, int c, char *out)
{
  sprintf(out, "-%c, --Unknown", (char)c);
  for (int i = 0; opts[i].name; i++)
    if (opts[i].val == c) {
      if (c < 256) sprintf(out, "-%c, --%s", (char)c, opts[i].name);
      else sprintf(out, "--%s", opts[i].name);
    }
}

void mcx_check(int rc, const char *what)
{
  if (rc == MCX_ERR_FULL) die("Hash table is full");
  if (rc != MCX_OK) die("%s: %s", what, mcx_last_error());
}

const char *plural(uint64_t n) { return n == 1 ? "" : "s"; }
const char *outpath(const char *p) { return strcmp(p, "-") ? p : "STDOUT"; }

int write_sink(void *ctx, const void *data, size_t nbytes)
{
  return fwrite(data, 1, nbytes, (FILE *)ctx) == nbytes ? 0 : 1;
}

/* cmd_mem_args_set_memory / cmd_mem_args_set_nkmers (cmd_mem.c:12-36) */
void cmd_mem_set_memory(cmd_mem_args *m, const char *usage, const char *arg)
{
  if (m->mem_set) print_usage(usage, "-m, --memory <M> specifed more than once");
  if (!mem_to_integer(arg, &m->mem_to_use) || !m->mem_to_use) print_usage(usage, "Invalid memory argument: %s", arg);
  m->mem_set = true;
}

void cmd_mem_set_nkmers(cmd_mem_args *m, const char *usage, const char *arg)
{
  if (m->nkmers_set) print_usage(usage, "-n, --nkmers <N> specifed more than once");
  if (!mem_to_integer(arg, &m->num_kmers) || !m->num_kmers) print_usage(usage, "Invalid hash size: %s", arg);
  m->nkmers_set = true;
}

/* cmd_check(!nthreads, cmd); nthreads = cmd_uint32_nonzero(cmd, optarg) */
void cmd_threads_arg(unsigned *nthreads, const char *usage, const char *cmd, const char *arg)
{
  if (*nthreads) print_usage(usage, "%s given twice", cmd);
  if (!parse_entire_uint(arg, nthreads) || !*nthreads) print_usage(usage, "%s requires an int x > 0", cmd);
}

/* graph_files_open: each file's colours go after those of the files before it unless its filter says otherwise */
void graph_files_open(char **paths, size_t n, const char *usage, graph_files *set)
{
  memset(set, 0, sizeof(*set));
  set->n = n;
  set->files = calloc(n, sizeof(ctx_reader));
  if (!set->files) die("Out of memory");
  for (size_t i = 0; i < n; i++) {
    ctx_reader *r = &set->files[i];
    ctx_reader_open(r, paths[i], set->ncols, MIN_KMER_SIZE, MAX_KMER_SIZE);
    if (r->kmer_size != set->files[0].kmer_size)
      print_usage(usage, "Kmer sizes don't match [%u vs %u]", set->files[0].kmer_size, r->kmer_size);
    if (r->into_ncols > set->ncols) set->ncols = r->into_ncols;
    const size_t nk = r->num_kmers < 0 ? 0 : (size_t)r->num_kmers;
    if (nk > set->max_kmers) set->max_kmers = nk;
    set->sum_kmers += nk;
  }
}

/* file_filter_flatten(.., 0) of every file: all colours go into colour 0 */
void graph_files_flatten(graph_files *set)
{
  set->ncols = 1;
  for (size_t i = 0; i < set->n; i++) {
    for (size_t j = 0; j < set->files[i].nfilter; j++) set->files[i].filter[j].into = 0;
    set->files[i].into_ncols = 1;
  }
}

void graph_files_close(graph_files *set)
{
  for (size_t i = 0; i < set->n; i++) ctx_reader_close(&set->files[i]);
  free(set->files);
  set->files = NULL;
}

/* the output header: graph_file_merge_header of every input */
col_info *graph_files_merge_headers(const graph_files *set, size_t ncols)
{
  col_info *cols = malloc(ncols * sizeof(col_info));
  if (!cols) die("Out of memory");
  for (size_t i = 0; i < ncols; i++) col_info_init(&cols[i]);
  for (size_t i = 0; i < set->n; i++) {
    const ctx_reader *r = &set->files[i];
    for (size_t j = 0; j < r->nfilter; j++) col_info_merge(&cols[r->filter[j].into], &r->ginfo[r->filter[j].from]);
  }
  return cols;
}

void col_infos_free(col_info *cols, size_t ncols)
{
  for (size_t i = 0; i < ncols; i++) col_info_free(&cols[i]);
  free(cols);
}

/* cmd_mem_args_set_memory's sizing of the table (cmd_mem.c:38-130): NULL and *plan, or why it cannot be sized */
const char *table_plan_for_args(const cmd_mem_args *m, size_t bits_per_kmer, int64_t nkmers, table_plan *plan)
{
  static char ebuf[256];
  return table_plan_for_build(m->mem_to_use, m->mem_set, m->num_kmers, m->nkmers_set, bits_per_kmer, nkmers, plan, ebuf, sizeof(ebuf));
}

void table_plan_status(const table_plan *plan)
{
  char s[64];
  status("[memory] graph: %s", bytes_to_str(plan->bytes, 1, s));
}

/* the planned table on `device`: NULL and *g, or the refusal of a machine without a device */
const char *graph_table_create(mcx_graph **g, const table_plan *plan, size_t kmer_size, size_t ncols, unsigned device)
{
  if (mcx_device_count() < 1) return "No MI355X / HIP device found: " CMD_NAME " has no CPU build path";
  mcx_check(mcx_graph_create(g, (int)kmer_size, (int)ncols, plan->capacity, (int)device), "Cannot allocate graph");
  return NULL;
}

void hasht_status(mcx_graph *g)
{
  uint64_t slots = 0, tbytes = 0;
  char s1[64], s2[64];
  mcx_graph_capacity(g, &slots, &tbytes);
  status("[hasht] Allocated table in HBM with %s entries, using %s", ulong_to_str(slots, s1), bytes_to_str(tbytes, 1, s2));
}

/* graph_load (graphs_load.c:86-214) with the hash table on the GPU: stream the records through mcx_graph_add_records */
void graph_load(mcx_graph *g, ctx_reader *r, const graph_load_opts *o)
{
  static const graph_load_opts defaults = {-1, 0, false, NULL, 0};
  if (!o) o = &defaults;
  const size_t rec_bytes = 8 * (size_t)r->num_words + 5 * (size_t)r->num_cols;
  const size_t chunk_recs = (o->buf ? o->buf_bytes : (64u << 20)) / rec_bytes;
  unsigned char *buf = o->buf ? o->buf : malloc(chunk_recs * rec_bytes);
  int32_t *from = malloc(r->nfilter * sizeof(int32_t)), *into = malloc(r->nfilter * sizeof(int32_t));
  if (!buf || !from || !into) die("Out of memory");
  for (size_t i = 0; i < r->nfilter; i++) {
    from[i] = (int32_t)r->filter[i].from;
    into[i] = o->into_all >= 0 ? o->into_all : (int32_t)r->filter[i].into;
  }
  mcx_records_stats st = {0, 0, 0, -1, -1, -1};
  bool warned_zero = !o->warn_covg, warned_edges = !o->warn_covg;
  char a[64], b[64], kstr[2 * MAX_KMER_SIZE + 8];
  for (;;) {
    const size_t got = fread(buf, 1, chunk_recs * rec_bytes, r->fh);
    if (got == 0) break;
    /* graph_file_read_raw: a partial key is "Unexpected end of file", a partial tail an _gfread error */
    if (got % rec_bytes) die("Unexpected end of file: %s", r->path);
    const uint64_t base = st.nkmers_read;
    int rc = mcx_graph_add_records(g, buf, got / rec_bytes, (int)r->num_cols, from, into, (int)r->nfilter, o->rec_flags, &st);
    if (rc != MCX_OK && st.first_oversized >= 0) die("Oversized kmer in path [kmer: %u]: %s", r->kmer_size, r->path);
    mcx_check(rc, "load graph records");
    if (st.first_zero_covg >= 0 && !warned_zero) {
      kmer_words_to_str(buf + ((uint64_t)st.first_zero_covg - base) * rec_bytes, r->kmer_size, kstr);
      warn("Kmer has zero covg in all colours [kmer: %s; path: %s]", kstr, r->path);
      warned_zero = true;
    }
    if (st.first_edges_no_covg >= 0 && !warned_edges) {
      kmer_words_to_str(buf + ((uint64_t)st.first_edges_no_covg - base) * rec_bytes, r->kmer_size, kstr);
      warn("Kmer has edges but no coverage [kmer: %s; path: %s]", kstr, r->path);
      warned_edges = true;
    }
  }
  if (r->num_kmers >= 0 && st.nkmers_read != (uint64_t)r->num_kmers)
    warn("%s kmers in the graph file than expected [exp: %zu; act: %zu; path: %s]",
         st.nkmers_read > (uint64_t)r->num_kmers ? "More" : "Fewer", (size_t)r->num_kmers, (size_t)st.nkmers_read, r->path);
  status("[GReader] Loaded %s / %s (%.2f%%) of kmers parsed", ulong_to_str(st.nkmers_loaded, a), ulong_to_str(st.nkmers_read, b),
         st.nkmers_read ? 100.0 * (double)st.nkmers_loaded / (double)st.nkmers_read : 0.0);
  if (!o->buf) free(buf);
  free(from); free(into);
}

/* one opened file's colours through its filter, as clean, popbubbles, subgraph, unitigs and reads load it */
void ctx_load_graph_file(mcx_graph *g, ctx_reader *r)
{
  char a[64], b[64];
  status("[GReader] %s kmers, %s filesize", ulong_to_str((uint64_t)(r->num_kmers < 0 ? 0 : r->num_kmers), a),
         bytes_to_str((uint64_t)(r->file_size < 0 ? 0 : r->file_size), 1, b));
  graph_load(g, r, NULL);
}

void ctx_dumped_status(uint64_t nkmers, size_t kmer_size, size_t ncols, size_t hdr_bytes, const char *out_path)
{
  char a[64], b[64];
  const size_t rec_bytes = 8 * ((2 * kmer_size + 63) / 64) + 5 * ncols;
  status("Dumped %s kmers in %zu colour%s into: %s (format version: 6; %s)", ulong_to_str(nkmers, a), ncols, plural(ncols),
         outpath(out_path), bytes_to_str(hdr_bytes + nkmers * rec_bytes, 1, b));
}

/* graph_writer_save_mkhdr: header, every record of the table, the "Dumped" line; "-" is stdout */
void ctx_write_graph(mcx_graph *g, const char *out_path, size_t kmer_size, size_t ncols, const col_info *cols, bool sort_kmers)
{
  uint64_t nk = 0;
  mcx_check(mcx_graph_nkmers(g, &nk), "nkmers");
  FILE *fout = stdout;
  if (strcmp(out_path, "-") != 0) {
    fout = fopen(out_path, "wb");
    if (!fout) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  }
  const size_t hdr = ctx_write_header(fout, (uint32_t)kmer_size, (uint32_t)ncols, cols);
  mcx_check(mcx_graph_export(g, sort_kmers ? 1 : 0, write_sink, fout), "export");
  if (fflush(fout) != 0) die("Cannot write to file: %s", out_path);
  ctx_dumped_status(nk, kmer_size, ncols, hdr, out_path);
  if (fout != stdout && fclose(fout) != 0) die("Cannot write to file: %s", out_path);
}
