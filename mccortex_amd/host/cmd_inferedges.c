/* cmd_inferedges.c -- `mccortex<K> inferedges` (src/commands/ctx_infer_edges.c): same options, messages
 * and output.  The graph is loaded into the device table (mcx_graph_add_records) and every record is
 * then checked against it on the MI355X (mcx_graph_infer_edges: infer_kmer_edges, src/tools/infer_edges.c).
 * A file is read twice, in chunks, so graphs larger than host memory work: once for the load, once for
 * the inference pass, which writes to -o or, without -o, rewrites in place the chunks that changed. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <fcntl.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

#define CHUNK_BYTES (64u << 20)  /* host records per read */

static const char inferedges_usage[] =
"usage: " CMD_NAME " inferedges [options] <pop.ctx>\n"
"\n"
"  Infer edges adds edges between all kmers that share k-1 bases.\n"
"  By default adds all missing edges (--all). To add only edges that exist in\n"
"  at least one other sample in the population, use --pop.\n"
"  It is important that you run this step before doing read threading.\n"
"\n"
"  -h, --help            This help message\n"
"  -q, --quiet           Silence status output normally printed to STDERR\n"
"  -f, --force           Overwrite output files\n"
"  -o, --out <out.ctx>   Save output graph file\n"
"  -m, --memory <mem>    Memory to use (e.g. 1M, 20GB)\n"
"  -n, --nkmers <N>      Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>     Number of threads to use [default: 2]\n"
"  -P, --pop             Add edges that are in the union only\n"
"  -A, --all             Add all edges [default]\n"
"  -D, --device <N>      GPU to run on [default: 0]\n"
"\n";

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},          {"out", required_argument, NULL, 'o'},
  {"force", no_argument, NULL, 'f'},         {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'},  {"threads", required_argument, NULL, 't'},
  {"pop", no_argument, NULL, 'P'},           {"all", no_argument, NULL, 'A'},
  {"device", required_argument, NULL, 'D'},  {NULL, 0, NULL, 0}};

/* futil_fopen_create (file_util.c:139-174): "-" is stdout */
static FILE *fopen_create(const char *path, bool force)
{
  if (!strcmp(path, "-")) return stdout;
  int fd = open(path, O_CREAT | (force ? 0 : O_EXCL) | O_WRONLY | O_TRUNC, 0666);
  if (fd < 0) {
    if (errno == EEXIST) die("File already exists: %s", path);
    die("Cannot write to file: %s [%s]", path, strerror(errno));
  }
  FILE *fh = fdopen(fd, "w");
  if (!fh) die("Cannot open file: %s [%s]", path, strerror(errno));
  return fh;
}

static void write_all(FILE *fh, const void *p, size_t n)
{
  if (n && fwrite(p, 1, n, fh) != n) die("Cannot write to file [%s]", strerror(errno));
}

/* export sink of the stream mode: the merged table, in the table's order */
typedef struct { unsigned char *p; size_t n, cap; } membuf;
static int membuf_sink(void *ctx, const void *recs, size_t nbytes)
{
  membuf *m = ctx;
  if (m->n + nbytes > m->cap) {
    size_t cap = m->cap ? m->cap : (1u << 20);
    while (cap < m->n + nbytes) cap *= 2;
    unsigned char *p = realloc(m->p, cap);
    if (!p) return 1;
    m->p = p; m->cap = cap;
  }
  memcpy(m->p + m->n, recs, nbytes);
  m->n += nbytes;
  return 0;
}

int ctx_infer_edges(int argc, char **argv)
{
  const char *out_path = NULL;
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, add_pop_edges = false, add_all_edges = false;
  unsigned device = 0, nthreads = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "hfo:m:n:t:PAD:", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(inferedges_usage, NULL);
      case 'f': if (force) print_usage(inferedges_usage, "%s given twice", cmd); force = true; break;
      case 'o': if (out_path) print_usage(inferedges_usage, "%s given twice", cmd); out_path = optarg; break;
      case 't': nthreads = 0; cmd_threads_arg(&nthreads, inferedges_usage, cmd, optarg); break; /* (may be repeated) */
      case 'm': cmd_mem_set_memory(&mem, inferedges_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, inferedges_usage, optarg); break;
      case 'A': add_all_edges = true; break;
      case 'P': add_pop_edges = true; break;
      case 'D': if (!parse_entire_uint(optarg, &device)) print_usage(inferedges_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " inferedges -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (!add_pop_edges && !add_all_edges) add_all_edges = true;
  if (add_pop_edges && add_all_edges) print_usage(inferedges_usage, "Please specify only one of --all --pop");
  if (optind + 1 > argc) print_usage(inferedges_usage, "Expected exactly one graph file");
  else if (optind + 1 < argc) print_usage(inferedges_usage, "Expected only one graph file. What is this: '%s'", argv[optind]);

  const char *graph_path = argv[optind];
  status("Reading graph: %s", !strcmp(graph_path, "-") ? "STDIN" : graph_path);
  if (strchr(graph_path, ':') != NULL) print_usage(inferedges_usage, "Cannot use ':' in input graph for `" CMD_NAME " inferedges`");

  /* a stream is anything that is not a regular file ("-", a pipe, <(...)): it cannot be read twice */
  struct stat st;
  const bool reading_stream = stat(graph_path, &st) != 0 || !S_ISREG(st.st_mode);
  const bool editing_file = !(out_path || reading_stream);
  if (reading_stream && strcmp(graph_path, "-") != 0 && stat(graph_path, &st) != 0)
    die("Cannot open file: %s [%s]", graph_path, strerror(errno));

  ctx_reader r;
  ctx_reader_open_mode(&r, graph_path, reading_stream ? "r" : "r+", 0, MIN_KMER_SIZE, MAX_KMER_SIZE);
  if (reading_stream) r.file_size = r.num_kmers = -1;
  if (!ctx_reader_from_direct(&r)) print_usage(inferedges_usage, "Inferedges with filter not implemented - sorry");

  FILE *fout = NULL;
  if (!editing_file) fout = fopen_create(out_path ? out_path : "-", force);
  if (fout == stdout) status("Writing to STDOUT");
  else if (fout != NULL) status("Writing to: %s", out_path);
  else status("Editing file in place: %s", graph_path);
  status("Inferring all missing %sedges", add_pop_edges ? "population " : "");

  /* ---- memory (ctx_infer_edges.c: a stream holds coverage and edges, a file one presence bit per colour) ---- */
  const size_t ncols = r.num_cols, W = r.num_words;
  const size_t bits_per_kmer = 64 * W + (reading_stream ? ncols * 8 * (4 + 1) : ncols);
  table_plan plan;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, r.num_kmers, &plan);
  if (err) die("%s", err);
  status("[memory] %zu bits per kmer", bits_per_kmer);
  table_plan_status(&plan);
  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, r.kmer_size, ncols, device))) die("%s", err);

  const size_t rec_bytes = 8 * W + 5 * ncols;
  const size_t chunk_recs = CHUNK_BYTES / rec_bytes > 0 ? CHUNK_BYTES / rec_bytes : 1;
  unsigned char *buf = malloc(chunk_recs * rec_bytes);
  if (!buf) die("Out of memory");
  /* (the path holds no filter: every colour goes into the same colour of the table) */
  graph_load(g, &r, &(graph_load_opts){-1, 0, false, buf, chunk_recs * rec_bytes});
  uint64_t nkmers = 0;
  mcx_check(mcx_graph_nkmers(g, &nkmers), "nkmers");

  if (add_pop_edges) status("Inferring edges from population...\n");
  else status("Inferring all missing edges...\n");
  const uint32_t flags = (add_pop_edges ? MCX_INFER_POP : 0) | (reading_stream ? MCX_INFER_PRESENCE_COVG : 0);
  uint64_t num_kmers_edited = 0, nmod = 0;

  if (reading_stream) {
    /* infer_edges over the merged table, then the table after the header as read */
    status("[inferedges] Processing stream");
    membuf m = {NULL, 0, 0};
    mcx_check(mcx_graph_export(g, 0, membuf_sink, &m), "export");
    mcx_check(mcx_graph_infer_edges(g, m.p, m.n / rec_bytes, (int)ncols, flags, &num_kmers_edited), "inferedges");
    ctx_write_header_raw(fout, &r);
    write_all(fout, m.p, m.n);
    free(m.p);
  } else if (fout == NULL) {
    /* inferedges_on_mmap: the chunks that changed are written back where they were read */
    status("[inferedges] Processing mmap file: %s [hdr: %zu bytes file: %zu bytes]", graph_path, r.hdr_size, (size_t)r.file_size);
    if (fseek(r.fh, (long)r.hdr_size, SEEK_SET) != 0) die("fseek failed: %s", strerror(errno));
    off_t pos = (off_t)r.hdr_size;
    for (uint64_t left = (uint64_t)r.num_kmers; left > 0;) {
      const size_t n = left < chunk_recs ? (size_t)left : chunk_recs;
      if (fread(buf, 1, n * rec_bytes, r.fh) != n * rec_bytes) die("Unexpected end of file: %s", r.path);
      mcx_check(mcx_graph_infer_edges(g, buf, n, (int)ncols, flags, &nmod), "inferedges");
      if (nmod && pwrite(fileno(r.fh), buf, n * rec_bytes, pos) != (ssize_t)(n * rec_bytes))
        die("Cannot write to file: %s [%s]", r.path, strerror(errno));
      num_kmers_edited += nmod;
      pos += (off_t)(n * rec_bytes);
      left -= n;
    }
  } else {
    /* inferedges_on_file: header as read, then every record in input order */
    status("[inferedges] Processing file: %s", graph_path);
    ctx_write_header_raw(fout, &r);
    if (fseek(r.fh, (long)r.hdr_size, SEEK_SET) != 0) die("graph_file_fseek failed: %s", strerror(errno));
    for (;;) {
      const size_t got = fread(buf, 1, chunk_recs * rec_bytes, r.fh);
      if (got == 0) break;
      const size_t n = got / rec_bytes;
      mcx_check(mcx_graph_infer_edges(g, buf, n, (int)ncols, flags, &nmod), "inferedges");
      write_all(fout, buf, n * rec_bytes);
      num_kmers_edited += nmod;
    }
  }
  if (fout != NULL) {
    if (fout != stdout) { if (fclose(fout) != 0) die("Cannot write to file: %s", out_path); }
    else fflush(fout);
  }

  char modified_str[100], kmers_str[100];
  ulong_to_str(num_kmers_edited, modified_str);
  ulong_to_str(nkmers, kmers_str);
  const double modified_rate = nkmers ? (100.0 * (double)num_kmers_edited) / (double)nkmers : 0;
  status("%s of %s (%.2f%%) nodes modified\n", modified_str, kmers_str, modified_rate);

  if (editing_file) {
    /* futil_update_timestamp */
    if (utimes(r.path, NULL) != 0) warn("Cannot update timestamp: %s [%s]", r.path, strerror(errno));
  }
  ctx_reader_close(&r);
  free(buf);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
