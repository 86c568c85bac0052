/* cmd_coverage.c -- `mccortex<K> coverage` (src/commands/ctx_coverage.c): same options, messages and output.  The graphs
 * are loaded colour by colour into a table in HBM (not flattened: each file's colours follow those of the files before
 * it, colour filters are honoured); what the table holds for every k-mer of every read is looked up and written as text
 * on the MI355X (mcx_graph_coverage_text), batch by batch; the host adds the header lines and the sequence as read.
 *
 * Where this differs from the reference (DESIGN.md lists it): with -E but without -e the reference allocates no edges
 * and prints degrees from a buffer it never filled, here -E loads the edges as -e does and prints the real degrees; read
 * names come from this repository's own parser under the published rules of the seq_file library, as for `reads`;
 * --device picks the GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

#define READS_BATCH_BASES (32UL << 20) /* of build's order: bases per device call */

static const char coverage_usage[] =
"usage: " CMD_NAME " coverage [options] <in.ctx> [in2.ctx ..]\n"
"\n"
"  Print contig coverage\n"
"\n"
"  -h, --help           This help message\n"
"  -q, --quiet          Silence status output normally printed to STDERR\n"
"  -f, --force          Overwrite output files\n"
"  -m, --memory <mem>   Memory to use (e.g. 1M, 20GB)\n"
"  -n, --nkmers <N>     Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -e, --edges          Print edges as well. Uses hex encoding [TGCA|TGCA].\n"
"  -E, --degree         Print edge degree: 00. 01/ 02[ 10\\ 11- 12{ 20] 21} 22X\n"
"  -s, --seq <in>       Sequence file to get coverages for (can specify multiple times)\n"
"  -o, --out <out.txt>  Save output [default: STDOUT]\n"
"      --device <N>     GPU to run on [default: 0]\n"
"\n";

enum { OPT_DEVICE = 1000 };

/* (the reference's table spells the long form of -E "degrees"; getopt_long_only takes --degree as its prefix) */
static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},         {"out", required_argument, NULL, 'o'},
  {"force", no_argument, NULL, 'f'},        {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'}, {"edges", no_argument, NULL, 'e'},
  {"degrees", no_argument, NULL, 'E'},      {"seq", required_argument, NULL, '1'},
  {"seq", required_argument, NULL, 's'},    {"device", required_argument, NULL, OPT_DEVICE},
  {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(coverage_usage, "%s given twice", cmd); } while (0)

/* the text of a batch as the device hands it out */
typedef struct { char *p; size_t n, cap; } textbuf;
static int text_sink(void *ctx, const void *data, size_t nbytes)
{
  textbuf *t = ctx;
  if (t->n + nbytes > t->cap) {
    size_t cap = t->cap ? t->cap : (1u << 20);
    while (cap < t->n + nbytes) cap *= 2;
    char *p = realloc(t->p, cap);
    if (!p) return 1;
    t->p = p; t->cap = cap;
  }
  memcpy(t->p + t->n, data, nbytes);
  t->n += nbytes;
  return 0;
}

static void put(FILE *fout, const void *p, size_t n)
{
  if (n && fwrite(p, 1, n, fout) != n) die("Cannot write to output [%s]", strerror(errno));
}

int ctx_coverage(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, print_edges = false, print_degrees = false;
  const char *out_path = NULL;
  unsigned device = 0;
  seq_in **sfiles = NULL;
  size_t nsfiles = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:eE1:s:", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(coverage_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 'm': cmd_mem_set_memory(&mem, coverage_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, coverage_usage, optarg); break;
      case 'e': ONCE(print_edges); print_edges = true; break;
      case 'E': ONCE(print_degrees); print_degrees = true; break;
      case '1': case 's':
        sfiles = realloc(sfiles, (nsfiles + 1) * sizeof(*sfiles));
        if (!sfiles) die("Out of memory");
        if (!(sfiles[nsfiles++] = seq_in_open(optarg))) die("Cannot read --seq file %s", optarg);
        break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(coverage_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " coverage -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (nsfiles == 0) print_usage(coverage_usage, "Require at least one --seq file");
  if (optind == argc) print_usage(coverage_usage, "Require input graph files (.ctx)");

  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), coverage_usage, &in);
  const size_t ncols = in.ncols, kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;
  const bool want_edges = print_edges || print_degrees;

  /* kmer memory = kmer + (coverage + edges) per colour */
  const size_t bits_per_kmer = 64 * W + (32 + (want_edges ? 8 : 0)) * ncols;
  table_plan plan;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (err) die("%s", err);
  table_plan_status(&plan);

  /* futil_fopen_create: an existing file is kept unless --force */
  FILE *fout = stdout;
  if (out_path && strcmp(out_path, "-") != 0) {
    if (!force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);
    fout = fopen(out_path, "w");
    if (!fout) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  }

  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, ncols, device))) {
    if (fout != stdout) { fclose(fout); unlink(out_path); }
    die("%s", err);
  }
  for (size_t i = 0; i < in.n; i++) { ctx_load_graph_file(g, &in.files[i]); ctx_reader_close(&in.files[i]); }
  free(in.files);
  hasht_status(g);

  status("Reading coverage...");
  const uint32_t flags = (print_edges ? MCX_COVERAGE_EDGES : 0) | (print_degrees ? MCX_COVERAGE_DEGREES : 0);
  const size_t lpc = 1 + (print_edges ? 1 : 0) + (print_degrees ? 1 : 0);
  static const char *const kinds[3] = {"edges", "degree", "covgs"};
  size_t nreads = 0, cap_lines = 0;
  uint64_t *line_off = NULL;
  textbuf text = {NULL, 0, 0};
  mcx_coverage_stats stats;
  memset(&stats, 0, sizeof(stats));
  read_batch b;
  read_batch_init(&b, false);
  read_batch_keep_names(&b);
  char head[64];
  for (size_t f = 0; f < nsfiles; f++) {
    for (;;) {
      read_batch_clear(&b);
      seq_in_fill(sfiles[f], &b, READS_BATCH_BASES);
      if (!b.nreads) break;
      const size_t nlines = b.nreads * ncols * lpc;
      if (nlines + 1 > cap_lines) {
        cap_lines = 2 * (nlines + 1);
        line_off = realloc(line_off, cap_lines * sizeof(*line_off));
        if (!line_off) die("Out of memory");
      }
      text.n = 0;
      mcx_check(mcx_graph_coverage_text(g, b.bases, b.offsets, b.nreads, flags, text_sink, &text, line_off, &stats), "coverage");
      if (text.n != line_off[nlines]) die("coverage: %zu bytes of text for %llu expected", text.n, (unsigned long long)line_off[nlines]);
      for (size_t i = 0, line = 0; i < b.nreads; i++) {
        const char *name = b.names + b.name_off[i];
        const size_t name_len = (size_t)(b.name_off[i + 1] - b.name_off[i]);
        fputc('>', fout); put(fout, name, name_len); fputc('\n', fout);
        put(fout, b.bases + b.offsets[i], (size_t)(b.offsets[i + 1] - b.offsets[i])); fputc('\n', fout);
        for (size_t col = 0; col < ncols; col++)
          for (int kind = 0; kind < 3; kind++) {
            if ((kind == 0 && !print_edges) || (kind == 1 && !print_degrees)) continue;
            fputc('>', fout); put(fout, name, name_len);
            put(fout, head, (size_t)snprintf(head, sizeof(head), "_c%zu_%s\n", col, kinds[kind]));
            put(fout, text.p + line_off[line], (size_t)(line_off[line + 1] - line_off[line]));
            line++;
          }
      }
      nreads += b.nreads;
    }
    seq_in_close(sfiles[f]);
  }
  char nstr[64];
  status("Printed graph coverage for %s reads", ulong_to_str(nreads, nstr));

  read_batch_free(&b);
  free(line_off);
  free(text.p);
  free(sfiles);
  if (fflush(fout) != 0) die("Cannot write to file: %s", outpath(out_path ? out_path : "-"));
  if (fout != stdout && fclose(fout) != 0) die("Cannot write to file: %s", out_path);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
