/* cmd_popbubbles.c -- `mccortex<K> popbubbles` (src/commands/ctx_pop_bubbles.c, src/tools/pop_bubbles.c): same
 * options, defaults, messages and output.  The graphs are loaded into the device table as `clean` loads them; the
 * parallel unitigs, the visiting order and the prune run on the MI355X (mcx_graph_pop_bubbles).
 *
 * Given one file, the reference flattens it to one colour, pops, then reads the file again and writes each colour's
 * edges ANDed with the popped union edges.  Pruning removes an edge from every colour at once, so that gives the
 * same records as loading every colour and pruning per colour -- which is what happens here, for one file or many.
 * The header is the merge of the inputs' headers (graph_writer_stream_mkhdr / graph_writer_save_mkhdr): popping
 * sets no cleaning flag. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

#define DEFAULT_MEM (1UL << 29) /* cmd.h:13 */

static const char pop_usage[] =
"usage: " CMD_NAME " popbubbles [options] <in.ctx> [in2.ctx ...]\n"
"\n"
"  Pop bubbles in the graph. All graphs are loaded and treated as one colour\n"
"  for bubble popping. Output is a multicolour graph.\n"
"\n"
"  -h, --help            This help message\n"
"  -q, --quiet           Silence status output normally printed to STDERR\n"
"  -f, --force           Overwrite output files\n"
"  -o, --out <out.ctx>   Output file [required]\n"
"  -m, --memory <mem>    Memory to use\n"
"  -n, --nkmers <kmers>  Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>     Number of threads to use [default: 2]\n"
"  -C, --max-covg <C>    Only remove branches whose mean coverage is less than <C>\n"
"  -L, --max-len <L>     Only remove branches whose lengths are less than <L> kmers\n"
"  -D, --max-diff <D>    Only pop bubbles whose branch lengths are within <D> kmers\n"
"  -S, --sort            Output a graph file ordered by kmer\n"
"      --device <N>      GPU to run on [default: 0]\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},           {"out", required_argument, NULL, 'o'},
  {"memory", required_argument, NULL, 'm'},   {"nkmers", required_argument, NULL, 'n'},
  {"threads", required_argument, NULL, 't'},  {"force", no_argument, NULL, 'f'},
  {"max-covg", required_argument, NULL, 'C'}, {"max-len", required_argument, NULL, 'L'},
  {"max-diff", required_argument, NULL, 'D'}, {"sort", no_argument, NULL, 'S'},
  {"device", required_argument, NULL, OPT_DEVICE}, {NULL, 0, NULL, 0}};

static void optname(int c, char *out)
{
  sprintf(out, "-%c, --Unknown", (char)c);
  for (int i = 0; longopts[i].name; i++)
    if (longopts[i].val == c) {
      if (c < 256) sprintf(out, "-%c, --%s", (char)c, longopts[i].name);
      else sprintf(out, "--%s", longopts[i].name);
    }
}

static void check(int rc, const char *what)
{
  if (rc == MCX_ERR_FULL) die("Hash table is full");
  if (rc != MCX_OK) die("%s: %s", what, mcx_last_error());
}

static const char *plural(uint64_t n) { return n == 1 ? "" : "s"; }
static const char *outpath(const char *p) { return strcmp(p, "-") ? p : "STDOUT"; }

static int write_sink(void *ctx, const void *recs, size_t nbytes)
{
  return fwrite(recs, 1, nbytes, (FILE *)ctx) == nbytes ? 0 : 1;
}

/* cmd_uint32 into the reference's int32_t settings */
static int32_t limit_arg(const char *cmd, const char *arg)
{
  unsigned u = 0;
  if (!parse_entire_uint(arg, &u) || u > 0x7fffffffu) print_usage(pop_usage, "%s requires an int x >= 0: %s", cmd, arg);
  return (int32_t)u;
}

int ctx_pop_bubbles(int argc, char **argv)
{
  const char *out_path = NULL;
  size_t mem_to_use = DEFAULT_MEM, num_kmers_arg = 0;
  bool mem_set = false, nkmers_set = false, force = false, sort_kmers = false;
  int32_t max_covg = -1, max_klen = -1, max_kdiff = -1; /* <= 0, <= 0, < 0: ignore */
  unsigned nthreads = 0, device = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:m:n:t:fC:L:D:S", longopts, NULL)) != -1) {
    optname(c, cmd);
    switch (c) {
      case 'h': print_usage(pop_usage, NULL);
      case 'o': if (out_path) print_usage(pop_usage, "%s given twice", cmd); out_path = optarg; break;
      case 'f': if (force) print_usage(pop_usage, "%s given twice", cmd); force = true; break;
      case 't':
        if (nthreads) print_usage(pop_usage, "%s given twice", cmd);
        if (!parse_entire_uint(optarg, &nthreads) || !nthreads) print_usage(pop_usage, "%s requires an int x > 0", cmd);
        break;
      case 'm':
        if (mem_set) print_usage(pop_usage, "-m, --memory <M> specifed more than once");
        if (!mem_to_integer(optarg, &mem_to_use) || !mem_to_use) print_usage(pop_usage, "Invalid memory argument: %s", optarg);
        mem_set = true; break;
      case 'n':
        if (nkmers_set) print_usage(pop_usage, "-n, --nkmers <N> specifed more than once");
        if (!mem_to_integer(optarg, &num_kmers_arg) || !num_kmers_arg) print_usage(pop_usage, "Invalid hash size: %s", optarg);
        nkmers_set = true; break;
      case 'C': if (max_covg >= 0) print_usage(pop_usage, "%s given twice", cmd); max_covg = limit_arg(cmd, optarg); break;
      case 'L': if (max_klen >= 0) print_usage(pop_usage, "%s given twice", cmd); max_klen = limit_arg(cmd, optarg); break;
      case 'D': if (max_kdiff >= 0) print_usage(pop_usage, "%s given twice", cmd); max_kdiff = limit_arg(cmd, optarg); break;
      case 'S': if (sort_kmers) print_usage(pop_usage, "%s given twice", cmd); sort_kmers = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(pop_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " popbubbles -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (out_path == NULL) out_path = "-";
  if (nthreads == 0) nthreads = 2;
  if (optind >= argc) print_usage(pop_usage, "Require input graph files (.ctx)");

  /* graph_files_open: each file's colours go after those of the files before it unless its filter says otherwise */
  const size_t nfiles = (size_t)(argc - optind);
  ctx_reader *gfiles = calloc(nfiles, sizeof(ctx_reader));
  if (!gfiles) die("Out of memory");
  size_t ncols = 0, max_kmers = 0, sum_kmers = 0;
  for (size_t i = 0; i < nfiles; i++) {
    ctx_reader_open(&gfiles[i], argv[optind + (int)i], ncols, MIN_KMER_SIZE, MAX_KMER_SIZE);
    if (gfiles[i].kmer_size != gfiles[0].kmer_size)
      print_usage(pop_usage, "Kmer sizes don't match [%u vs %u]", gfiles[0].kmer_size, gfiles[i].kmer_size);
    if (gfiles[i].into_ncols > ncols) ncols = gfiles[i].into_ncols;
    const size_t nk = gfiles[i].num_kmers < 0 ? 0 : (size_t)gfiles[i].num_kmers;
    if (nk > max_kmers) max_kmers = nk;
    sum_kmers += nk;
  }
  const size_t kmer_size = gfiles[0].kmer_size, W = gfiles[0].num_words;

  /* futil_create_output */
  if (strcmp(out_path, "-") != 0 && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);

  /* ---- memory: as `clean` sizes the table for the same inputs ---- */
  const size_t bits_per_kmer = W * 64 + (4 + 1) * 8 * ncols + 2 + (sort_kmers ? 64 : 0);
  table_plan plan;
  char ebuf[256], s1[64], s2[64], s3[64];
  const char *err = table_plan_for_build(mem_to_use, mem_set, num_kmers_arg, nkmers_set, bits_per_kmer, (int64_t)sum_kmers, &plan,
                                         ebuf, sizeof(ebuf));
  if (err) die("%s", err);
  status("[memory] graph: %s", bytes_to_str(plan.bytes, 1, s1));

  if (mcx_device_count() < 1) die("No MI355X / HIP device found: %s has no CPU build path", CMD_NAME);
  mcx_graph *g = NULL;
  check(mcx_graph_create(&g, (int)kmer_size, (int)ncols, plan.capacity, (int)device), "Cannot allocate graph");

  /* the output header: graph_file_merge_header of every input */
  col_info *cols = malloc(ncols * sizeof(col_info));
  if (!cols) die("Out of memory");
  for (size_t i = 0; i < ncols; i++) col_info_init(&cols[i]);
  for (size_t i = 0; i < nfiles; i++)
    for (size_t j = 0; j < gfiles[i].nfilter; j++) col_info_merge(&cols[gfiles[i].filter[j].into], &gfiles[i].ginfo[gfiles[i].filter[j].from]);
  for (size_t i = 0; i < nfiles; i++) ctx_load_graph_file(g, &gfiles[i]);

  uint64_t slots = 0, tbytes = 0;
  mcx_graph_capacity(g, &slots, &tbytes);
  status("[hasht] Allocated table in HBM with %s entries, using %s", ulong_to_str(slots, s1), bytes_to_str(tbytes, 1, s2));

  status("Popping bubbles...");
  status("[pop_bubbles] Popping bubbles...");
  if (max_covg > 0) status("[pop_bubbles]   where branch coverage <= %i", max_covg);
  if (max_klen > 0) status("[pop_bubbles]   where branch length <= %i", max_klen);
  if (max_kdiff >= 0) status("[pop_bubbles]   where branch length diff < %i", max_kdiff);
  mcx_pop_stats ps;
  check(mcx_graph_pop_bubbles(g, max_covg, max_klen, max_kdiff, &ps), "popbubbles");
  status("Popped %s bubbles", ulong_to_str(ps.num_popped, s1));
  status("Removing nodes...");
  uint64_t nk = 0;
  check(mcx_graph_nkmers(g, &nk), "nkmers");
  status("Number of kmers %s -> %s (-%s)", ulong_to_str(ps.nkmers_before, s1), ulong_to_str(nk, s2),
         ulong_to_str(ps.nkmers_before - nk, s3));

  status("Saving to: %s\n", out_path);
  FILE *fout = stdout;
  if (strcmp(out_path, "-") != 0) {
    fout = fopen(out_path, "wb");
    if (!fout) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  }
  const size_t hdr = ctx_write_header(fout, (uint32_t)kmer_size, (uint32_t)ncols, cols);
  check(mcx_graph_export(g, sort_kmers ? 1 : 0, write_sink, fout), "export");
  if (fflush(fout) != 0) die("Cannot write to file: %s", out_path);
  status("Dumped %s kmers in %zu colour%s into: %s (format version: 6; %s)", ulong_to_str(nk, s1), ncols, plural(ncols),
         outpath(out_path), bytes_to_str(hdr + nk * (8 * W + 5 * ncols), 1, s2));
  if (fout != stdout && fclose(fout) != 0) die("Cannot write to file: %s", out_path);

  for (size_t i = 0; i < ncols; i++) col_info_free(&cols[i]);
  for (size_t i = 0; i < nfiles; i++) ctx_reader_close(&gfiles[i]);
  free(cols); free(gfiles);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
