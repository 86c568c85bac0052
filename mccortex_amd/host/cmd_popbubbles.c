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

#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

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

/* -x given twice */
#define ONCE(seen) do { if (seen) print_usage(pop_usage, "%s given twice", cmd); } while (0)

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
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, sort_kmers = false;
  int32_t max_covg = -1, max_klen = -1, max_kdiff = -1; /* <= 0, <= 0, < 0: ignore */
  unsigned nthreads = 0, device = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:m:n:t:fC:L:D:S", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(pop_usage, NULL);
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 'f': ONCE(force); force = true; break;
      case 't': cmd_threads_arg(&nthreads, pop_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, pop_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, pop_usage, optarg); break;
      case 'C': ONCE(max_covg >= 0); max_covg = limit_arg(cmd, optarg); break;
      case 'L': ONCE(max_klen >= 0); max_klen = limit_arg(cmd, optarg); break;
      case 'D': ONCE(max_kdiff >= 0); max_kdiff = limit_arg(cmd, optarg); break;
      case 'S': ONCE(sort_kmers); sort_kmers = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(pop_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " popbubbles -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (out_path == NULL) out_path = "-";
  if (nthreads == 0) nthreads = 2;
  if (optind >= argc) print_usage(pop_usage, "Require input graph files (.ctx)");

  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), pop_usage, &in);
  const size_t ncols = in.ncols, kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;

  /* futil_create_output */
  if (strcmp(out_path, "-") != 0 && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);

  /* ---- memory: as `clean` sizes the table for the same inputs ---- */
  const size_t bits_per_kmer = W * 64 + (4 + 1) * 8 * ncols + 2 + (sort_kmers ? 64 : 0);
  table_plan plan;
  char s1[64], s2[64], s3[64];
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (err) die("%s", err);
  table_plan_status(&plan);
  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, ncols, device))) die("%s", err);

  col_info *cols = graph_files_merge_headers(&in, ncols);
  for (size_t i = 0; i < in.n; i++) ctx_load_graph_file(g, &in.files[i]);
  hasht_status(g);

  status("Popping bubbles...");
  status("[pop_bubbles] Popping bubbles...");
  if (max_covg > 0) status("[pop_bubbles]   where branch coverage <= %i", max_covg);
  if (max_klen > 0) status("[pop_bubbles]   where branch length <= %i", max_klen);
  if (max_kdiff >= 0) status("[pop_bubbles]   where branch length diff < %i", max_kdiff);
  mcx_pop_stats ps;
  mcx_check(mcx_graph_pop_bubbles(g, max_covg, max_klen, max_kdiff, &ps), "popbubbles");
  status("Popped %s bubbles", ulong_to_str(ps.num_popped, s1));
  status("Removing nodes...");
  uint64_t nk = 0;
  mcx_check(mcx_graph_nkmers(g, &nk), "nkmers");
  status("Number of kmers %s -> %s (-%s)", ulong_to_str(ps.nkmers_before, s1), ulong_to_str(nk, s2),
         ulong_to_str(ps.nkmers_before - nk, s3));

  status("Saving to: %s\n", out_path);
  ctx_write_graph(g, out_path, kmer_size, ncols, cols, sort_kmers);

  col_infos_free(cols, ncols);
  graph_files_close(&in);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
