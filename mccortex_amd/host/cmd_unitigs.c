/* cmd_unitigs.c -- `mccortex<K> unitigs` (src/commands/ctx_unitigs.c): same options, messages and formats.  The
 * graphs are loaded into a one-colour device table as `clean` loads them (every file flattened into colour 0); the
 * unitigs are found, ordered and spelled on the MI355X (mcx_graph_unitigs) and the text arrives here in chunks.
 * The output is deterministic where the reference's is not: include/mcx_gpu.h states the contract. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

static const char unitigs_usage[] =
"usage: " CMD_NAME " unitigs [options] <in.ctx> [<in2.ctx> ...]\n"
"\n"
"  Print unitigs with k-1 bases of overlap.\n"
"\n"
"  -h, --help            This help message\n"
"  -q, --quiet           Silence status output normally printed to STDERR\n"
"  -f, --force           Overwrite output files\n"
"  -o, --out <out.txt>   Save output graph file [default: STDOUT]\n"
"  -m, --memory <mem>    Memory to use\n"
"  -n, --nkmers <kmers>  Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>     Number of threads to use [default: 2]\n"
"  -D, --device <N>      GPU to run on [default: 0]\n"
"  -F, --fasta           Print in FASTA format (default)\n"
"  -g, --gfa             Print in Graphical Fragment Assembly (GFA) format\n"
"  -d, --dot             Print in graphviz (DOT) format\n"
"  -P, --points          Used with --dot, print contigs as points\n"
"\n"
"  e.g. " CMD_NAME " unitigs --dot in.ctx | dot -Tpdf > in.pdf\n"
"\n";

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},         {"out", required_argument, NULL, 'o'},
  {"force", no_argument, NULL, 'f'},        {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'}, {"threads", required_argument, NULL, 't'},
  {"device", required_argument, NULL, 'D'}, {"fasta", no_argument, NULL, 'F'},
  {"gfa", no_argument, NULL, 'g'},          {"dot", no_argument, NULL, 'd'},
  {"points", no_argument, NULL, 'P'},       {NULL, 0, NULL, 0}};

static const char *syntax_strs[3] = {"FASTA", "GFA", "DOT (Graphviz)"};

/* -x given twice */
#define ONCE(seen) do { if (seen) print_usage(unitigs_usage, "%s given twice", cmd); } while (0)

int ctx_unitigs(int argc, char **argv)
{
  const char *out_path = NULL;
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, points = false;
  unsigned nthreads = 0, device = 0;
  int syntax = MCX_UNITIGS_FASTA;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:t:D:FgdP", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(unitigs_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 't': cmd_threads_arg(&nthreads, unitigs_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, unitigs_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, unitigs_usage, optarg); break;
      case 'D': if (!parse_entire_uint(optarg, &device)) print_usage(unitigs_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      /* cmd_check(!syntax, cmd): a format option after a non-FASTA one is refused, whichever it is */
      case 'F': ONCE(syntax); syntax = MCX_UNITIGS_FASTA; break;
      case 'g': ONCE(syntax); syntax = MCX_UNITIGS_GFA; break;
      case 'd': ONCE(syntax); syntax = MCX_UNITIGS_DOT; break;
      case 'P': ONCE(points); points = true; break;
      case ':': case '?': die("`" CMD_NAME " unitigs -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (points && syntax == MCX_UNITIGS_FASTA) print_usage(unitigs_usage, "--point is only for use with --dot");
  if (out_path == NULL) out_path = "-";
  if (nthreads == 0) nthreads = 2; /* accepted, not used: the device does the work */
  if (optind >= argc) print_usage(unitigs_usage, NULL);
  if (points && syntax != MCX_UNITIGS_DOT) print_usage(unitigs_usage, "--points only valid with --graphviz / --dot");

  /* graph_files_open, then file_filter_flatten(.., 0): every colour of every file goes into colour 0 */
  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), unitigs_usage, &in);
  graph_files_flatten(&in);
  const size_t kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;

  const size_t bits_per_kmer = W * 64 + (4 + 1) * 8 + 1;
  table_plan plan;
  char s1[64];
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (err) die("%s", err);
  table_plan_status(&plan);
  status("Output in %s format to %s\n", syntax_strs[syntax], outpath(out_path));

  /* futil_fopen_create: an existing file is kept unless --force */
  FILE *fout = stdout;
  if (strcmp(out_path, "-") != 0) {
    if (!force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);
    fout = fopen(out_path, "w");
    if (!fout) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  }

  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, 1, device))) die("%s", err);
  for (size_t i = 0; i < in.n; i++) ctx_load_graph_file(g, &in.files[i]);
  hasht_status(g);

  if (syntax == MCX_UNITIGS_FASTA) status("Printing unitgs in FASTA using %u threads", nthreads);
  mcx_unitigs_stats st = {0, 0, 0, 0};
  mcx_check(mcx_graph_unitigs(g, syntax, points ? MCX_UNITIGS_POINTS : 0, write_sink, fout, &st), "unitigs");
  if (fflush(fout) != 0) die("Cannot write to file: %s", out_path);
  status("Dumped %s unitigs\n", ulong_to_str(st.num_unitigs, s1));
  if (fout != stdout && fclose(fout) != 0) die("Cannot write to file: %s", out_path);

  graph_files_close(&in);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
