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

#define DEFAULT_MEM (1UL << 29) /* cmd.h:13 */

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

static void optname(char c, char *out)
{
  sprintf(out, "-%c, --Unknown", c);
  for (int i = 0; longopts[i].name; i++)
    if (longopts[i].val == c) sprintf(out, "-%c, --%s", c, longopts[i].name);
}

static void check(int rc, const char *what)
{
  if (rc == MCX_ERR_FULL) die("Hash table is full");
  if (rc != MCX_OK) die("%s: %s", what, mcx_last_error());
}

static int write_sink(void *ctx, const void *text, size_t nbytes)
{
  return fwrite(text, 1, nbytes, (FILE *)ctx) == nbytes ? 0 : 1;
}

int ctx_unitigs(int argc, char **argv)
{
  const char *out_path = NULL;
  size_t mem_to_use = DEFAULT_MEM, num_kmers_arg = 0;
  bool mem_set = false, nkmers_set = false, force = false, points = false;
  unsigned nthreads = 0, device = 0;
  int syntax = MCX_UNITIGS_FASTA;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:t:D:FgdP", longopts, NULL)) != -1) {
    optname((char)c, cmd);
    switch (c) {
      case 'h': print_usage(unitigs_usage, NULL);
      case 'f': if (force) print_usage(unitigs_usage, "%s given twice", cmd); force = true; break;
      case 'o': if (out_path) print_usage(unitigs_usage, "%s given twice", cmd); out_path = optarg; break;
      case 't':
        if (nthreads) print_usage(unitigs_usage, "%s given twice", cmd);
        if (!parse_entire_uint(optarg, &nthreads) || !nthreads) print_usage(unitigs_usage, "%s requires an int x > 0", cmd);
        break;
      case 'm':
        if (mem_set) print_usage(unitigs_usage, "-m, --memory <M> specifed more than once");
        if (!mem_to_integer(optarg, &mem_to_use) || !mem_to_use) print_usage(unitigs_usage, "Invalid memory argument: %s", optarg);
        mem_set = true; break;
      case 'n':
        if (nkmers_set) print_usage(unitigs_usage, "-n, --nkmers <N> specifed more than once");
        if (!mem_to_integer(optarg, &num_kmers_arg) || !num_kmers_arg) print_usage(unitigs_usage, "Invalid hash size: %s", optarg);
        nkmers_set = true; break;
      case 'D': if (!parse_entire_uint(optarg, &device)) print_usage(unitigs_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      /* cmd_check(!syntax, cmd): a format option after a non-FASTA one is refused, whichever it is */
      case 'F': if (syntax) print_usage(unitigs_usage, "%s given twice", cmd); syntax = MCX_UNITIGS_FASTA; break;
      case 'g': if (syntax) print_usage(unitigs_usage, "%s given twice", cmd); syntax = MCX_UNITIGS_GFA; break;
      case 'd': if (syntax) print_usage(unitigs_usage, "%s given twice", cmd); syntax = MCX_UNITIGS_DOT; break;
      case 'P': if (points) print_usage(unitigs_usage, "%s given twice", cmd); points = true; break;
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
  const size_t nfiles = (size_t)(argc - optind);
  ctx_reader *gfiles = calloc(nfiles, sizeof(ctx_reader));
  if (!gfiles) die("Out of memory");
  size_t file_ncols = 0, sum_kmers = 0;
  for (size_t i = 0; i < nfiles; i++) {
    ctx_reader_open(&gfiles[i], argv[optind + (int)i], file_ncols, MIN_KMER_SIZE, MAX_KMER_SIZE);
    if (gfiles[i].kmer_size != gfiles[0].kmer_size)
      print_usage(unitigs_usage, "Kmer sizes don't match [%u vs %u]", gfiles[0].kmer_size, gfiles[i].kmer_size);
    if (gfiles[i].into_ncols > file_ncols) file_ncols = gfiles[i].into_ncols;
    sum_kmers += gfiles[i].num_kmers < 0 ? 0 : (size_t)gfiles[i].num_kmers;
    for (size_t j = 0; j < gfiles[i].nfilter; j++) gfiles[i].filter[j].into = 0;
    gfiles[i].into_ncols = 1;
  }
  const size_t kmer_size = gfiles[0].kmer_size, W = gfiles[0].num_words;

  const size_t bits_per_kmer = W * 64 + (4 + 1) * 8 + 1;
  table_plan plan;
  char ebuf[256], s1[64], s2[64];
  const char *err = table_plan_for_build(mem_to_use, mem_set, num_kmers_arg, nkmers_set, bits_per_kmer, (int64_t)sum_kmers, &plan,
                                         ebuf, sizeof(ebuf));
  if (err) die("%s", err);
  status("[memory] graph: %s", bytes_to_str(plan.bytes, 1, s1));
  status("Output in %s format to %s\n", syntax_strs[syntax], strcmp(out_path, "-") ? out_path : "STDOUT");

  /* futil_fopen_create: an existing file is kept unless --force */
  FILE *fout = stdout;
  if (strcmp(out_path, "-") != 0) {
    if (!force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);
    fout = fopen(out_path, "w");
    if (!fout) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  }

  if (mcx_device_count() < 1) die("No MI355X / HIP device found: %s has no CPU build path", CMD_NAME);
  mcx_graph *g = NULL;
  check(mcx_graph_create(&g, (int)kmer_size, 1, plan.capacity, (int)device), "Cannot allocate graph");
  for (size_t i = 0; i < nfiles; i++) ctx_load_graph_file(g, &gfiles[i]);
  uint64_t slots = 0, tbytes = 0;
  mcx_graph_capacity(g, &slots, &tbytes);
  status("[hasht] Allocated table in HBM with %s entries, using %s", ulong_to_str(slots, s1), bytes_to_str(tbytes, 1, s2));

  if (syntax == MCX_UNITIGS_FASTA) status("Printing unitgs in FASTA using %u threads", nthreads);
  mcx_unitigs_stats st = {0, 0, 0, 0};
  check(mcx_graph_unitigs(g, syntax, points ? MCX_UNITIGS_POINTS : 0, write_sink, fout, &st), "unitigs");
  if (fflush(fout) != 0) die("Cannot write to file: %s", out_path);
  status("Dumped %s unitigs\n", ulong_to_str(st.num_unitigs, s1));
  if (fout != stdout && fclose(fout) != 0) die("Cannot write to file: %s", out_path);

  for (size_t i = 0; i < nfiles; i++) ctx_reader_close(&gfiles[i]);
  free(gfiles);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
