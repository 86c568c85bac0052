/* cmd_subgraph.c -- `mccortex<K> subgraph` (src/commands/ctx_subgraph.c, src/tools/subgraph.c): same options,
 * defaults, messages and output.  The graphs are loaded into the device table as `clean` loads them, every colour
 * at once; the seed lookup, the breadth-first extension and the prune run on the MI355X (mcx_graph_subgraph_*).
 *
 * Where this differs from the reference (DESIGN.md lists it): -N/--ncols is parsed and otherwise ignored, since
 * every colour is resident in HBM there is no reload pass and no "Need to use --ncols" error for stdout; there is no
 * "[memory] fringe nodes" line, the queue holds one entry per k-mer and cannot run out; "Found ... seed kmers" gives
 * the true number of distinct seed k-mers found also with --dist 0; a neighbour that is not in the graph is passed
 * over.  The header is the merge of the inputs' headers with the intersection name subgraph:{...} on every colour
 * (graph_writer_merge_mkhdr with intersect_gname). */
#define _GNU_SOURCE
#include "host.h"

#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

#define SEED_BATCH_BASES (32UL << 20)

static const char subgraph_usage[] =
"usage: " CMD_NAME " subgraph [options] <in.ctx>[:cols] [in2.ctx ...]\n"
"\n"
"  Loads graphs (in.ctx) and dumps a graph (out.ctx) that contains all kmers within\n"
"  <dist> edges of kmers in <seeds.fa>.  Maintains number of colours / covgs etc.\n"
"  Seed files are read once and may be pipes ('-' is stdin).\n"
"\n"
"  -h, --help            This help message\n"
"  -q, --quiet           Silence status output normally printed to STDERR\n"
"  -f, --force           Overwrite output files\n"
"  -o, --out <out.ctx>   Save output graph file [required]\n"
"  -m, --memory <mem>    Memory to use\n"
"  -n, --nkmers <kmers>  Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>     Number of threads to use [default: 2]\n"
"  -N, --ncols <c>       Accepted and ignored: all colours are loaded at once\n"
"  -1, --seq <seed.fa>   Read in a seed file [require at least one]\n"
"  -s, --seed <seed.fa>  Same as --seq\n"
"  -d, --dist <N>        Number of kmers to extend by [default: 0]\n"
"  -v, --invert          Dump kmers not in subgraph\n"
"  -U, --unitigs         Grab entire runs of kmers that are touched by a read\n"
"      --sort            Output a graph file ordered by kmer\n"
"      --device <N>      GPU to run on [default: 0]\n"
"\n";

enum { OPT_DEVICE = 1000, OPT_SORT };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},           {"force", no_argument, NULL, 'f'},
  {"out", required_argument, NULL, 'o'},      {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'},   {"threads", required_argument, NULL, 't'},
  {"ncols", required_argument, NULL, 'N'},    {"seed", required_argument, NULL, 's'},
  {"seq", required_argument, NULL, '1'},      {"dist", required_argument, NULL, 'd'},
  {"invert", no_argument, NULL, 'v'},         {"unitigs", no_argument, NULL, 'U'},
  {"sort", no_argument, NULL, OPT_SORT},      {"device", required_argument, NULL, OPT_DEVICE},
  {NULL, 0, NULL, 0}};

/* -x given twice */
#define ONCE(seen) do { if (seen) print_usage(subgraph_usage, "%s given twice", cmd); } while (0)

static void str_append(char **s, size_t *len, const char *add)
{
  const size_t n = strlen(add);
  *s = realloc(*s, *len + n + 1);
  if (!*s) die("Out of memory");
  memcpy(*s + *len, add, n + 1);
  *len += n;
}

int ctx_subgraph(int argc, char **argv)
{
  const char *out_path = NULL;
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, sort_kmers = false, invert = false, grab_unitigs = false;
  bool dist_set = false;
  unsigned nthreads = 0, device = 0, use_ncols = 0, dist = 0;
  seq_in **seeds = NULL;
  size_t nseeds = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "hfo:m:n:t:N:s:1:d:vU", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(subgraph_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 't': cmd_threads_arg(&nthreads, subgraph_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, subgraph_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, subgraph_usage, optarg); break;
      case 'N':
        ONCE(use_ncols);
        if (!parse_entire_uint(optarg, &use_ncols) || !use_ncols) print_usage(subgraph_usage, "%s requires an int x > 0", cmd);
        break;
      case '1':
      case 's': {
        seq_in *in = seq_in_open(optarg);
        if (!in) die("Cannot read --seq file %s", optarg);
        seeds = realloc(seeds, (nseeds + 1) * sizeof(*seeds));
        if (!seeds) die("Out of memory");
        seeds[nseeds++] = in;
        break;
      }
      case 'd':
        ONCE(dist_set && dist); /* cmd_check(!dist, cmd) */
        if (!parse_entire_uint(optarg, &dist)) print_usage(subgraph_usage, "%s requires an int x >= 0: %s", cmd, optarg);
        dist_set = true; break;
      case 'v': ONCE(invert); invert = true; break;
      case 'U': ONCE(grab_unitigs); grab_unitigs = true; break;
      case OPT_SORT: ONCE(sort_kmers); sort_kmers = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(subgraph_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " subgraph -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (nthreads == 0) nthreads = 2;
  if (nseeds == 0) print_usage(subgraph_usage, "Require at least one --seq file");
  if (optind >= argc) print_usage(subgraph_usage, "Require input graph files (.ctx)");
  if (out_path == NULL) out_path = "-";

  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), subgraph_usage, &in);
  const size_t ncols = in.ncols, kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;

  /* futil_create_output */
  if (strcmp(out_path, "-") != 0 && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);

  /* ---- memory: as `popbubbles` sizes the table for the same inputs ---- */
  const size_t bits_per_kmer = W * 64 + (4 + 1) * 8 * ncols + 2 + (sort_kmers ? 64 : 0);
  table_plan plan;
  char s1[64], s2[64];
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (err) die("%s", err);
  table_plan_status(&plan);
  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, ncols, device))) die("%s", err);

  /* the output header: graph_file_merge_header of every input, then the intersection name on every colour */
  col_info *cols = graph_files_merge_headers(&in, ncols);
  char *gname = NULL;
  size_t gname_len = 0;
  str_append(&gname, &gname_len, "subgraph:{");
  bool first = true;
  for (size_t i = 0; i < in.n; i++)
    for (size_t j = 0; j < in.files[i].nfilter; j++) { /* graph_info_make_intersect */
      const col_info *src = &in.files[i].ginfo[in.files[i].filter[j].from];
      if (!first) str_append(&gname, &gname_len, ",");
      first = false;
      str_append(&gname, &gname_len, src->name);
      if (src->cleaning.is_graph_intersection) {
        str_append(&gname, &gname_len, ",");
        str_append(&gname, &gname_len, src->cleaning.intersection_name);
      }
    }
  str_append(&gname, &gname_len, "}");
  for (size_t i = 0; i < ncols; i++) { /* graph_info_append_intersect */
    err_cleaning *ec = &cols[i].cleaning;
    if (!ec->is_graph_intersection) {
      free(ec->intersection_name);
      ec->intersection_name = strdup(gname);
      if (!ec->intersection_name) die("Out of memory");
    } else {
      size_t len = strlen(ec->intersection_name);
      str_append(&ec->intersection_name, &len, ",");
      str_append(&ec->intersection_name, &len, gname);
    }
    ec->is_graph_intersection = 1;
  }
  for (size_t i = 0; i < in.n; i++) ctx_load_graph_file(g, &in.files[i]);
  hasht_status(g);

  /* subgraph_from_reads */
  const uint32_t flags = (grab_unitigs ? MCX_SUBGRAPH_UNITIGS : 0) | (invert ? MCX_SUBGRAPH_INVERT : 0);
  mcx_check(mcx_graph_subgraph_begin(g, flags), "subgraph");
  read_batch batch;
  read_batch_init(&batch, false);
  for (size_t i = 0; i < nseeds; i++) {
    while (seq_in_fill(seeds[i], &batch, SEED_BATCH_BASES) > 0 || batch.nreads) {
      mcx_check(mcx_graph_subgraph_seed_reads(g, batch.bases, batch.offsets, batch.nreads), "subgraph seeds");
      read_batch_clear(&batch);
    }
    seq_in_close(seeds[i]);
  }
  read_batch_free(&batch);
  free(seeds);
  /* the device extends, inverts and prunes in one call: its lines come before it, so a long run shows what it is
   * doing; the "Found" line needs the call's count and follows it (the reference prints it first) */
  if (dist > 0) status("Extending subgraph by %s kmers\n", ulong_to_str(dist, s1));
  if (invert) status("Inverting selection...");
  status("Pruning untouched nodes...");
  mcx_subgraph_stats st;
  mcx_check(mcx_graph_subgraph_finish(g, dist, flags, &st), "subgraph");
  status("Found %s / %s (%.2f%%) seed kmers", ulong_to_str(st.num_seed_found, s1), ulong_to_str(st.num_seed_kmers, s2),
         (100.0 * (double)st.num_seed_found) / (double)st.num_seed_kmers);

  ctx_write_graph(g, out_path, kmer_size, ncols, cols, sort_kmers);

  col_infos_free(cols, ncols);
  graph_files_close(&in);
  free(gname);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
