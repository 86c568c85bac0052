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

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

#define DEFAULT_MEM (1UL << 29) /* cmd.h:13 */
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
  size_t mem_to_use = DEFAULT_MEM, num_kmers_arg = 0;
  bool mem_set = false, nkmers_set = false, force = false, sort_kmers = false, invert = false, grab_unitigs = false;
  bool dist_set = false;
  unsigned nthreads = 0, device = 0, use_ncols = 0, dist = 0;
  seq_in **seeds = NULL;
  size_t nseeds = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "hfo:m:n:t:N:s:1:d:vU", longopts, NULL)) != -1) {
    optname(c, cmd);
    switch (c) {
      case 'h': print_usage(subgraph_usage, NULL);
      case 'f': if (force) print_usage(subgraph_usage, "%s given twice", cmd); force = true; break;
      case 'o': if (out_path) print_usage(subgraph_usage, "%s given twice", cmd); out_path = optarg; break;
      case 't':
        if (nthreads) print_usage(subgraph_usage, "%s given twice", cmd);
        if (!parse_entire_uint(optarg, &nthreads) || !nthreads) print_usage(subgraph_usage, "%s requires an int x > 0", cmd);
        break;
      case 'm':
        if (mem_set) print_usage(subgraph_usage, "-m, --memory <M> specifed more than once");
        if (!mem_to_integer(optarg, &mem_to_use) || !mem_to_use) print_usage(subgraph_usage, "Invalid memory argument: %s", optarg);
        mem_set = true; break;
      case 'n':
        if (nkmers_set) print_usage(subgraph_usage, "-n, --nkmers <N> specifed more than once");
        if (!mem_to_integer(optarg, &num_kmers_arg) || !num_kmers_arg) print_usage(subgraph_usage, "Invalid hash size: %s", optarg);
        nkmers_set = true; break;
      case 'N':
        if (use_ncols) print_usage(subgraph_usage, "%s given twice", cmd);
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
        if (dist_set && dist) print_usage(subgraph_usage, "%s given twice", cmd); /* cmd_check(!dist, cmd) */
        if (!parse_entire_uint(optarg, &dist)) print_usage(subgraph_usage, "%s requires an int x >= 0: %s", cmd, optarg);
        dist_set = true; break;
      case 'v': if (invert) print_usage(subgraph_usage, "%s given twice", cmd); invert = true; break;
      case 'U': if (grab_unitigs) print_usage(subgraph_usage, "%s given twice", cmd); grab_unitigs = true; break;
      case OPT_SORT: if (sort_kmers) print_usage(subgraph_usage, "%s given twice", cmd); sort_kmers = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(subgraph_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " subgraph -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (nthreads == 0) nthreads = 2;
  if (nseeds == 0) print_usage(subgraph_usage, "Require at least one --seq file");
  if (optind >= argc) print_usage(subgraph_usage, "Require input graph files (.ctx)");
  if (out_path == NULL) out_path = "-";

  /* graph_files_open: each file's colours go after those of the files before it unless its filter says otherwise */
  const size_t nfiles = (size_t)(argc - optind);
  ctx_reader *gfiles = calloc(nfiles, sizeof(ctx_reader));
  if (!gfiles) die("Out of memory");
  size_t ncols = 0, max_kmers = 0, sum_kmers = 0;
  for (size_t i = 0; i < nfiles; i++) {
    ctx_reader_open(&gfiles[i], argv[optind + (int)i], ncols, MIN_KMER_SIZE, MAX_KMER_SIZE);
    if (gfiles[i].kmer_size != gfiles[0].kmer_size)
      print_usage(subgraph_usage, "Kmer sizes don't match [%u vs %u]", gfiles[0].kmer_size, gfiles[i].kmer_size);
    if (gfiles[i].into_ncols > ncols) ncols = gfiles[i].into_ncols;
    const size_t nk = gfiles[i].num_kmers < 0 ? 0 : (size_t)gfiles[i].num_kmers;
    if (nk > max_kmers) max_kmers = nk;
    sum_kmers += nk;
  }
  const size_t kmer_size = gfiles[0].kmer_size, W = gfiles[0].num_words;

  /* futil_create_output */
  if (strcmp(out_path, "-") != 0 && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);

  /* ---- memory: as `popbubbles` sizes the table for the same inputs ---- */
  const size_t bits_per_kmer = W * 64 + (4 + 1) * 8 * ncols + 2 + (sort_kmers ? 64 : 0);
  table_plan plan;
  char ebuf[256], s1[64], s2[64];
  const char *err = table_plan_for_build(mem_to_use, mem_set, num_kmers_arg, nkmers_set, bits_per_kmer, (int64_t)sum_kmers, &plan,
                                         ebuf, sizeof(ebuf));
  if (err) die("%s", err);
  status("[memory] graph: %s", bytes_to_str(plan.bytes, 1, s1));

  if (mcx_device_count() < 1) die("No MI355X / HIP device found: %s has no CPU build path", CMD_NAME);
  mcx_graph *g = NULL;
  check(mcx_graph_create(&g, (int)kmer_size, (int)ncols, plan.capacity, (int)device), "Cannot allocate graph");

  /* the output header: graph_file_merge_header of every input, then the intersection name on every colour */
  col_info *cols = malloc(ncols * sizeof(col_info));
  if (!cols) die("Out of memory");
  for (size_t i = 0; i < ncols; i++) col_info_init(&cols[i]);
  char *gname = NULL;
  size_t gname_len = 0;
  str_append(&gname, &gname_len, "subgraph:{");
  bool first = true;
  for (size_t i = 0; i < nfiles; i++)
    for (size_t j = 0; j < gfiles[i].nfilter; j++) {
      const col_info *src = &gfiles[i].ginfo[gfiles[i].filter[j].from];
      col_info_merge(&cols[gfiles[i].filter[j].into], src);
      /* graph_info_make_intersect */
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
  for (size_t i = 0; i < nfiles; i++) ctx_load_graph_file(g, &gfiles[i]);

  uint64_t slots = 0, tbytes = 0;
  mcx_graph_capacity(g, &slots, &tbytes);
  status("[hasht] Allocated table in HBM with %s entries, using %s", ulong_to_str(slots, s1), bytes_to_str(tbytes, 1, s2));

  /* subgraph_from_reads */
  const uint32_t flags = (grab_unitigs ? MCX_SUBGRAPH_UNITIGS : 0) | (invert ? MCX_SUBGRAPH_INVERT : 0);
  check(mcx_graph_subgraph_begin(g, flags), "subgraph");
  read_batch batch;
  read_batch_init(&batch, false);
  for (size_t i = 0; i < nseeds; i++) {
    while (seq_in_fill(seeds[i], &batch, SEED_BATCH_BASES) > 0 || batch.nreads) {
      check(mcx_graph_subgraph_seed_reads(g, batch.bases, batch.offsets, batch.nreads), "subgraph seeds");
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
  check(mcx_graph_subgraph_finish(g, dist, flags, &st), "subgraph");
  status("Found %s / %s (%.2f%%) seed kmers", ulong_to_str(st.num_seed_found, s1), ulong_to_str(st.num_seed_kmers, s2),
         (100.0 * (double)st.num_seed_found) / (double)st.num_seed_kmers);

  uint64_t nk = 0;
  check(mcx_graph_nkmers(g, &nk), "nkmers");
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
  free(cols); free(gfiles); free(gname);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
