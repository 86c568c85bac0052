/* cmd_join.c -- `mccortex<K> join` (src/commands/ctx_join.c, graph_writer_merge_mkhdr of src/graph/graph_writer.c): same
 * options, checks, messages, colour offsets and header.  The merge itself is a sort and a segmented reduce on the MI355X
 * (mcx_join_*): the records of every file go to HBM as they are, one pass orders them by key, one pass writes each run
 * of equal keys as one record.
 *
 * Differences from the reference:
 *   - the output is always sorted by key.  -S / --sort is accepted and only decides, with -i, whether the k-mers of
 *     the intersection that no input has are written (below); a single input is sorted too, where the reference
 *     streams it in file order;
 *   - -n / --nkmers is accepted and ignored: there is no hash table, so nothing to size and nothing that can be full;
 *   - -N / --ncols is accepted and validated with the reference's two messages but does not change the result (the
 *     reference's tests/join/Makefile asserts that of the reference as well);
 *   - -m / --memory is checked against the HBM the engine needs, which is computed from the file sizes before anything
 *     is read; inputs that do not fit are refused (joining in several passes is not implemented);
 *   - with several -i graphs a k-mer is in the intersection when every one of them has it; the reference counts loaded
 *     records, which differs only for a file that holds a k-mer twice. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

static const char join_usage[] =
"usage: " CMD_NAME " join [options] in1.ctx [[offset:]in2.ctx[:1,2,4-5] ...]\n"
"\n"
"  Merge cortex graphs.\n"
"\n"
"  -h, --help              This help message\n"
"  -q, --quiet             Silence status output normally printed to STDERR\n"
"  -f, --force             Overwrite output files\n"
"  -o, --out <out.ctx>     Output file [required]\n"
"  -m, --memory <mem>      Memory to use\n"
"  -n, --nkmers <kmers>    Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -N, --ncols <c>         How many colours to load at once [default: 1]\n"
"  -i, --intersect <a.ctx> Only load the kmers that are in graph A.ctx. Can be\n"
"                          specified multiple times. <a.ctx> is NOT merged into\n"
"                          the output file.\n"
"  -S, --sort              Output sorted graph file\n"
"      --device <N>        GPU to run on [default: 0]\n"
"\n"
"  Files can be specified with specific colours: samples.ctx:2,3\n"
"  Offset specifies where to load the first colour: 3:samples.ctx\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},           {"out", required_argument, NULL, 'o'},
  {"force", no_argument, NULL, 'f'},          {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'},   {"ncols", required_argument, NULL, 'N'},
  {"intersect", required_argument, NULL, 'i'}, {"sort", no_argument, NULL, 'S'},
  {"device", required_argument, NULL, OPT_DEVICE}, {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(join_usage, "%s given twice", cmd); } while (0)

static uint64_t reader_nkmers(const ctx_reader *r) { return r->num_kmers < 0 ? 0 : (uint64_t)r->num_kmers; }

/* graph_info_make_intersect: the sample name of header colour 0, and what it was itself intersected with */
static void make_intersect(const col_info *c, char **name)
{
  const size_t have = *name ? strlen(*name) : 0;
  const size_t add = strlen(c->name) + (c->cleaning.is_graph_intersection ? 1 + strlen(c->cleaning.intersection_name) : 0);
  char *s = realloc(*name, have + add + 2);
  if (!s) die("Out of memory");
  s[have] = '\0';
  if (have) strcat(s, ",");
  strcat(s, c->name);
  if (c->cleaning.is_graph_intersection) { strcat(s, ","); strcat(s, c->cleaning.intersection_name); }
  *name = s;
}

/* graph_info_append_intersect */
static void append_intersect(err_cleaning *ec, const char *name)
{
  if (!ec->is_graph_intersection) {
    free(ec->intersection_name);
    ec->intersection_name = strdup(name);
  } else {
    char *s = realloc(ec->intersection_name, strlen(ec->intersection_name) + strlen(name) + 2);
    if (s) { strcat(s, ","); strcat(s, name); }
    ec->intersection_name = s;
  }
  if (!ec->intersection_name) die("Out of memory");
  ec->is_graph_intersection = 1;
}

/* the records of one file through the pinned buffer into the engine; "[GReader]" lines as graph_load prints them */
static void join_load(mcx_join *j, ctx_reader *r, int source, unsigned char *buf, size_t buf_bytes)
{
  char a[64], b[64];
  status("[GReader] %s kmers, %s filesize", ulong_to_str(reader_nkmers(r), a), bytes_to_str((uint64_t)(r->file_size < 0 ? 0 : r->file_size), 1, b));
  const size_t rec_bytes = 8 * (size_t)r->num_words + 5 * (size_t)r->num_cols;
  const size_t chunk_recs = buf_bytes / rec_bytes;
  if (!chunk_recs) die("Too many colours in %s for the read buffer", r->path);
  int32_t *from = malloc(r->nfilter * sizeof(int32_t)), *into = malloc(r->nfilter * sizeof(int32_t));
  if (!from || !into) die("Out of memory");
  for (size_t i = 0; i < r->nfilter; i++) { from[i] = (int32_t)r->filter[i].from; into[i] = source < 0 ? (int32_t)r->filter[i].into : 0; }
  mcx_join_stats s0, s1;
  mcx_check(mcx_join_get_stats(j, &s0), "join");
  uint64_t nread = 0;
  for (;;) {
    const size_t got = fread(buf, 1, chunk_recs * rec_bytes, r->fh);
    if (got == 0) break;
    if (got % rec_bytes) die("Unexpected end of file: %s", r->path);
    mcx_check(mcx_join_add_records(j, source, buf, got / rec_bytes, (int)r->num_cols, from, into, (int)r->nfilter), "load graph records");
    nread += got / rec_bytes;
  }
  mcx_check(mcx_join_get_stats(j, &s1), "join");
  const uint64_t kept = source < 0 ? s1.recs_kept - s0.recs_kept : s1.isec_recs_kept - s0.isec_recs_kept;
  if (r->num_kmers >= 0 && nread != (uint64_t)r->num_kmers)
    warn("%s kmers in the graph file than expected [exp: %zu; act: %zu; path: %s]",
         nread > (uint64_t)r->num_kmers ? "More" : "Fewer", (size_t)r->num_kmers, (size_t)nread, r->path);
  status("[GReader] Loaded %s / %s (%.2f%%) of kmers parsed", ulong_to_str(kept, a), ulong_to_str(nread, b),
         nread ? 100.0 * (double)kept / (double)nread : 0.0);
  free(from); free(into);
}

int ctx_join(int argc, char **argv)
{
  const char *out_path = NULL;
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, sort_kmers = false;
  unsigned use_ncols = 0, device = 0;
  ctx_reader *isec = NULL;
  size_t nisec = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:N:i:S", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(join_usage, NULL);
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 'f': ONCE(force); force = true; break;
      case 'm': cmd_mem_set_memory(&mem, join_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, join_usage, optarg); break;
      case 'N':
        ONCE(use_ncols);
        if (!parse_entire_uint(optarg, &use_ncols) || !use_ncols) print_usage(join_usage, "%s requires an int x > 0", cmd);
        break;
      case 'i':
        isec = realloc(isec, (nisec + 1) * sizeof(ctx_reader));
        if (!isec) die("Out of memory");
        ctx_reader_open(&isec[nisec], optarg, 0, MIN_KMER_SIZE, MAX_KMER_SIZE);
        if (isec[nisec].into_ncols > 1) warn("Flattening intersection graph into colour 0: %s", optarg);
        nisec++;
        break;
      case 'S': ONCE(sort_kmers); sort_kmers = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(join_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " join -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (!out_path) print_usage(join_usage, "--out <out.ctx> required");
  if (optind >= argc) print_usage(join_usage, "Please specify at least one input graph file");
  const size_t nfiles = (size_t)(argc - optind);
  status("Probing %zu graph files and %zu intersect files", nfiles, nisec);

  graph_files in;
  graph_files_open(argv + optind, nfiles, join_usage, &in);
  const size_t ncols = in.ncols, kmer_size = in.files[0].kmer_size;

  /* the smallest intersection graph goes first: it is loaded first and its edges are the mask (ctx_join.c:150-158) */
  uint64_t min_isec_kmers = 0;
  for (size_t i = 0; i < nisec; i++) {
    if (isec[i].kmer_size != kmer_size) print_usage(join_usage, "Kmer sizes don't match [%u vs %u]", (unsigned)kmer_size, isec[i].kmer_size);
    const uint64_t nk = reader_nkmers(&isec[i]);
    if (i == 0) min_isec_kmers = nk;
    else if (nk < min_isec_kmers) {
      ctx_reader t = isec[i]; isec[i] = isec[0]; isec[0] = t;
      min_isec_kmers = nk;
    }
  }

  const bool to_stdout = !strcmp(out_path, "-");
  if (use_ncols) {
    if (use_ncols < ncols && to_stdout) die("I need %zu colours if outputting to STDOUT (--ncols)", ncols);
    if (use_ncols > ncols) warn("I only need %zu colour%s ('--ncols %u' ignored)", ncols, plural(ncols), use_ncols);
  }
  /* futil_create_output */
  if (!to_stdout && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);
  status("Output %zu cols; from %zu files; intersecting %zu graphs; ", ncols, nfiles, nisec);

  /* ---- memory: the records as they lie in the files, a locator per record, the sort's four 64-bit arrays, its scratch
   * and the run tables per record, two output chunks ---- */
  uint64_t body_bytes = 0, nrecs = 0;
  for (size_t i = 0; i < nfiles + nisec; i++) {
    const ctx_reader *r = i < nfiles ? &in.files[i] : &isec[i - nfiles];
    if (r->file_size >= 0) body_bytes += (uint64_t)r->file_size - r->hdr_size;
    nrecs += reader_nkmers(r);
  }
  /* per record what mcx_join_finish checks (mcx_join.h): 8 locator + 32 sort arrays + 10 run tables + 16 for the radix
   * sort's own scratch (a second copy of keys and values); every record counted as kept */
  const uint64_t need = body_bytes + nrecs * (8 + 32 + 10 + 16) + (2ull << 26) + (1ull << 20);
  char s1[64], s2[64];
  if (mem.mem_set && need > mem.mem_to_use)
    die("Not enough memory for requested graph: require at least %s [>%s]", bytes_to_str(need, 1, s1), bytes_to_str(mem.mem_to_use, 1, s2));
  status("[memory] join: %s of HBM for %s records", bytes_to_str(need, 1, s1), ulong_to_str(nrecs, s2));

  if (mcx_device_count() < 1) die("No MI355X / HIP device found: %s has no CPU build path", CMD_NAME);
  uint64_t hbm_free = 0, hbm_total = 0;
  mcx_check(mcx_device_memory((int)device, &hbm_free, &hbm_total), "device query");
  if (need > hbm_free)
    die("Requesting more memory than is available [ Reqeusted: %s HBM free: %s ]", bytes_to_str(need, 1, s1), bytes_to_str(hbm_free, 1, s2));

  /* ---- header: graph_file_merge_header of every input, then the intersection's name on every colour that is loaded ---- */
  col_info *cols = graph_files_merge_headers(&in, ncols);
  if (nisec) {
    char *iname = NULL;
    for (size_t i = 0; i < nisec; i++) make_intersect(&isec[i].ginfo[0], &iname);
    bool *loaded = calloc(ncols, sizeof(bool)); /* graph_file_is_colour_loaded */
    if (!loaded) die("Out of memory");
    for (size_t f = 0; f < nfiles; f++)
      for (size_t m = 0; m < in.files[f].nfilter; m++) loaded[in.files[f].filter[m].into] = true;
    for (size_t i = 0; i < ncols; i++)
      if (loaded[i]) append_intersect(&cols[i].cleaning, iname);
    free(loaded);
    free(iname);
  }

  /* the reference writes the intersection's k-mers that no input has when it dumps the table: graph_write_empty with
   * more than one input, or the sorted dump */
  const uint32_t flags = nisec && (nfiles > 1 || sort_kmers) ? MCX_JOIN_KEEP_EMPTY : 0;
  mcx_join *j = NULL;
  mcx_check(mcx_join_create(&j, (int)kmer_size, (int)ncols, (int)nisec, flags, (int)device), "Cannot set up the join");
  const size_t buf_bytes = 64u << 20;
  void *buf = NULL;
  mcx_check(mcx_join_buffer(j, buf_bytes, &buf), "Cannot allocate the read buffer");
  for (size_t i = 0; i < nisec; i++) join_load(j, &isec[i], (int)i, buf, buf_bytes);
  if (nisec) status("Loaded intersection set\n");
  for (size_t i = 0; i < nfiles; i++) join_load(j, &in.files[i], -1, buf, buf_bytes);

  FILE *fout = stdout;
  if (!to_stdout) {
    fout = fopen(out_path, "wb");
    if (!fout) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  }
  const size_t hdr = ctx_write_header(fout, (uint32_t)kmer_size, (uint32_t)ncols, cols);
  mcx_join_stats st;
  mcx_check(mcx_join_finish(j, write_sink, fout, &st), "join");
  if (fflush(fout) != 0) die("Cannot write to file: %s", out_path);
  if (nisec) status("[join] %s kmers in the intersection; %s written without coverage", ulong_to_str(st.kmers_intersection, s1), ulong_to_str(st.kmers_written_no_covg, s2));
  ctx_dumped_status(st.kmers_written, kmer_size, ncols, hdr, out_path);
  if (fout != stdout && fclose(fout) != 0) die("Cannot write to file: %s", out_path);

  mcx_join_destroy(j);
  col_infos_free(cols, ncols);
  for (size_t i = 0; i < nisec; i++) ctx_reader_close(&isec[i]);
  free(isec);
  graph_files_close(&in);
  return EXIT_SUCCESS;
}
