/* cmd_breakpoints.c -- `mccortex<K> breakpoints` (src/commands/ctx_breakpoints.c, src/tools/breakpoint_caller.c): the graph
 * files are loaded into one multi-colour table with one more colour, `BrkpntRef`, behind them; the trusted sequences are
 * read whole into memory and handed to the MI355X, which adds them to that colour, indexes where their k-mers occur and
 * makes the calls (mcx_graph_breakpoints).  The host writes the JSON header (breakpoints_print_header) and the
 * reference's comment lines through zlib and hands the text the device made to the same stream.
 *
 * Where this differs from the reference (DESIGN.md lists it): the breaks are taken in key order, FORWARD before REVERSE,
 * and the calls are numbered in that order (the reference walks its hash table with racing threads); merged flanks and
 * alleles are ordered by their smallest colour; the header's max_ref_flank_kmers is the real -R (the reference passes
 * min_ref_nkmers twice); -p is refused, the walks hold no links; --device picks the GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <limits.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include "../../include/mcx_gpu.h"

#define DEFAULT_MIN_REF_NKMERS 5
#define DEFAULT_MAX_REF_NKMERS 1000

static const char breakpoints_usage[] =
"usage: " CMD_NAME " breakpoints [options] <in.ctx> [in2.ctx ..]\n"
"\n"
"  Use trusted assembled genome to call large events.  Output is gzipped.\n"
"  The table holds the k-mers of the graph files and of the trusted sequences.\n"
"\n"
"  -h, --help              This help message\n"
"  -q, --quiet             Silence status output normally printed to STDERR\n"
"  -f, --force             Overwrite output files\n"
"  -m, --memory <mem>      Memory to use\n"
"  -n, --nkmers <kmers>    Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>       Accepted as the reference takes it; the calls are made on the device\n"
"  -p, --paths <in.ctp>    Load link file (not part of this build: the walks hold no links)\n"
"  -o, --out <out.txt.gz>  Save calls (gzipped output) [default: STDOUT]\n"
"  -s, --seq <in>          Trusted input (can specify multiple times)\n"
"  -r, --minref <N>        Require <N> kmers at ref breakpoint [default: " MCX_STR(DEFAULT_MIN_REF_NKMERS) "]\n"
"  -R, --maxref <N>        Stop after <N> kmers at ref breakpoint [default: " MCX_STR(DEFAULT_MAX_REF_NKMERS) "]\n"
"  -E, --no-ref-edges      Don't load edges from the reference\n"
"      --device <N>        GPU to run on [default: 0]\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},          {"memory", required_argument, NULL, 'm'}, {"nkmers", required_argument, NULL, 'n'},
  {"threads", required_argument, NULL, 't'}, {"paths", required_argument, NULL, 'p'},  {"out", required_argument, NULL, 'o'},
  {"force", no_argument, NULL, 'f'},         {"seq", required_argument, NULL, '1'},    {"seq", required_argument, NULL, 's'},
  {"minref", required_argument, NULL, 'r'},  {"maxref", required_argument, NULL, 'R'}, {"no-ref-edges", no_argument, NULL, 'E'},
  {"device", required_argument, NULL, OPT_DEVICE}, {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(breakpoints_usage, "%s given twice", cmd); } while (0)

static const char brk_comment[] =
"\n"
"# This file was generated with McCortex\n"
"#   written by Isaac Turner <turner.isaac@gmail.com>\n"
"#   url: https://github.com/mcveanlab/mccortex\n"
"# \n"
"# Comment lines begin with a # and are ignored, but must come after the header\n"
"# Format is:\n"
"#   chr=seq:start-end:strand:offset\n"
"#   all coordinates are 1-based\n"
"#   <strand> is + or -. If +, start <= end. If -, start >= end.\n"
"#   <offset> is the position in the sequence where ref starts agreeing\n"
"\n";

static int gz_sink(void *ctx, const void *data, size_t nbytes)
{
  while (nbytes) { /* (gzwrite takes an unsigned) */
    const unsigned n = nbytes > (1u << 30) ? (1u << 30) : (unsigned)nbytes;
    if (gzwrite((gzFile)ctx, data, n) != (int)n) return 1;
    data = (const char *)data + n;
    nbytes -= n;
  }
  return 0;
}

/* the names as the calls print them (ctx_breakpoints.c:239-246): cut at the first whitespace, ',' -> '.', ':' -> ';' */
static void clean_names(const read_batch *b, char **names_out, uint64_t **off_out)
{
  char *names = malloc(b->names_len + 1);
  uint64_t *off = malloc((b->nreads + 1) * sizeof(*off));
  if (!names || !off) die("Out of memory");
  uint64_t at = 0;
  for (size_t i = 0; i < b->nreads; i++) {
    off[i] = at;
    for (uint64_t j = b->name_off[i]; j < b->name_off[i + 1]; j++) {
      const char ch = b->names[j];
      if (ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n' || ch == '\v' || ch == '\f') break;
      names[at++] = ch == ',' ? '.' : ch == ':' ? ';' : ch;
    }
  }
  off[b->nreads] = at;
  *names_out = names;
  *off_out = off;
}

/* breakpoints_print_header: json_hdr_make_std, the reference colour marked, the parameters of the calling, the trusted
 * files and their sequences */
static void write_header(gzFile gz, const char *out_path, int argc, char **argv, size_t kmer_size, size_t ncols, uint64_t nkmers, const col_info *cols,
                         const mcx_breakpoints_params *prm, char **seq_paths, size_t nseq, const read_batch *ref, const char *names, const uint64_t *name_off)
{
  char file_key[17], cmd_key[9];
  ctp_hex_key(file_key, 16);
  ctp_hex_key(cmd_key, 8);
  gzputs(gz, "{\n  \"file_format\": \"CtxBreakpoints\",\n  \"format_version\": 3,\n  \"file_key\": ");
  ctp_put_str(gz, file_key);
  gzprintf(gz, ",\n  \"graph\": {\n    \"num_colours\": %zu,\n    \"kmer_size\": %zu,\n    \"num_kmers_in_graph\": %llu,\n    \"colours\": [", ncols, kmer_size,
           (unsigned long long)nkmers);
  for (size_t i = 0; i < ncols; i++) {
    const col_info *col = &cols[i];
    gzprintf(gz, "%s{\n        \"colour\": %zu,\n        \"sample\": ", i ? ", " : "", i);
    ctp_put_str(gz, col->name ? col->name : "undefined");
    gzprintf(gz, ",\n        \"total_sequence\": %llu,\n        \"cleaned_tips\": %s,\n", (unsigned long long)col->total_sequence,
             col->cleaning.cleaned_tips ? "true" : "false");
    if (col->cleaning.cleaned_unitigs) gzprintf(gz, "        \"cleaned_unitigs\": %u", col->cleaning.clean_unitigs_thresh);
    else gzputs(gz, "        \"cleaned_unitigs\": false");
    gzputs(gz, i + 1 == ncols ? ",\n        \"is_ref\": true\n      }" : "\n      }");
  }
  gzputs(gz, "]\n  },\n  \"commands\": [");
  ctp_str s = {NULL, 0, 0};
  ctp_hdr_command(&s, cmd_key, argc, argv, out_path, file_key, NULL);
  /* json_hdr_augment_cmd: the command's own object goes in as its last member */
  while (s.len && s.b[s.len - 1] != '}') s.len--;
  while (s.len && (s.b[s.len - 1] == '}' || s.b[s.len - 1] == ' ' || s.b[s.len - 1] == '\n')) s.len--;
  gzwrite(gz, s.b, (unsigned)s.len);
  free(s.b);
  gzprintf(gz, ",\n      \"breakpoints\": {\n        \"min_ref_flank_kmers\": %u,\n        \"max_ref_flank_kmers\": %u,\n        \"load_ref_edges\": %s,\n"
               "        \"ref_files\": [", prm->min_ref, prm->max_ref, (prm->flags & MCX_BREAKPOINTS_NO_REF_EDGES) ? "false" : "true");
  for (size_t i = 0; i < nseq; i++) {
    char abspath[PATH_MAX + 1];
    if (i) gzputs(gz, ", ");
    ctp_put_str(gz, realpath(seq_paths[i], abspath) ? abspath : seq_paths[i]);
  }
  gzputs(gz, "],\n        \"contigs\": [");
  for (size_t i = 0; i < ref->nreads; i++) {
    char *id = strndup(names + name_off[i], (size_t)(name_off[i + 1] - name_off[i]));
    if (!id) die("Out of memory");
    gzputs(gz, i ? ", {\n            \"id\": " : "{\n            \"id\": ");
    ctp_put_str(gz, id);
    gzprintf(gz, ",\n            \"length\": %llu\n          }", (unsigned long long)(ref->offsets[i + 1] - ref->offsets[i]));
    free(id);
  }
  gzputs(gz, "]\n      }\n    }]\n}\n");
}

int ctx_breakpoints(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, no_ref_edges = false, max_seen = false;
  unsigned nthreads = 0, device = 0, min_ref = 0, max_ref = 0;
  const char *out_path = NULL;
  char **seq_paths = calloc((size_t)argc + 1, sizeof(char *));
  size_t nseq = 0;
  char cmd[100];
  int c;
  if (!seq_paths) die("Out of memory");
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "hm:n:t:p:o:f1:s:r:R:E", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(breakpoints_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 't': cmd_threads_arg(&nthreads, breakpoints_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, breakpoints_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, breakpoints_usage, optarg); break;
      case 'p': die("-p, --paths <in.ctp>: link files are not part of this build's `breakpoints`; the walks hold no links");
      case 'r': ONCE(min_ref); if (!parse_entire_uint(optarg, &min_ref) || !min_ref) print_usage(breakpoints_usage, "%s requires an int x > 0: %s", cmd, optarg); break;
      case 'R': ONCE(max_seen); max_seen = true; if (!parse_entire_uint(optarg, &max_ref)) print_usage(breakpoints_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case '1':
      case 's': seq_paths[nseq++] = optarg; break;
      case 'E': ONCE(no_ref_edges); no_ref_edges = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(breakpoints_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " breakpoints -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (out_path == NULL) out_path = "-";
  if (!min_ref) min_ref = DEFAULT_MIN_REF_NKMERS;
  if (!max_ref) max_ref = DEFAULT_MAX_REF_NKMERS; /* -R 0 means the default, as in the reference */
  if (nseq == 0) print_usage(breakpoints_usage, "Require at least one --seq file");
  if (optind >= argc) print_usage(breakpoints_usage, "Require input graph files (.ctx)");
  if (min_ref > max_ref) print_usage(breakpoints_usage, "-r, --minref <N> must not be above -R, --maxref <N>: %u > %u", min_ref, max_ref);

  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), breakpoints_usage, &in);
  const size_t kmer_size = in.files[0].kmer_size, W = in.files[0].num_words, ncols = in.ncols + 1; /* a colour for the reference */
  col_info *cols = graph_files_merge_headers(&in, ncols);
  col_info_set_name(&cols[ncols - 1], "BrkpntRef");

  /* seq_load_all_reads: all of every --seq file into memory */
  read_batch ref;
  read_batch_init(&ref, false);
  read_batch_keep_names(&ref);
  for (size_t i = 0; i < nseq; i++) {
    seq_in *s = seq_in_open(seq_paths[i]);
    if (!s) die("Cannot read --seq file %s", seq_paths[i]);
    while (seq_in_fill(s, &ref, SIZE_MAX)) {}
    seq_in_close(s);
  }
  if (ref.nreads == 0) die("No sequences in the --seq file%s", nseq > 1 ? "s" : "");
  if (ref.nreads > (1u << 30)) die("More chromosomes than permitted (%zu > %u)", ref.nreads, 1u << 30);
  for (size_t i = 0; i < ref.nreads; i++)
    if (ref.offsets[i + 1] - ref.offsets[i] > (1ull << 32))
      die("Read longer than limit (%llu > %llu; %zu: '%.*s')", (unsigned long long)(ref.offsets[i + 1] - ref.offsets[i]), 1ull << 32, i,
          (int)(ref.name_off[i + 1] - ref.name_off[i]), ref.names + ref.name_off[i]);
  char *names = NULL;
  uint64_t *name_off = NULL;
  clean_names(&ref, &names, &name_off);
  col_info_update(&cols[ncols - 1], ref.nbases, ref.nreads);

  mcx_breakpoints_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.min_ref = min_ref;
  prm.max_ref = max_ref;
  prm.flags = no_ref_edges ? MCX_BREAKPOINTS_NO_REF_EDGES : 0u;

  /* kmer memory = kmer + coverage + edges of every colour; the table takes the files' k-mers and the reference's */
  const size_t bits_per_kmer = 64 * W + 40 * ncols;
  table_plan plan;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)(in.sum_kmers + ref.nbases), &plan);
  if (err) die("%s", err);
  table_plan_status(&plan);

  /* futil_gzopen_create: an existing file is kept unless --force */
  const bool to_stdout = strcmp(out_path, "-") == 0;
  if (!to_stdout && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);
  gzFile gz = to_stdout ? gzdopen(dup(STDOUT_FILENO), "w") : gzopen(out_path, "w");
  if (!gz) die("Cannot open output file: %s [%s]", out_path, strerror(errno));

  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, ncols, device))) {
    gzclose(gz);
    if (!to_stdout) unlink(out_path);
    die("%s", err);
  }
  for (size_t i = 0; i < in.n; i++) ctx_load_graph_file(g, &in.files[i]);
  hasht_status(g);

  status("[kograh] Adding reference annotations to the graph on the device");
  status("Running BreakpointCaller on the device, output to: %s", outpath(out_path));
  status("  Finding breakpoints after at least %u kmers (%zubp) of homology", min_ref, (size_t)min_ref + kmer_size - 1);
  /* the reference goes in first: the header tells the k-mers of the graph with the reference in it; then the calls
   * stream behind the header */
  mcx_breakpoints_stats st;
  memset(&st, 0, sizeof(st));
  mcx_breakpoints_params load = prm;
  load.flags |= MCX_BREAKPOINTS_LOAD_ONLY;
  mcx_check(mcx_graph_breakpoints(g, ref.bases, ref.offsets, ref.nreads, names, name_off, &load, NULL, NULL, NULL, NULL, &st), "breakpoints");
  uint64_t nkmers = 0;
  mcx_check(mcx_graph_nkmers(g, &nkmers), "breakpoints");
  write_header(gz, out_path, argc, argv, kmer_size, ncols, nkmers, cols, &prm, seq_paths, nseq, &ref, names, name_off);
  gzputs(gz, brk_comment);
  mcx_breakpoints_params calling = prm;
  calling.flags |= MCX_BREAKPOINTS_REF_LOADED;
  mcx_check(mcx_graph_breakpoints(g, ref.bases, ref.offsets, ref.nreads, names, name_off, &calling, NULL, NULL, gz_sink, gz, &st), "breakpoints");
  if (gzclose(gz) != Z_OK) die("Cannot write to file: %s", outpath(out_path));

  char n0[50], n1[50], n2[50];
  status("  %s calls printed to %s", ulong_to_str(st.calls, n0), outpath(out_path));
  status("[Breakpoints] reference: %s k-mer occurrences indexed over %s k-mers, %s k-mers added", ulong_to_str(st.occurrences, n0),
         ulong_to_str(st.ref_keys, n1), ulong_to_str(st.ref_added, n2));
  status("[Breakpoints] breaks: %s, flanks: %s (%llu without a run), alleles: %s (%llu without a run)", ulong_to_str(st.breaks, n0), ulong_to_str(st.flanks, n1),
         (unsigned long long)st.flanks_norun, ulong_to_str(st.alleles, n2), (unsigned long long)st.alleles_norun);
  status("[Breakpoints] walks stopped: %llu where their run ended, %llu at --maxref, %llu flanks off the reference, %llu at a dead end, "
         "%llu at a fork outside the colour, %llu at a fork inside it, %llu in a loop",
         (unsigned long long)st.stop_runs, (unsigned long long)st.stop_maxref, (unsigned long long)st.stop_flank, (unsigned long long)st.stop_nocovg,
         (unsigned long long)st.stop_nocolcovg, (unsigned long long)st.stop_nolinks, (unsigned long long)st.stop_repeat);

  free(names);
  free(name_off);
  free(seq_paths);
  read_batch_free(&ref);
  col_infos_free(cols, ncols);
  graph_files_close(&in);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
