/* cmd_bubbles.c -- `mccortex<K> bubbles` (src/commands/ctx_bubbles.c, src/tools/bubble_caller.c): the graph files are
 * loaded into one multi-colour table as the other graph commands load them and the calls of every fork are made on the
 * MI355X (mcx_graph_bubbles).  The host writes the JSON header (bubble_caller_print_header) and the reference's comment
 * lines through zlib and hands the text the device made to the same stream.
 *
 * Where this differs from the reference (DESIGN.md lists it): the forks are taken in key order, FORWARD before REVERSE,
 * and the calls are numbered in that order (the reference walks its hash table with racing threads); -p is refused, the
 * walks hold no links; -S is a plain flag, as the reference's usage text shows it (its option table declares an argument);
 * --device picks the GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include "../../include/mcx_gpu.h"

#define DEFAULT_MAX_FLANK 500
#define DEFAULT_MAX_ALLELE 2000

static const char bubbles_usage[] =
"usage: " CMD_NAME " bubbles [options] <in.ctx> [in2.ctx ...]\n"
"\n"
"  Find bubbles in the graph, which are potential variants.\n"
"\n"
"  -h, --help              This help message\n"
"  -q, --quiet             Silence status output normally printed to STDERR\n"
"  -f, --force             Overwrite output files\n"
"  -o, --out <bub.txt.gz>  Output file [required]\n"
"  -m, --memory <mem>      Memory to use\n"
"  -n, --nkmers <kmers>    Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>       Accepted as the reference takes it; the calls are made on the device\n"
"  -p, --paths <in.ctp>    Load link file (not part of this build: the walks hold no links)\n"
"  -H, --haploid <col>     List of haploid colours (e.g. ref colour); '*' means all\n"
"  -A, --max-allele <len>  Max bubble branch length in kmers [default: " MCX_STR(DEFAULT_MAX_ALLELE) "]\n"
"  -F, --max-flank <len>   Max flank length in kmers [default: " MCX_STR(DEFAULT_MAX_FLANK) "]\n"
"  -S, --keep-serial       Keep serial bubbles. Use if mapping is hard. Higher FP.\n"
"      --device <N>        GPU to run on [default: 0]\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},           {"out", required_argument, NULL, 'o'},        {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'},   {"threads", required_argument, NULL, 't'},    {"paths", required_argument, NULL, 'p'},
  {"force", no_argument, NULL, 'f'},          {"haploid", required_argument, NULL, 'H'},    {"max-allele", required_argument, NULL, 'A'},
  {"max-flank", required_argument, NULL, 'F'}, {"keep-serial", no_argument, NULL, 'S'},     {"device", required_argument, NULL, OPT_DEVICE},
  {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(bubbles_usage, "%s given twice", cmd); } while (0)

static const char bub_comment[] =
"\n"
"# This file was generated with McCortex\n"
"#   written by Isaac Turner <turner.isaac@gmail.com>\n"
"#   url: https://github.com/mcveanlab/mccortex\n"
"# \n"
"# Comment lines begin with a # and are ignored, but must come after the header\n"
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

/* range_parse_array: "3", "0-2", "4-1", "0,2-3,7" or "*" over ncols colours; the list (the caller frees it), or NULL */
static uint32_t *colour_list(const char *arg, size_t ncols, size_t *n_out)
{
  size_t n = 0, cap = ncols + 8;
  uint32_t *v = malloc(cap * sizeof(*v));
  if (!v) die("Out of memory");
  if (!strcmp(arg, "*")) {
    for (size_t i = 0; i < ncols; i++) v[n++] = (uint32_t)i;
    *n_out = n;
    return v;
  }
  for (const char *p = arg; *p;) {
    char *e;
    if (*p < '0' || *p > '9') { free(v); return NULL; }
    unsigned long a = strtoul(p, &e, 10), b = a;
    if (*e == '-') {
      p = e + 1;
      if (*p < '0' || *p > '9') { free(v); return NULL; }
      b = strtoul(p, &e, 10);
    }
    if (a >= ncols || b >= ncols) { free(v); return NULL; }
    for (unsigned long x = a;; x += a <= b ? 1 : -1) {
      if (n == cap && !(v = realloc(v, (cap *= 2) * sizeof(*v)))) die("Out of memory");
      v[n++] = (uint32_t)x;
      if (x == b) break;
    }
    if (*e == ',' && e[1]) p = e + 1;
    else if (!*e) p = e;
    else { free(v); return NULL; }
  }
  if (!n) { free(v); return NULL; }
  *n_out = n;
  return v;
}

/* bubble_caller_print_header: json_hdr_make_std and the parameters of the calling, closed by an empty line */
static void write_header(gzFile gz, const char *out_path, int argc, char **argv, size_t kmer_size, size_t ncols, uint64_t nkmers, const col_info *cols,
                         const mcx_bubbles_params *prm)
{
  char file_key[17], cmd_key[9];
  ctp_hex_key(file_key, 16);
  ctp_hex_key(cmd_key, 8);
  gzputs(gz, "{\n  \"file_format\": \"CtxBubbles\",\n  \"format_version\": 2,\n  \"file_key\": ");
  ctp_put_str(gz, file_key);
  gzprintf(gz, ",\n  \"graph\": {\n    \"num_colours\": %zu,\n    \"kmer_size\": %zu,\n    \"num_kmers_in_graph\": %llu,\n    \"colours\": [", ncols, kmer_size,
           (unsigned long long)nkmers);
  for (size_t i = 0; i < ncols; i++) {
    const col_info *col = &cols[i];
    gzprintf(gz, "%s{\n        \"colour\": %zu,\n        \"sample\": ", i ? ", " : "", i);
    ctp_put_str(gz, col->name ? col->name : "undefined");
    gzprintf(gz, ",\n        \"total_sequence\": %llu,\n        \"cleaned_tips\": %s,\n", (unsigned long long)col->total_sequence,
             col->cleaning.cleaned_tips ? "true" : "false");
    if (col->cleaning.cleaned_unitigs) gzprintf(gz, "        \"cleaned_unitigs\": %u\n", col->cleaning.clean_unitigs_thresh);
    else gzputs(gz, "        \"cleaned_unitigs\": false\n");
    gzputs(gz, "      }");
  }
  gzputs(gz, "]\n  },\n  \"commands\": [");
  ctp_str s = {NULL, 0, 0};
  ctp_hdr_command(&s, cmd_key, argc, argv, out_path, file_key, NULL);
  /* json_hdr_augment_cmd: the command's own object goes in as its last member */
  while (s.len && s.b[s.len - 1] != '}') s.len--;
  while (s.len && (s.b[s.len - 1] == '}' || s.b[s.len - 1] == ' ' || s.b[s.len - 1] == '\n')) s.len--;
  gzwrite(gz, s.b, (unsigned)s.len);
  free(s.b);
  gzprintf(gz, ",\n      \"bubbles\": {\n        \"max_flank_kmers\": %u,\n        \"max_allele_kmers\": %u,\n        \"haploid_colours\": [", prm->max_flank,
           prm->max_allele);
  for (uint32_t i = 0; i < prm->nhaploid; i++) gzprintf(gz, "%s%u", i ? ", " : "", prm->haploid[i]);
  gzputs(gz, "]\n      }\n    }]\n}\n");
}

int ctx_bubbles(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, keep_serial = false;
  unsigned nthreads = 0, device = 0, max_allele = 0, max_flank = 0;
  const char *out_path = NULL, *hap_arg = NULL;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:m:n:t:p:fH:A:F:S", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(bubbles_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 't': cmd_threads_arg(&nthreads, bubbles_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, bubbles_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, bubbles_usage, optarg); break;
      case 'p': die("-p, --paths <in.ctp>: link files are not part of this build's `bubbles`; the walks hold no links");
      case 'H': ONCE(hap_arg); hap_arg = optarg; break;
      case 'A': ONCE(max_allele); if (!parse_entire_uint(optarg, &max_allele) || !max_allele) print_usage(bubbles_usage, "%s requires an int x > 0: %s", cmd, optarg); break;
      case 'F': ONCE(max_flank); if (!parse_entire_uint(optarg, &max_flank) || !max_flank) print_usage(bubbles_usage, "%s requires an int x > 0: %s", cmd, optarg); break;
      case 'S': ONCE(keep_serial); keep_serial = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(bubbles_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " bubbles -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (out_path == NULL) out_path = "-";
  if (!max_allele) max_allele = DEFAULT_MAX_ALLELE;
  if (!max_flank) max_flank = DEFAULT_MAX_FLANK;
  if (optind >= argc) print_usage(bubbles_usage, "Require input graph files (.ctx)");

  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), bubbles_usage, &in);
  const size_t kmer_size = in.files[0].kmer_size, W = in.files[0].num_words, ncols = in.ncols;
  col_info *cols = graph_files_merge_headers(&in, ncols);

  mcx_bubbles_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.max_allele = max_allele;
  prm.max_flank = max_flank;
  prm.flags = keep_serial ? MCX_BUBBLES_KEEP_SERIAL : 0u;
  uint32_t *hap = NULL;
  if (hap_arg) {
    size_t nhap = 0;
    if (!(hap = colour_list(hap_arg, ncols, &nhap))) die("Invalid haploid colour list: %s", hap_arg);
    prm.haploid = hap;
    prm.nhaploid = (uint32_t)nhap;
  }

  /* kmer memory = kmer + coverage + edges of every colour */
  const size_t bits_per_kmer = 64 * W + 40 * ncols;
  table_plan plan;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
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
  uint64_t nkmers = 0;
  mcx_check(mcx_graph_nkmers(g, &nkmers), "bubbles");

  status("Calling bubbles on the device, output: %s", outpath(out_path));
  {
    char list[256] = "";
    size_t at = 0;
    for (uint32_t i = 0; i < prm.nhaploid && at + 16 < sizeof(list); i++) at += (size_t)snprintf(list + at, sizeof(list) - at, "\t%u", prm.haploid[i]);
    status("Haploid colours:%s", list);
  }
  write_header(gz, out_path, argc, argv, kmer_size, ncols, nkmers, cols, &prm);
  gzputs(gz, bub_comment);
  mcx_bubbles_stats st;
  memset(&st, 0, sizeof(st));
  mcx_check(mcx_graph_bubbles(g, &prm, NULL, NULL, gz_sink, gz, &st), "bubbles");
  if (gzclose(gz) != Z_OK) die("Cannot write to file: %s", outpath(out_path));

  char n0[50], n1[50], n2[50];
  status("Bubble Caller called %s bubbles\n", ulong_to_str(st.bubbles, n0));
  status("Haploid bubbles dropped: %s", ulong_to_str(st.haploid_dropped, n0));
  status("Serial bubbles dropped: %s", ulong_to_str(st.serial_dropped, n0));
  status("[Bubbles] forks: %s, paths: %s, steps: %s", ulong_to_str(st.forks, n0), ulong_to_str(st.paths, n1), ulong_to_str(st.steps, n2));
  status("[Bubbles] paths stopped: %llu at the length limit, %llu at a dead end, %llu at a fork outside the colour, %llu at a fork inside it, %llu in a loop",
         (unsigned long long)st.stop_limit, (unsigned long long)st.stop_nocovg, (unsigned long long)st.stop_nocolcovg, (unsigned long long)st.stop_nolinks,
         (unsigned long long)st.stop_repeat);
  status("  saved to: %s\n", outpath(out_path));

  col_infos_free(cols, ncols);
  graph_files_close(&in);
  free(hap);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
