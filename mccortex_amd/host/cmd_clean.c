/* cmd_clean.c -- `mccortex<K> clean` (src/commands/ctx_clean.c, src/tools/clean_graph.c): same options, defaults,
 * messages and output.  The graphs are loaded into the device table as `build --graph` loads them; the unitigs,
 * their medians, the tip test and the prune run on the MI355X (mcx_graph_unitig_stats, mcx_graph_clean); the
 * threshold is picked on the host between the two calls (clean_thresh.c). */
#define _GNU_SOURCE
#include "host.h"

#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/mcx_gpu.h"

static const char clean_usage[] =
"usage: " CMD_NAME " clean [options] <in.ctx> [in2.ctx ...]\n"
"\n"
"  Clean a cortex graph. Joins graphs first, if multiple inputs given.\n"
"  If output graph file is not specified just saves output statistics.\n"
"  If given a multisample graph, cleans each sample against the merged population.\n"
"\n"
"  -h, --help               This help message\n"
"  -q, --quiet              Silence status output normally printed to STDERR\n"
"  -f, --force              Overwrite output files\n"
"  -o, --out <out.ctx>      Save output graph file [required]\n"
"  -m, --memory <mem>       Memory to use\n"
"  -n, --nkmers <kmers>     Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>        Number of threads to use [default: 2]\n"
"  -N, --ncols <N>          Number of graph colours to use\n"
"  -S, --sort               Output a graph file ordered by kmer\n"
"  -D, --device <N>         GPU to run on [default: 0]\n"
"\n"
"  Cleaning:\n"
"  -T[L], --tips[=L]        Clip tips shorter than <L> kmers [default: auto]\n"
"  -U[X], --unitigs[=X]     Remove low coverage unitigs with median cov < X [default: auto]\n"
"  -B, --fallback <T>       Fall back threshold if we can't pick\n"
"\n"
"  Statistics:\n"
"  -c, --covg-before <out.csv> Save kmer coverage histogram before cleaning\n"
"  -C, --covg-after <out.csv>  Save kmer coverage histogram after cleaning\n"
"  -l, --len-before <out.csv>  Save unitig length histogram before cleaning\n"
"  -L, --len-after <out.csv>   Save unitig length histogram after cleaning\n"
"\n"
"  --unitigs without a threshold, causes a calculated threshold to be used\n"
"  Default: --tips 2*kmer_size --unitigs\n"
"  Set thresholds to zero to turn-off cleaning\n"
"\n";

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},           {"out", required_argument, NULL, 'o'},
  {"force", no_argument, NULL, 'f'},          {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'},   {"threads", required_argument, NULL, 't'},
  {"ncols", required_argument, NULL, 'N'},    {"sort", no_argument, NULL, 'S'},
  {"tips", optional_argument, NULL, 'T'},     {"unitigs", optional_argument, NULL, 'U'},
  {"fallback", required_argument, NULL, 'B'}, {"len-before", required_argument, NULL, 'l'},
  {"len-after", required_argument, NULL, 'L'}, {"covg-before", required_argument, NULL, 'c'},
  {"covg-after", required_argument, NULL, 'C'}, {"device", required_argument, NULL, 'D'},
  {NULL, 0, NULL, 0}};

/* cleaning_write_covg_histogram / cleaning_write_len_histogram (clean_graph.c) */
static FILE *open_hist(const char *path, const char *name)
{
  status("[cleaning] Writing %s distribution to: %s", name, outpath(path));
  if (!strcmp(path, "-")) return stdout;
  FILE *f = fopen(path, "w");
  if (!f) warn("Couldn't write %s distribution to file: %s", name, path);
  return f;
}

static void close_hist(FILE *f)
{
  if (f == stdout) fflush(f);
  else fclose(f);
}

static void write_covg_hist(const char *path, const uint64_t *covg, const uint64_t *ucovg, size_t len)
{
  FILE *f = open_hist(path, "unitig coverage");
  if (!f) return;
  fprintf(f, "Covg,NumKmers,NumUnitigs\n");
  size_t end;
  for (end = len - 1; end > 2 && covg[end] == 0; end--) {}
  for (size_t i = 1; i <= end; i++)
    if (covg[i] > 0) fprintf(f, "%zu,%llu,%llu\n", i, (unsigned long long)covg[i], (unsigned long long)ucovg[i]);
  close_hist(f);
}

static void write_len_hist(const char *path, const uint64_t *hist, size_t len, size_t kmer_size)
{
  FILE *f = open_hist(path, "unitig length");
  if (!f) return;
  fprintf(f, "UnitigKmerLength,bp,Count\n");
  size_t end;
  for (end = len - 1; end > 1 && hist[end] == 0; end--) {}
  fprintf(f, "1,%zu,%llu\n", kmer_size, (unsigned long long)hist[1]);
  for (size_t i = 2; i <= end; i++)
    if (hist[i] > 0) fprintf(f, "%zu,%zu,%llu\n", i, kmer_size + i - 1, (unsigned long long)hist[i]);
  close_hist(f);
}

/* -x given twice */
#define ONCE(seen) do { if (seen) print_usage(clean_usage, "%s given twice", cmd); } while (0)

int ctx_clean(int argc, char **argv)
{
  const char *out_path = NULL;
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, sort_kmers = false;
  int min_keep_tip = -1, unitig_min = -1; /* < 0: default, 0: no cleaning */
  bool unitig_cleaning = false, tip_cleaning = false;
  unsigned fallback_thresh = 0, nthreads = 0, user_ncols = 0, device = 0, u = 0;
  const char *len_before = NULL, *len_after = NULL, *covg_before = NULL, *covg_after = NULL;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:t:N:ST::U::B:l:L:c:C:D:", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(clean_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': if (out_path) print_usage(clean_usage, NULL); out_path = optarg; break; /* (no "given twice" here) */
      case 'm': cmd_mem_set_memory(&mem, clean_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, clean_usage, optarg); break;
      case 'N':
        if (!parse_entire_uint(optarg, &user_ncols) || !user_ncols) print_usage(clean_usage, "%s requires an int x > 0", cmd);
        break;
      case 't': cmd_threads_arg(&nthreads, clean_usage, cmd, optarg); break;
      case 'T':
        ONCE(min_keep_tip >= 0 || tip_cleaning);
        if (optarg && !parse_entire_uint(optarg, &u)) print_usage(clean_usage, "%s requires an int x >= 0", cmd);
        min_keep_tip = optarg ? (int)u : -1;
        tip_cleaning = true;
        break;
      case 'S': ONCE(sort_kmers); sort_kmers = true; break;
      case 'U':
        ONCE(unitig_min >= 0 || unitig_cleaning);
        if (optarg && !parse_entire_uint(optarg, &u)) print_usage(clean_usage, "%s requires an int x >= 0", cmd);
        unitig_min = optarg ? (int)u : -1;
        unitig_cleaning = true;
        break;
      case 'B':
        ONCE(fallback_thresh);
        if (!parse_entire_uint(optarg, &fallback_thresh) || !fallback_thresh) print_usage(clean_usage, "%s requires an int x > 0", cmd);
        break;
      case 'l': ONCE(len_before); len_before = optarg; break;
      case 'L': ONCE(len_after); len_after = optarg; break;
      case 'c': ONCE(covg_before); covg_before = optarg; break;
      case 'C': ONCE(covg_after); covg_after = optarg; break;
      case 'D': if (!parse_entire_uint(optarg, &device)) print_usage(clean_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " clean -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (nthreads == 0) nthreads = 2;
  if (optind >= argc) print_usage(clean_usage, "Please give input graph files");

  bool doing_cleaning = unitig_cleaning || tip_cleaning;
  if (!doing_cleaning && out_path != NULL) unitig_cleaning = tip_cleaning = doing_cleaning = true; /* default cleaning */
  if (doing_cleaning && out_path == NULL) print_usage(clean_usage, "Please specify --out <out.ctx> for cleaned graph");
  if (!doing_cleaning && (covg_after || len_after))
    warn("You gave --len-after <out> / --covg-after <out> without any cleaning (set -U, --unitigs or -t, --tips)");
  if (doing_cleaning && strcmp(out_path, "-") != 0 && !force && access(out_path, F_OK) == 0)
    print_usage(clean_usage, "Output file already exists: %s", out_path);
  if (fallback_thresh && !unitig_cleaning) warn("-B, --fallback <T> without --unitigs");

  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), clean_usage, &in);
  const size_t nfiles = in.n, kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;
  if (out_path == NULL) graph_files_flatten(&in); /* stats only: one colour */
  size_t file_ncols = in.ncols;
  if (user_ncols && file_ncols < user_ncols) {
    warn("I only need %zu colour%s ('--ncols %u' ignored)", file_ncols, plural(file_ncols), user_ncols);
    user_ncols = (unsigned)file_ncols;
  }
  /* --ncols below the files' colours is the reference's low-memory path; the output is the same with every
   * colour loaded, which is what happens here */
  const size_t ncols = file_ncols;
  if (min_keep_tip < 0) min_keep_tip = 2 * (int)kmer_size;

  for (size_t i = 0; i < nfiles; i++) {
    for (size_t j = 0; j < in.files[i].nfilter; j++) {
      const uint32_t from = in.files[i].filter[j].from;
      const err_cleaning *cl = &in.files[i].ginfo[from].cleaning;
      if (cl->cleaned_unitigs && unitig_cleaning)
        warn("%s:%u already has unitig cleaning with threshold: <%u", in.files[i].path, from, cl->clean_unitigs_thresh);
      if (cl->cleaned_tips && tip_cleaning) warn("%s:%u already has had tip cleaned", in.files[i].path, from);
    }
  }

  size_t step = 0;
  status("Actions:\n");
  if (covg_before) status("%zu. Saving kmer coverage distribution to: %s", step++, covg_before);
  if (len_before) status("%zu. Saving unitig length distribution to: %s", step++, len_before);
  if (tip_cleaning) status("%zu. Cleaning tips shorter than %i nodes", step++, min_keep_tip);
  if (unitig_cleaning) {
    if (unitig_min > 0) status("%zu. Cleaning unitigs with coverage < %i", step++, unitig_min);
    if (unitig_min < 0) status("%zu. Cleaning unitigs with auto-detected threshold", step++);
  }
  if (covg_after) status("%zu. Saving kmer coverage distribution to: %s", step++, covg_after);
  if (len_after) status("%zu. Saving unitig length distribution to: %s", step++, len_after);

  /* ---- memory: as `build --graph` sizes the table for the same inputs ---- */
  const size_t bits_per_kmer = W * 64 + (4 + 1) * 8 * ncols + (sort_kmers ? 64 : 0);
  table_plan plan;
  char s1[64];
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (err) die("%s", err);
  status("[cleaning] %zu input graph%s, max kmers: %s, using %zu colour%s", nfiles, plural(nfiles), ulong_to_str(in.max_kmers, s1),
         ncols, plural(ncols));
  table_plan_status(&plan);
  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, ncols, device))) die("%s", err);

  col_info *cols = graph_files_merge_headers(&in, ncols);
  for (size_t i = 0; i < nfiles; i++) ctx_load_graph_file(g, &in.files[i]);

  uint64_t initial_nkmers = 0;
  mcx_check(mcx_graph_nkmers(g, &initial_nkmers), "nkmers");
  status("[cleaning] Total kmers loaded: %s\n", ulong_to_str(initial_nkmers, s1));
  hasht_status(g);

  /* ---- cleaning_get_threshold ---- */
  status("[cleaning] Calculating unitig stats with %u threads...", nthreads);
  status("[cleaning]   Using kmer gamma method");
  uint64_t *before = calloc(3 * MCX_CLEAN_NBINS, sizeof(uint64_t)), *after = calloc(3 * MCX_CLEAN_NBINS, sizeof(uint64_t));
  if (!before || !after) die("Out of memory");
  mcx_check(mcx_graph_unitig_stats(g, before), "unitig stats");
  if (covg_before) write_covg_hist(covg_before, before, before + MCX_CLEAN_NBINS, MCX_CLEAN_NBINS);
  if (len_before) write_len_hist(len_before, before + 2 * MCX_CLEAN_NBINS, MCX_CLEAN_NBINS, kmer_size);
  double alpha = 0, beta = 0, fp = 0, fn = 0;
  const int est = cleaning_pick_kmer_threshold(before, MCX_CLEAN_NBINS, &alpha, &beta, &fp, &fn);
  if (est < 0) warn("Cannot pick a cleaning threshold");
  else {
    status("[cleaning] alpha=%f, beta=%f FP=%f FN=%f", alpha, beta, fp, fn);
    status("[cleaning] Recommended unitig cleaning threshold: < %i", est);
  }
  if (est < 0) status("Cannot find recommended cleaning threshold");
  else status("Recommended cleaning threshold is: %i", est);
  if (unitig_min < 0) {
    if (fallback_thresh > 0 && est < (int)fallback_thresh) {
      status("Using fallback threshold: %u", fallback_thresh);
      unitig_min = (int)fallback_thresh;
    } else if (est >= 0) unitig_min = est;
  }
  if (unitig_min < 0) die("Need cleaning threshold (--unitigs=<D> or --fallback <D>)");

  /* ---- clean_graph: min_keep_tip applies even with --unitigs alone, the threshold even with --tips alone ---- */
  if (doing_cleaning && initial_nkmers > 0) {
    if (unitig_min == 0 && min_keep_tip == 0) warn("[cleaning] No cleaning specified");
    else {
      if (unitig_min > 0) {
        status("[cleaning] Removing unitigs with coverage < %i...", unitig_min);
        status("[cleaning]   Using kmer gamma method");
      }
      if (min_keep_tip > 0) status("[cleaning] Removing tips shorter than %i...", min_keep_tip);
      status("[cleaning]   using %u threads", nthreads);
      mcx_clean_stats cs;
      mcx_check(mcx_graph_clean(g, (uint32_t)unitig_min, (uint32_t)min_keep_tip, &cs, after), "clean");
      char a[50], b[50], c2[50], d[50], e[50], f[50];
      status("[cleaning] Removing %s low coverage unitigs [%s kmer%s], %s unitig tips [%s kmer%s] and %s of both [%s kmer%s]",
             ulong_to_str(cs.num_low_covg_unitigs, a), ulong_to_str(cs.num_low_covg_unitig_kmers, b), plural(cs.num_low_covg_unitig_kmers),
             ulong_to_str(cs.num_tips, c2), ulong_to_str(cs.num_tip_kmers, d), plural(cs.num_tip_kmers),
             ulong_to_str(cs.num_tip_and_low_unitigs, e), ulong_to_str(cs.num_tip_and_low_unitig_kmers, f),
             plural(cs.num_tip_and_low_unitig_kmers));
      uint64_t remain = 0;
      mcx_check(mcx_graph_nkmers(g, &remain), "nkmers");
      status("[cleaning] Remaining kmers: %s removed: %s (%.1f%%)", ulong_to_str(remain, a), ulong_to_str(initial_nkmers - remain, b),
             (100.0 * (double)(initial_nkmers - remain)) / (double)initial_nkmers);
      if (covg_after) write_covg_hist(covg_after, after, after + MCX_CLEAN_NBINS, MCX_CLEAN_NBINS);
      if (len_after) write_len_hist(len_after, after + 2 * MCX_CLEAN_NBINS, MCX_CLEAN_NBINS, kmer_size);
    }
  }

  if (out_path != NULL) {
    for (size_t i = 0; i < ncols; i++) {
      err_cleaning *cl = &cols[i].cleaning;
      cl->cleaned_unitigs |= unitig_cleaning;
      cl->cleaned_tips |= tip_cleaning;
      if (unitig_cleaning) /* (cleaned_unitigs has just been set: the maximum of the old and new thresholds) */
        cl->clean_unitigs_thresh = cl->cleaned_unitigs ? (cl->clean_unitigs_thresh > (uint32_t)unitig_min ? cl->clean_unitigs_thresh
                                                                                                             : (uint32_t)unitig_min)
                                                       : (uint32_t)unitig_min;
    }
    uint64_t nk = 0;
    mcx_check(mcx_graph_nkmers(g, &nk), "nkmers");
    char a[100], b[100];
    status("Removed %s of %s (%.2f%%) kmers", ulong_to_str(initial_nkmers - nk, a), ulong_to_str(initial_nkmers, b),
           (100.0 * (double)(initial_nkmers - nk)) / (double)initial_nkmers);
    ctx_write_graph(g, out_path, kmer_size, ncols, cols, sort_kmers);
  }

  col_infos_free(cols, ncols);
  graph_files_close(&in);
  free(before); free(after);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
