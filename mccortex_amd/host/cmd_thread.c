/* cmd_thread.c -- `mccortex<K> thread` (src/commands/ctx_thread.c, src/commands/read_thread_cmd.c) without -p and -u:
 * the reference's usage text and option table and its output file, a gzipped .ctp of format version 4: the JSON header
 * (gpath_save_mkhdr, json_hdr_make_std, correct_aln_input_json_hdr), a comment block and the links.  The graph file is
 * loaded into a table of one colour; contigs, junctions, links, their counts and the text of the body are made on the
 * MI355X (mcx_graph_thread, mcx_graph_links_text), batch by batch through the batch loop of `reads` (reads_run_tasks).
 *
 * Where this differs from the reference (DESIGN.md lists it): the k-mers of the body come in key order (the reference
 * writes them in hash-table order from racing threads); -p, -0 and -u are refused, the walker that uses links is not
 * part of this build, and so -M, -l, -L, -X, -e and -E are parsed, validated and recorded in the header and change
 * nothing (read_thread_cmd.c:173-178); --seq2 and --seqi are refused, the insert gap between mates is not built; -Q,
 * -O, -H, -g, -G, -x, -y and -z are refused by name; --device picks the GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <limits.h>
#include <pwd.h>
#include <stdlib.h>
#include <string.h>
#include <sys/utsname.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include "../../include/mcx_gpu.h"

static const char thread_usage[] =
"usage: " CMD_NAME " thread [options] <in.ctx>\n"
"\n"
"  Thread reads through the graph.  Save to file <out.ctp>.  <pop.ctx> can should\n"
"  have everyone in it and can be a pooled graph (with only 1 colour).  Samples\n"
"  are loaded from <in.ctx> files one at a time.\n"
"\n"
"  -h, --help               This help message\n"
"  -q, --quiet              Silence status output normally printed to STDERR\n"
"  -f, --force              Overwrite output files\n"
"  -o, --out <out.ctp.gz>   Save output file [required]\n"
"  -m, --memory <mem>       Memory to use (e.g. 1M, 20GB)\n"
"  -n, --nkmers <N>         Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>        Number of threads to use [default: 2]\n"
"  -p, --paths <in.ctp>     Load link file (can specify multiple times)\n"
"  -0, --zero-paths         Zero counts on initially loaded links. Use if existing\n"
"                           links were built from sequence being re-used by this run\n"
"\n"
"  Input:\n"
"  -1, --seq <in.fa>        Thread reads from file (supports sam,bam,fq,*.gz\n"
"  -2, --seq2 <in1:in2>     Thread paired end sequences\n"
"  -i, --seqi <in.bam>      Thread PE reads from a single file\n"
"  -M, --matepair <orient>  Mate pair orientation: FF,FR,RF,RR [default: FR]\n"
"  -Q, --fq-cutoff <Q>      Filter quality scores [default: 0 (off)]\n"
"  -O, --fq-offset <N>      FASTQ ASCII offset    [default: 0 (auto-detect)]\n"
"  -H, --cut-hp <bp>        Breaks reads at homopolymers >= <bp> [default: off]\n"
"  -l, --min-frag-len <bp>  Min fragment size for --seq2 [default:0]\n"
"  -L, --max-frag-len <bp>  Max fragment size for --seq2 [default:1000]\n"
"\n"
"  Link Params:\n"
"  -w, --one-way            Use one-way gap filling (conservative) [default]\n"
"  -W, --two-way            Use two-way gap filling (liberal)\n"
"  -d, --gap-diff-const <d> Set parameters for allowable gap lengths (decimals):\n"
"  -D, --gap-diff-coeff <D>   abs(gap_exp - gap_seen) <= gap_exp*D + d\n"
"  -X, --max-context        Number of kmers to use either side of a gap\n"
"  -e, --end-check          Extra check after bridging gap [default: on]\n"
"  -E, --no-end-check       Skip extra check after gap bridging\n"
"  -g, --gap-hist <o.csv>   Save size distribution of sequence gaps bridged\n"
"  -G, --frag-hist <o.csv>  Save size distribution of PE fragments\n"
"\n"
"  -u, --use-new-paths      Use links as they are being added (higher err rate) [default: no]\n"
"      --device <N>         GPU to run on [default: 0]\n"
"\n"
"  Debugging Options: Probably best not to touch these\n"
"    -x,--print-contigs -y,--print-paths -z,--print-reads\n"
"\n"
"  When loading existing links with -p, use offset (e.g. 2:in.ctp) to specify\n"
"  which colour to load the data into. See `" CMD_NAME " pjoin` to combine .ctp files\n"
"\n";

/* what a reader of the file needs to know about its lines, in this program's own words */
static const char ctp_comment[] =
"# Links written by " CMD_NAME " thread\n"
"# \n"
"# Lines that start with '#' are comments; they are allowed only below the JSON header\n"
"# Each k-mer with links has a line\n"
"#   [kmer] [number of links]\n"
"# followed by one line per link\n"
"#   [F or R] [number of junctions] [count per colour: n0,n1,...] [junction bases] [seq=... juncpos=...]\n"
"#\n"
"# Columns are separated by one space.\n"
"# The first four columns of a link line are required, the rest is optional\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},                 {"out", required_argument, NULL, 'o'},
  {"force", no_argument, NULL, 'f'},                {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'},         {"threads", required_argument, NULL, 't'},
  {"paths", required_argument, NULL, 'p'},          {"zero-paths", no_argument, NULL, '0'},
  {"seq", required_argument, NULL, '1'},            {"seq2", required_argument, NULL, '2'},
  {"seqi", required_argument, NULL, 'i'},           {"matepair", required_argument, NULL, 'M'},
  {"fq-cutoff", required_argument, NULL, 'Q'},      {"fq-offset", required_argument, NULL, 'O'},
  {"cut-hp", required_argument, NULL, 'H'},         {"min-frag-len", required_argument, NULL, 'l'},
  {"max-frag-len", required_argument, NULL, 'L'},   {"one-way", no_argument, NULL, 'w'},
  {"two-way", no_argument, NULL, 'W'},              {"gap-diff-const", required_argument, NULL, 'd'},
  {"gap-diff-coeff", required_argument, NULL, 'D'}, {"max-context", required_argument, NULL, 'X'},
  {"end-check", no_argument, NULL, 'e'},            {"no-end-check", no_argument, NULL, 'E'},
  {"gap-hist", required_argument, NULL, 'g'},       {"frag-hist", required_argument, NULL, 'G'},
  {"use-new-paths", no_argument, NULL, 'u'},        {"print-contigs", no_argument, NULL, 'x'},
  {"print-paths", no_argument, NULL, 'y'},          {"print-reads", no_argument, NULL, 'z'},
  {"device", required_argument, NULL, OPT_DEVICE},  {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(thread_usage, "%s given twice", cmd); } while (0)

/* what the options in front of a --seq set for it (CorrectAlnInput: `task` of read_thread_args_parse) */
typedef struct {
  bool two_way, end_check;
  float gap_wiggle, gap_variance;
  unsigned frag_len_min, frag_len_max, max_context;
  char matepair[3];
  double gap_wiggle_d, gap_variance_d; /* as given, for the header */
} thread_opts;

typedef struct {
  mcx_graph *g;
  const thread_opts *opts; /* [ntasks] */
  mcx_thread_stats stats;
} thread_run;

static void process(reads_run *run, reads_work *w)
{
  thread_run *T = run->user;
  const thread_opts *o = &T->opts[w->task];
  const mcx_thread_params p = {o->two_way ? MCX_THREAD_TWO_WAY : 0u, o->gap_variance, o->gap_wiggle, 0};
  mcx_check(mcx_graph_thread(T->g, w->b.bases, w->b.offsets, w->b.nreads, &p, &T->stats), "thread");
}

static bool parse_udouble(const char *s, double *out)
{
  char *end;
  const double v = strtod(s, &end);
  if (end == s || *end || !(v >= 0) || v > 3.0e38) return false;
  *out = v;
  return true;
}

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

/* gpath_save_mkhdr: the header of a .ctp file of version 4, closed by an empty line */
static void write_header(gzFile gz, const char *out_path, int argc, char **argv, size_t kmer_size, uint64_t nkmers, const col_info *col,
                         const reads_task *tasks, const thread_opts *opts, size_t ntasks, const mcx_links_info *info, const uint64_t *hist_len,
                         const uint64_t *hist_cnt, size_t nhist)
{
  char file_key[17], cmd_key[9], cwd[PATH_MAX + 1], abspath[PATH_MAX + 1], date[50], user[1025] = "noname";
  ctp_hex_key(file_key, 16);
  ctp_hex_key(cmd_key, 8);
  if (!getcwd(cwd, sizeof(cwd))) strcpy(cwd, ".");
  if (!realpath(out_path, abspath)) snprintf(abspath, sizeof(abspath), "%s", out_path);
  const time_t now = time(NULL);
  strftime(date, sizeof(date), "%Y-%m-%d %H:%M:%S", localtime(&now));
  gzputs(gz, "{\n  \"file_format\": \"ctp\",\n  \"format_version\": 4,\n  \"file_key\": ");
  ctp_put_str(gz, file_key);
  gzprintf(gz, ",\n  \"graph\": {\n    \"num_colours\": 1,\n    \"kmer_size\": %zu,\n    \"num_kmers_in_graph\": %llu,\n    \"colours\": [{\n", kmer_size,
           (unsigned long long)nkmers);
  gzputs(gz, "        \"colour\": 0,\n        \"sample\": ");
  ctp_put_str(gz, col->name ? col->name : "undefined");
  gzprintf(gz, ",\n        \"total_sequence\": %llu,\n        \"cleaned_tips\": %s,\n", (unsigned long long)col->total_sequence,
           col->cleaning.cleaned_tips ? "true" : "false");
  if (col->cleaning.cleaned_unitigs) gzprintf(gz, "        \"cleaned_unitigs\": %u\n", col->cleaning.clean_unitigs_thresh);
  else gzputs(gz, "        \"cleaned_unitigs\": false\n");
  gzputs(gz, "      }]\n  },\n  \"commands\": [{\n      \"key\": ");
  ctp_put_str(gz, cmd_key);
  gzputs(gz, ",\n      \"cmd\": [");
  ctp_put_str(gz, CMD_NAME);
  for (int i = 0; i < argc; i++) { gzputs(gz, ", "); ctp_put_str(gz, argv[i]); }
  gzputs(gz, "],\n      \"cwd\": ");
  ctp_put_str(gz, cwd);
  gzputs(gz, ",\n      \"out_path\": ");
  ctp_put_str(gz, abspath);
  gzputs(gz, ",\n      \"out_key\": ");
  ctp_put_str(gz, file_key);
  gzputs(gz, ",\n      \"date\": ");
  ctp_put_str(gz, date);
  gzputs(gz, ",\n      \"mccortex\": \"" CMD_NAME " on libmcxgpu\",\n      \"zlib\": ");
  ctp_put_str(gz, zlibVersion());
  struct passwd pwd, *res = NULL;
  char pwbuf[4096];
  if (getpwuid_r(geteuid(), &pwd, pwbuf, sizeof(pwbuf), &res) == 0 && res) snprintf(user, sizeof(user), "%s", res->pw_name);
  gzputs(gz, ",\n      \"user\": ");
  ctp_put_str(gz, user);
  struct utsname sys;
  if (uname(&sys) != -1) {
    const char *const names[5] = {"host", "os", "osrelease", "osversion", "hardware"};
    const char *const vals[5] = {sys.nodename, sys.sysname, sys.release, sys.version, sys.machine};
    for (int i = 0; i < 5; i++) { gzprintf(gz, ",\n      \"%s\": ", names[i]); ctp_put_str(gz, vals[i]); }
  }
  gzputs(gz, ",\n      \"prev\": [],\n      \"thread\": {\n        \"inputs\": [");
  for (size_t i = 0; i < ntasks; i++) { /* correct_aln_input_json_hdr */
    const thread_opts *o = &opts[i];
    gzputs(gz, i ? ", {\n" : "{\n");
    gzputs(gz, "            \"files\": [");
    ctp_put_str(gz, seq_in_path(tasks[i].f1));
    gzprintf(gz, "],\n            \"interleaved\": false,\n            \"fq_offset\": 0,\n            \"fq_cutoff\": 0,\n            \"hp_cutoff\": 0,\n"
             "            \"matepair\": \"%s\",\n            \"frag_len_min_bp\": %u,\n            \"frag_len_max_bp\": %u,\n"
             "            \"one_way_gap_fill\": %s,\n            \"use_end_check\": %s,\n            \"max_context\": %u,\n"
             "            \"gap_variance\": %.17g,\n            \"gap_wiggle\": %.17g\n          }",
             o->matepair, o->frag_len_min, o->frag_len_max, o->two_way ? "false" : "true", o->end_check ? "true" : "false", o->max_context,
             o->gap_variance_d, o->gap_wiggle_d);
  }
  gzprintf(gz, "]\n      }\n    }],\n  \"paths\": {\n    \"num_kmers_with_paths\": %llu,\n    \"num_paths\": %llu,\n    \"path_bytes\": %llu,\n"
           "    \"contig_hists\": [{\n        \"lengths\": [", (unsigned long long)info->num_kmers_with_paths, (unsigned long long)info->num_paths,
           (unsigned long long)info->path_bytes);
  for (size_t i = 0; i < nhist; i++) gzprintf(gz, "%s%llu", i ? ", " : "", (unsigned long long)hist_len[i]);
  gzputs(gz, "],\n        \"counts\": [");
  for (size_t i = 0; i < nhist; i++) gzprintf(gz, "%s%llu", i ? ", " : "", (unsigned long long)hist_cnt[i]);
  gzputs(gz, "]\n      }]\n  }\n}\n\n");
}

int ctx_thread(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, used = true;
  unsigned nthreads = 0, device = 0;
  const char *out_path = NULL;
  thread_opts cur = {false, true, 5.0f, 0.1f, 0, 1000, 200, "FR", 5.0, 0.1};
  reads_task *tasks = NULL;
  thread_opts *topts = NULL;
  size_t ntasks = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:t:p:01:2:i:M:Q:O:H:l:L:wWd:D:X:eEg:G:uxyz", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(thread_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 't': cmd_threads_arg(&nthreads, thread_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, thread_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, thread_usage, optarg); break;
      case 'p': die("-p, --paths <in.ctp>: the walker that uses links is not part of this build; `thread` makes links from the graph and the reads alone");
      case '0': die("-0, --zero-paths has no meaning without -p, --paths <in.ctp>, which is not part of this build");
      case 'u': die("-u, --use-new-paths: the walker that uses links is not part of this build");
      case '2': die("-2, --seq2 <in1:in2>: the insert gap between mates is not built; give each mate's file as --seq");
      case 'i': die("-i, --seqi <in.bam>: the insert gap between mates is not built; give the reads as --seq");
      case 'Q': die("-Q, --fq-cutoff <Q> is not part of this build's `thread`");
      case 'O': die("-O, --fq-offset <N> is not part of this build's `thread`");
      case 'H': die("-H, --cut-hp <bp> is not part of this build's `thread`");
      case 'g': die("-g, --gap-hist <o.csv> is not part of this build's `thread`");
      case 'G': die("-G, --frag-hist <o.csv> is not part of this build's `thread`");
      case 'x': die("-x, --print-contigs is not part of this build's `thread`");
      case 'y': die("-y, --print-paths is not part of this build's `thread`");
      case 'z': die("-z, --print-reads is not part of this build's `thread`");
      case '1':
        used = true;
        tasks = realloc(tasks, (ntasks + 1) * sizeof(*tasks));
        topts = realloc(topts, (ntasks + 1) * sizeof(*topts));
        if (!tasks || !topts) die("Out of memory");
        topts[ntasks] = cur;
        memset(&tasks[ntasks], 0, sizeof(*tasks));
        tasks[ntasks].kind = '1';
        if (!(tasks[ntasks].f1 = seq_in_open(optarg))) die("Cannot open -1 file: %s", optarg);
        ntasks++;
        break;
      case 'M':
        if (strcmp(optarg, "FF") && strcmp(optarg, "FR") && strcmp(optarg, "RF") && strcmp(optarg, "RR"))
          print_usage(thread_usage, "-M,--matepair <orient> must be one of: FF,FR,RF,RR");
        memcpy(cur.matepair, optarg, 3);
        used = false; break;
      case 'l': if (!parse_entire_uint(optarg, &cur.frag_len_min)) print_usage(thread_usage, "%s requires an int x >= 0: %s", cmd, optarg); used = false; break;
      case 'L': if (!parse_entire_uint(optarg, &cur.frag_len_max)) print_usage(thread_usage, "%s requires an int x >= 0: %s", cmd, optarg); used = false; break;
      case 'w': cur.two_way = false; used = false; break;
      case 'W': cur.two_way = true; used = false; break;
      case 'd':
        if (!parse_udouble(optarg, &cur.gap_wiggle_d)) print_usage(thread_usage, "%s requires a double x >= 0: %s", cmd, optarg);
        cur.gap_wiggle = (float)cur.gap_wiggle_d; used = false; break;
      case 'D':
        if (!parse_udouble(optarg, &cur.gap_variance_d)) print_usage(thread_usage, "%s requires a double x >= 0: %s", cmd, optarg);
        cur.gap_variance = (float)cur.gap_variance_d; used = false; break;
      case 'X': if (!parse_entire_uint(optarg, &cur.max_context)) print_usage(thread_usage, "%s requires an int x >= 0: %s", cmd, optarg); used = false; break;
      case 'e': cur.end_check = true; used = false; break;
      case 'E': cur.end_check = false; used = false; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(thread_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " thread/correct -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (nthreads == 0) nthreads = 2;
  if (optind + 1 > argc) print_usage(thread_usage, "Expected exactly one graph file");
  else if (optind + 1 < argc) print_usage(thread_usage, "Expected only one graph file. What is this: '%s'", argv[optind]);
  if (!used) print_usage(thread_usage, "Ignored arguments after last --seq");
  if (!out_path) print_usage(thread_usage, "--out <out.ctp> is required");
  for (size_t i = 0; i < ntasks; i++)
    if (topts[i].frag_len_min > topts[i].frag_len_max) die("--min-ins %u is greater than --max-ins %u", topts[i].frag_len_min, topts[i].frag_len_max);

  graph_files in;
  graph_files_open(argv + optind, 1, thread_usage, &in);
  if (in.ncols > 1) die("Please specify a single colour e.g. %s:0", in.files[0].path);
  const size_t kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;
  col_info *cols = graph_files_merge_headers(&in, 1);

  /* kmer memory = kmer + coverage + edges of the one colour */
  const size_t bits_per_kmer = 64 * W + 40;
  table_plan plan;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (err) die("%s", err);
  table_plan_status(&plan);

  /* futil_gzopen_create: an existing file is kept unless --force */
  const bool to_stdout = strcmp(out_path, "-") == 0;
  if (!to_stdout && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);
  gzFile gz = to_stdout ? gzdopen(dup(STDOUT_FILENO), "w") : gzopen(out_path, "w");
  if (!gz) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  status("Creating paths file: %s", outpath(out_path));

  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, 1, device))) {
    gzclose(gz);
    if (!to_stdout) unlink(out_path);
    die("%s", err);
  }
  ctx_load_graph_file(g, &in.files[0]);
  ctx_reader_close(&in.files[0]);
  free(in.files);
  hasht_status(g);
  status("Not using new paths as they are added (safe)");

  thread_run T;
  memset(&T, 0, sizeof(T));
  T.g = g; T.opts = topts;
  reads_run R;
  memset(&R, 0, sizeof(R));
  R.tasks = tasks; R.ntasks = ntasks;
  R.want_quals = false;
  R.process = process; R.user = &T;
  reads_run_tasks(&R, nthreads);

  mcx_links_info info;
  uint64_t nhist = 0, nkmers = 0, *hist = NULL;
  mcx_check(mcx_graph_links_info(g, &info), "thread");
  mcx_check(mcx_graph_links_contig_hist(g, NULL, NULL, 0, &nhist), "thread");
  hist = malloc((2 * nhist + 1) * sizeof(*hist));
  if (!hist) die("Out of memory");
  mcx_check(mcx_graph_links_contig_hist(g, hist, hist + nhist, nhist, &nhist), "thread");
  mcx_check(mcx_graph_nkmers(g, &nkmers), "thread");

  const mcx_thread_stats *s = &T.stats;
  char n[6][32];
  status("[GenPaths] %s reads: %s aligned perfectly, %s with no k-mer in the sample", ulong_to_str(s->aln.num_reads, n[0]),
         ulong_to_str(s->aln.num_perfect, n[1]), ulong_to_str(s->aln.num_no_kmers, n[2]));
  status("[GenPaths] gaps: %s, filled %s (%s by the backward walk), too short %s, too long or stopped %s; missing edges: %s",
         ulong_to_str(s->aln.gaps, n[0]), ulong_to_str(s->aln.gaps_filled, n[1]), ulong_to_str(s->aln.gaps_filled_backward, n[2]),
         ulong_to_str(s->aln.gaps_too_short, n[3]), ulong_to_str(s->aln.gaps_too_long_or_stopped, n[4]), ulong_to_str(s->aln.missing_edges, n[5]));
  status("[GenPaths] contigs: %s of %s k-mers; junctions: %s forward, %s reverse", ulong_to_str(s->contigs, n[0]), ulong_to_str(s->contig_kmers, n[1]),
         ulong_to_str(s->juncs_fw, n[2]), ulong_to_str(s->juncs_rv, n[3]));
  status("[GenPaths] links generated: %s; kept: %s on %s k-mers, %s of junction bases", ulong_to_str(s->links_added, n[0]),
         ulong_to_str(info.num_paths, n[1]), ulong_to_str(info.num_kmers_with_paths, n[2]), bytes_to_str(info.path_bytes, 1, n[3]));

  write_header(gz, out_path, argc, argv, kmer_size, nkmers, &cols[0], tasks, topts, ntasks, &info, hist, hist + nhist, (size_t)nhist);
  gzputs(gz, ctp_comment);
  mcx_check(mcx_graph_links_text(g, MCX_LINKS_SEQ, gz_sink, gz), "thread");
  if (gzclose(gz) != Z_OK) die("Cannot write to file: %s", outpath(out_path));
  status("Saved %s links on %s k-mers to %s", ulong_to_str(info.num_paths, n[0]), ulong_to_str(info.num_kmers_with_paths, n[1]), outpath(out_path));

  for (size_t i = 0; i < ntasks; i++) seq_in_close(tasks[i].f1);
  col_infos_free(cols, 1);
  free(hist);
  free(tasks);
  free(topts);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
