/* cmd_correct.c -- `mccortex<K> correct` (src/commands/ctx_correct.c, src/commands/read_thread_cmd.c) without link
 * files: the reference's usage text and option table, its output files and record layout.  The graph file is loaded
 * with its colours as they are; the walks over the union of the colours' edges and the sample test in colour -c are
 * made on the MI355X (mcx_graph_correct), batch by batch through the batch loop of `reads` (reads_run_tasks).
 *
 * Where this differs from the reference (DESIGN.md lists it): -p is refused, links are not part of this build, and so
 * -M, -l, -L, -X, -e and -E are parsed and validated and change nothing (read_thread_cmd.c:173-178 forces max_context
 * to 1 without links, graph_walker_agrees_contig holds when no paths are held, and the two mates of a pair are
 * corrected on their own, correct_reads.c:310-313); -Q, -O, -H, -g, -G and -C are refused by name; the records are
 * written in input order (the reference's workers write in whatever order they finish); a quality that the input did
 * not give is written as the --fq-zero character; --device picks the GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "../../include/mcx_gpu.h"

static const char correct_usage[] =
"usage: " CMD_NAME " correct [options] <input.ctx>\n"
"\n"
"  Correct reads against a (population) graph. Uses paths if specified.\n"
"  Bases are printed in lower case if they cannot be corrected.\n"
"\n"
"  -h, --help               This help message\n"
"  -q, --quiet              Silence status output normally printed to STDERR\n"
"  -f, --force              Overwrite output files\n"
"  -m, --memory <mem>       Memory to use (e.g. 1M, 20GB)\n"
"  -n, --nkmers <N>         Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>        Number of threads to use [default: 2]\n"
"  -p, --paths <in.ctp>     Load link file (can specify multiple times)\n"
"\n"
"  Input:\n"
"  -1, --seq <in:out>       Correct reads (output: <out>.fa.gz)\n"
"  -2, --seq2 <in1:in2:out> Correct reads (output: <out>{,.1,.2}.fa.gz)\n"
"  -i, --seqi <in.bam:out>  Correct reads (output: <out>{,.1,.2}.fa.gz)\n"
"  -F, --format <f>         Output format may be: FASTA or FASTQ\n"
"  -M, --matepair <orient>  Mate pair orientation: FF,FR,RF,RR [default: FR]\n"
"  -Q, --fq-cutoff <Q>      Filter quality scores [default: 0 (off)]\n"
"  -O, --fq-offset <N>      FASTQ ASCII offset    [default: 0 (auto-detect)]\n"
"  -H, --cut-hp <bp>        Breaks reads at homopolymers >= <bp> [default: off]\n"
"  -l, --min-frag-len <bp>  Min fragment size for --seq2 [default:0]\n"
"  -L, --max-frag-len <bp>  Max fragment size for --seq2 [default:1000]\n"
"\n"
"  Correction:\n"
"  -w, --one-way            Use one-way gap filling (conservative)\n"
"  -W, --two-way            Use two-way gap filling (liberal)\n"
"  -d, --gap-diff-const <d> Set parameters for allowable gap lengths (decimals):\n"
"  -D, --gap-diff-coeff <D>   abs(gap_exp - gap_seen) <= gap_exp*D + d\n"
"  -X, --max-context        Number of kmers to use either side of a gap\n"
"  -e, --end-check          Extra check after bridging gap [default: on]\n"
"  -E, --no-end-check       Skip extra check after gap bridging\n"
"  -Z, --fq-zero <char>     Replace zero'd quality score with character <char>\n"
"  -P, --print-orig         Print original sequence in the read name ('orig=SEQ')\n"
"  -g, --gap-hist <o.csv>   Save size distribution of sequence gaps bridged\n"
"  -G, --frag-hist <o.csv>  Save size distribution of PE fragments\n"
"  -C, --contig-hist <.csv> Save size distribution of assembled contigs\n"
"\n"
"  -c, --colour <col>       Sample graph colour to correct against\n"
"      --device <N>         GPU to run on [default: 0]\n"
"\n"
"  Output is <O>.fq.gz for FASTQ, <O>.fa.gz for FASTA, <O>.txt.gz for plain\n"
"  --seq outputs <out>.fa.gz, --seq2 outputs <out>.1.fa.gz, <out>.2.fa.gz\n"
"  --seq must come AFTER two/oneway options. Output is in input order.\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},                 {"memory", required_argument, NULL, 'm'},
  {"nkmers", required_argument, NULL, 'n'},         {"threads", required_argument, NULL, 't'},
  {"paths", required_argument, NULL, 'p'},          {"force", no_argument, NULL, 'f'},
  {"seq", required_argument, NULL, '1'},            {"seq2", required_argument, NULL, '2'},
  {"seqi", required_argument, NULL, 'i'},           {"matepair", required_argument, NULL, 'M'},
  {"format", required_argument, NULL, 'F'},         {"fq-cutoff", required_argument, NULL, 'Q'},
  {"fq-offset", required_argument, NULL, 'O'},      {"cut-hp", required_argument, NULL, 'H'},
  {"min-frag-len", required_argument, NULL, 'l'},   {"max-frag-len", required_argument, NULL, 'L'},
  {"one-way", no_argument, NULL, 'w'},              {"two-way", no_argument, NULL, 'W'},
  {"gap-diff-const", required_argument, NULL, 'd'}, {"gap-diff-coeff", required_argument, NULL, 'D'},
  {"max-context", required_argument, NULL, 'X'},    {"end-check", no_argument, NULL, 'e'},
  {"no-end-check", no_argument, NULL, 'E'},         {"fq-zero", required_argument, NULL, 'Z'},
  {"print-orig", no_argument, NULL, 'P'},           {"gap-hist", required_argument, NULL, 'g'},
  {"frag-hist", required_argument, NULL, 'G'},      {"contig-hist", required_argument, NULL, 'C'},
  {"col", required_argument, NULL, 'c'},            {"color", required_argument, NULL, 'c'}, /* (cmd_optname names the last) */
  {"colour", required_argument, NULL, 'c'},         {"device", required_argument, NULL, OPT_DEVICE},
  {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(correct_usage, "%s given twice", cmd); } while (0)

/* what the options in front of a --seq set for it (CorrectAlnInput: `task` of read_thread_args_parse) */
typedef struct {
  bool two_way;
  float gap_wiggle, gap_variance;
  unsigned frag_len_min, frag_len_max;
} correct_opts;

typedef struct {
  mcx_graph *g;
  const correct_opts *opts; /* [ntasks] */
  unsigned colour;
  char fq_zero;
  bool print_orig, want_quals;
  mcx_correct_stats stats;
  uint64_t *out_off;
  size_t cap_off;
  char *rec, *orig;
  size_t nrec, cap_rec, cap_orig;
} correct_run;

static int rec_sink(void *ctx, const void *data, size_t nbytes)
{
  correct_run *C = ctx;
  if (C->nrec + nbytes > C->cap_rec) {
    size_t cap = C->cap_rec ? C->cap_rec : (1u << 20);
    while (cap < C->nrec + nbytes) cap *= 2;
    char *p = realloc(C->rec, cap);
    if (!p) return 1;
    C->rec = p; C->cap_rec = cap;
  }
  memcpy(C->rec + C->nrec, data, nbytes);
  C->nrec += nbytes;
  return 0;
}

/* correct_read over one batch: the device corrects, the records go out in input order (handle_read:245-267) */
static void process(reads_run *run, reads_work *w)
{
  correct_run *C = run->user;
  const read_batch *b = &w->b;
  const size_t n = b->nreads;
  reads_task *t = &run->tasks[w->task];
  const correct_opts *o = &C->opts[w->task];
  if (n + 1 > C->cap_off) {
    C->cap_off = 2 * (n + 1);
    C->out_off = realloc(C->out_off, C->cap_off * sizeof(*C->out_off));
    if (!C->out_off) die("Out of memory");
  }
  const bool quals = C->want_quals && b->quals;
  const mcx_correct_params p = {C->colour, o->two_way ? MCX_CORRECT_TWO_WAY : 0u, o->gap_variance, o->gap_wiggle, C->fq_zero};
  C->nrec = 0;
  mcx_check(mcx_graph_correct(C->g, b->bases, quals ? b->quals : NULL, b->offsets, n, &p, rec_sink, C, C->out_off, &C->stats), "correct");
  if (C->nrec != C->out_off[n]) die("correct: %zu bytes of records for %llu expected", C->nrec, (unsigned long long)C->out_off[n]);
  for (size_t i = 0; i < n; i++) {
    int which = 0;
    if (w->mate && w->mate[i]) which = 1;
    else if (w->mate && i && w->mate[i - 1]) which = 2;
    const size_t at = (size_t)b->offsets[i], len = (size_t)(b->offsets[i + 1] - b->offsets[i]);
    const size_t bytes = (size_t)(C->out_off[i + 1] - C->out_off[i]), slen = quals ? bytes / 2 : bytes;
    const uint8_t *seq = (const uint8_t *)C->rec + C->out_off[i];
    size_t elen = 0;
    if (C->print_orig) {
      if (len + 7 > C->cap_orig) {
        C->cap_orig = 2 * (len + 7);
        C->orig = realloc(C->orig, C->cap_orig);
        if (!C->orig) die("Out of memory");
      }
      memcpy(C->orig, " orig=", 6);
      memcpy(C->orig + 6, b->bases + at, len);
      elen = len + 6;
    }
    seq_out_print_parts(t->out, which, b->names + b->name_off[i], (size_t)(b->name_off[i + 1] - b->name_off[i]), C->print_orig ? C->orig : NULL, elen,
                        seq, slen, quals ? seq + slen : NULL, C->fq_zero);
    t->printed++;
  }
}

static bool parse_udouble(const char *s, float *out)
{
  char *end;
  const double v = strtod(s, &end);
  if (end == s || *end || !(v >= 0) || v > 3.0e38) return false;
  *out = (float)v;
  return true;
}

int ctx_correct(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, print_orig = false, used = true;
  unsigned nthreads = 0, device = 0, colour = 0, u;
  char fq_zero = 0;
  seq_fmt fmt = SEQ_FMT_FASTQ;
  correct_opts cur = {false, 5.0f, 0.1f, 0, 1000};
  reads_task *tasks = NULL;
  correct_opts *topts = NULL;
  size_t ntasks = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "hm:n:t:p:f1:2:i:M:F:Q:O:H:l:L:wWd:D:X:eEZ:Pg:G:C:c:", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(correct_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 't': cmd_threads_arg(&nthreads, correct_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, correct_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, correct_usage, optarg); break;
      case 'p': die("-p, --paths <in.ctp>: link files are not part of this build; `correct` runs without links");
      case 'Q': die("-Q, --fq-cutoff <Q> is not part of this build's `correct`");
      case 'O': die("-O, --fq-offset <N> is not part of this build's `correct`");
      case 'H': die("-H, --cut-hp <bp> is not part of this build's `correct`");
      case 'g': die("-g, --gap-hist <o.csv> is not part of this build's `correct`");
      case 'G': die("-G, --frag-hist <o.csv> is not part of this build's `correct`");
      case 'C': die("-C, --contig-hist <.csv> is not part of this build's `correct`");
      case 'c': if (!parse_entire_uint(optarg, &colour)) print_usage(correct_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case 'F':
        ONCE(fmt != SEQ_FMT_FASTQ);
        if (!strcasecmp(optarg, "fq") || !strcasecmp(optarg, "fastq")) fmt = SEQ_FMT_FASTQ;
        else if (!strcasecmp(optarg, "fa") || !strcasecmp(optarg, "fasta")) fmt = SEQ_FMT_FASTA;
        else if (!strcasecmp(optarg, "plain") || !strcasecmp(optarg, "txt")) fmt = SEQ_FMT_PLAIN;
        else print_usage(correct_usage, "Invalid %s {FASTA,FASTQ,PLAIN} option: %s", cmd, optarg);
        break;
      case '1': case '2': case 'i':
        used = true;
        tasks = realloc(tasks, (ntasks + 1) * sizeof(*tasks));
        topts = realloc(topts, (ntasks + 1) * sizeof(*topts));
        if (!tasks || !topts) die("Out of memory");
        topts[ntasks] = cur;
        reads_task_parse(&tasks[ntasks++], c, optarg);
        break;
      case 'M':
        if (strcmp(optarg, "FF") && strcmp(optarg, "FR") && strcmp(optarg, "RF") && strcmp(optarg, "RR"))
          print_usage(correct_usage, "-M,--matepair <orient> must be one of: FF,FR,RF,RR");
        used = false; break;
      case 'l': if (!parse_entire_uint(optarg, &cur.frag_len_min)) print_usage(correct_usage, "%s requires an int x >= 0: %s", cmd, optarg); used = false; break;
      case 'L': if (!parse_entire_uint(optarg, &cur.frag_len_max)) print_usage(correct_usage, "%s requires an int x >= 0: %s", cmd, optarg); used = false; break;
      case 'w': cur.two_way = false; used = false; break;
      case 'W': cur.two_way = true; used = false; break;
      case 'd': if (!parse_udouble(optarg, &cur.gap_wiggle)) print_usage(correct_usage, "%s requires a double x >= 0: %s", cmd, optarg); used = false; break;
      case 'D': if (!parse_udouble(optarg, &cur.gap_variance)) print_usage(correct_usage, "%s requires a double x >= 0: %s", cmd, optarg); used = false; break;
      case 'X': if (!parse_entire_uint(optarg, &u)) print_usage(correct_usage, "%s requires an int x >= 0: %s", cmd, optarg); used = false; break;
      case 'e': case 'E': used = false; break;
      case 'Z':
        ONCE(fq_zero);
        if (strlen(optarg) != 1) print_usage(correct_usage, "--fq-zero <c> requires a single char");
        fq_zero = optarg[0];
        break;
      case 'P': ONCE(print_orig); print_orig = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(correct_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " thread/correct -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (nthreads == 0) nthreads = 2;
  if (optind + 1 > argc) print_usage(correct_usage, "Expected exactly one graph file");
  else if (optind + 1 < argc) print_usage(correct_usage, "Expected only one graph file. What is this: '%s'", argv[optind]);
  if (!used) print_usage(correct_usage, "Ignored arguments after last --seq");
  for (size_t i = 0; i < ntasks; i++)
    if (topts[i].frag_len_min > topts[i].frag_len_max) die("--min-ins %u is greater than --max-ins %u", topts[i].frag_len_min, topts[i].frag_len_max);

  graph_files in;
  graph_files_open(argv + optind, 1, correct_usage, &in);
  const size_t ncols = in.ncols, kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;
  if (colour >= ncols) die("-c, --colour %u: the graph has %zu colour%s", colour, ncols, ncols == 1 ? "" : "s");

  /* every output before anything is loaded; on a failure nothing of this run stays behind */
  for (size_t i = 0; i < ntasks; i++) {
    tasks[i].out = seq_out_open(tasks[i].out_base, fmt, tasks[i].kind != '1', force);
    if (!tasks[i].out) {
      for (size_t j = 0; j < i; j++) seq_out_close(tasks[j].out, true);
      die("Error creating output files");
    }
  }

  /* kmer memory = kmer + (coverage + edges) per colour: the file is loaded as it is */
  const size_t bits_per_kmer = 64 * W + 40 * ncols;
  table_plan plan;
  mcx_graph *g = NULL;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (!err) {
    table_plan_status(&plan);
    err = graph_table_create(&g, &plan, kmer_size, ncols, device);
  }
  if (err) {
    for (size_t j = 0; j < ntasks; j++) seq_out_close(tasks[j].out, true);
    die("%s", err);
  }
  for (size_t i = 0; i < in.n; i++) { ctx_load_graph_file(g, &in.files[i]); ctx_reader_close(&in.files[i]); }
  free(in.files);
  hasht_status(g);

  correct_run C;
  memset(&C, 0, sizeof(C));
  C.g = g; C.opts = topts; C.colour = colour;
  C.fq_zero = fq_zero ? fq_zero : '.';
  C.print_orig = print_orig;
  C.want_quals = fmt == SEQ_FMT_FASTQ;
  reads_run R;
  memset(&R, 0, sizeof(R));
  R.tasks = tasks; R.ntasks = ntasks;
  R.want_quals = C.want_quals;
  R.process = process; R.user = &C;
  reads_run_tasks(&R, nthreads);

  for (size_t i = 0; i < ntasks; i++) {
    seq_out_close(tasks[i].out, false);
    seq_in_close(tasks[i].f1);
    if (tasks[i].f2) seq_in_close(tasks[i].f2);
  }
  const mcx_correct_stats *s = &C.stats;
  char a[64], b[64];
  status("[CorrectReads] %s reads: %s aligned perfectly, %s with no k-mer in the sample", ulong_to_str(s->num_reads, a),
         ulong_to_str(s->num_perfect, b), ulong_to_str(s->num_no_kmers, cmd));
  status("[CorrectReads] gaps: %s, filled %s (%s by the backward walk), too short %s, too long or stopped %s", ulong_to_str(s->gaps, a),
         ulong_to_str(s->gaps_filled, b), ulong_to_str(s->gaps_filled_backward, cmd), ulong_to_str(s->gaps_too_short, cmd + 32),
         ulong_to_str(s->gaps_too_long_or_stopped, cmd + 64));
  status("[CorrectReads] ends: %s, extended %s; missing edges: %s; bases filled: %s", ulong_to_str(s->end_gaps, a),
         ulong_to_str(s->end_gaps_extended, b), ulong_to_str(s->missing_edges, cmd), ulong_to_str(s->bases_filled, cmd + 32));
  free(tasks);
  free(topts);
  free(C.out_off);
  free(C.rec);
  free(C.orig);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
