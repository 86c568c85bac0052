/* cmd_reads.c -- `mccortex<K> reads` (src/commands/ctx_reads.c): same options, messages and output files.  The graphs
 * are flattened into colour 0 of a one-colour table in HBM, as `unitigs` loads them; which reads share a k-mer with it
 * is decided on the MI355X (mcx_graph_reads_touch), batch by batch, while a reader thread parses the next batch.
 *
 * Where this differs from the reference (DESIGN.md lists it): the survivors are written in input order (the reference's
 * workers write in whatever order they finish); read names come from this repository's own parser under the published
 * rules of the seq_file library; --device picks the GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <getopt.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "../../include/mcx_gpu.h"

#define READS_BATCH_BASES (32UL << 20) /* of build's order: bases per device call */

static const char reads_usage[] =
"usage: " CMD_NAME " reads [options] <in.ctx>[:cols] [in2.ctx ...]\n"
"\n"
"  Filters reads based on which have a kmer in the graph. \n"
"\n"
"  -h, --help                  This help message\n"
"  -q, --quiet                 Silence status output normally printed to STDERR\n"
"  -f, --force                 Overwrite output files\n"
"  -m, --memory <mem>          Memory to use\n"
"  -n, --nkmers <kmers>        Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>           Number of threads to use [default: 2]\n"
"  -F, --format <f>            Output format may be: FASTA, FASTQ [default: FASTQ]\n"
"  -v, --invert                Print reads/read pairs with no kmer in graph\n"
"  -1, --seq  <in>:<O>         Writes output to <O>.fq.gz\n"
"  -2, --seq2 <in1>:<in2>:<O>  Writes output to <O>.{1,2}.fq.gz\n"
"  -i, --seqi <in>:<O>         Writes output to <O>.{1,2}.fq.gz\n"
"      --device <N>            GPU to run on [default: 0]\n"
"\n"
"  Output is <O>.fq.gz for FASTQ, <O>.fa.gz for FASTA, <O>.txt.gz for plain\n"
"  Paired reads are saved to e.g. <O>.1.fq.gz, <O>.2.fq.gz, and unpaired reads\n"
"  to <O>.fq.gz.\n"
"\n"
"  User can specify --seq/--seq2/--seqi multiple times. If either read of a\n"
"  pair touches the graph, both are printed.\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},         {"force", no_argument, NULL, 'f'},
  {"memory", required_argument, NULL, 'm'}, {"nkmers", required_argument, NULL, 'n'},
  {"threads", required_argument, NULL, 't'}, {"format", required_argument, NULL, 'F'},
  {"invert", no_argument, NULL, 'v'},       {"seq", required_argument, NULL, '1'},
  {"seq2", required_argument, NULL, '2'},   {"seqi", required_argument, NULL, 'i'},
  {"device", required_argument, NULL, OPT_DEVICE},
  {NULL, 0, NULL, 0}};

/* -x given twice */
#define ONCE(seen) do { if (seen) print_usage(reads_usage, "%s given twice", cmd); } while (0)

/* asyncio_task_parse: <in>:<O> or <in1>:<in2>:<O>, split on ':' or, when there is none, on ',' */
void reads_task_parse(reads_task *t, int c, const char *arg)
{
  memset(t, 0, sizeof(*t));
  t->kind = c;
  char *s = strdup(arg), *paths[4];
  if (!s) die("Out of memory");
  const char sep = strchr(s, ':') ? ':' : ',';
  size_t n = 0;
  for (char *p = s; n < 4;) {
    paths[n++] = p;
    if (!(p = strchr(p, sep))) break;
    *p++ = '\0';
  }
  const bool pe = c == '2';
  if (n != (pe ? 3u : 2u)) die("Expected -%c %s:<out>", (char)c, pe ? "<in1>:<in2>" : "<in>");
  t->out_base = paths[pe ? 2 : 1];
  if (pe) {
    if (!(t->f1 = seq_in_open(paths[0]))) die("Cannot open %c file: %s", (char)c, paths[0]);
    if (!(t->f2 = seq_in_open(paths[1]))) die("Cannot open %c file: %s", (char)c, paths[1]);
  } else if (!(t->f1 = seq_in_open(paths[0]))) {
    die("Cannot open -%c file: %s", (char)c, paths[0]);
  }
  /* (s stays allocated: out_base points into it) */
}

/* ---- batches on their way from the reader to the device (reads_run, host.h) ---- */
typedef reads_work work;

/* what `reads` does with a batch */
typedef struct {
  mcx_graph *g;
  bool invert;
  mcx_touch_stats stats;
  size_t total_reads;
  uint8_t *hit;
  size_t cap_hit;
} reads_filter;

static work *work_new(reads_run *R, size_t task)
{
  work *w = calloc(1, sizeof(*w));
  if (!w) die("Out of memory");
  read_batch_init(&w->b, R->want_quals);
  read_batch_keep_names(&w->b);
  w->task = task;
  return w;
}

static void work_free(work *w)
{
  read_batch_free(&w->b);
  free(w->mate);
  free(w);
}

/* filter_reads over one batch: the device says which reads touch the graph, the survivors go out in input order */
static void process(reads_run *run, work *w)
{
  reads_filter *R = run->user;
  const size_t n = w->b.nreads;
  reads_task *t = &run->tasks[w->task];
  if (n > R->cap_hit) {
    R->cap_hit = n * 2;
    R->hit = realloc(R->hit, R->cap_hit);
    if (!R->hit) die("Out of memory");
  }
  mcx_check(mcx_graph_reads_touch(R->g, w->b.bases, w->b.offsets, n, R->hit, &R->stats), "reads");
  for (size_t i = 0; i < n; i++) {
    if (w->mate && w->mate[i]) {
      if ((R->hit[i] || R->hit[i + 1]) != R->invert) {
        seq_out_print(t->out, 1, &w->b, i);
        seq_out_print(t->out, 2, &w->b, i + 1);
        t->printed += 2;
      }
      R->total_reads += 2;
      i++;
    } else {
      if ((R->hit[i] != 0) != R->invert) {
        seq_out_print(t->out, 0, &w->b, i);
        t->printed++;
      }
      R->total_reads++;
    }
  }
}

static void emit(reads_run *R, work *w)
{
  if (!w->b.nreads) { work_free(w); return; }
  if (!R->threaded) { R->process(R, w); work_free(w); return; }
  pthread_mutex_lock(&R->mu);
  while (R->slot) pthread_cond_wait(&R->cv, &R->mu);
  R->slot = w;
  pthread_cond_broadcast(&R->cv);
  pthread_mutex_unlock(&R->mu);
}

static void mate_alloc(work *w, size_t n)
{
  w->mate = calloc(n ? n : 1, 1);
  if (!w->mate) die("Out of memory");
}

static size_t read_len(const read_batch *b, size_t i) { return (size_t)(b->offsets[i + 1] - b->offsets[i]); }

static void keep_tail(read_batch *b, size_t from, bool want_quals)
{
  read_batch tmp;
  read_batch_init(&tmp, want_quals);
  read_batch_keep_names(&tmp);
  for (size_t i = from; i < b->nreads; i++) read_batch_append(&tmp, b, i);
  read_batch_free(b);
  *b = tmp;
}

/* the reads of one task, batch by batch, with the pairs marked (asyncio_run_pool's reader side) */
static void produce_task(reads_run *R, size_t ti)
{
  reads_task *t = &R->tasks[ti];
  if (t->kind == '1') {
    for (;;) {
      work *w = work_new(R, ti);
      seq_in_fill(t->f1, &w->b, READS_BATCH_BASES);
      if (!w->b.nreads) { work_free(w); break; }
      emit(R, w);
    }
    return;
  }
  read_batch b1, b2;
  read_batch_init(&b1, R->want_quals); read_batch_keep_names(&b1);
  read_batch_init(&b2, R->want_quals); read_batch_keep_names(&b2);
  if (t->kind == '2') { /* pair i = read i of each file */
    for (;;) {
      const size_t got1 = seq_in_fill(t->f1, &b1, READS_BATCH_BASES), got2 = seq_in_fill(t->f2, &b2, READS_BATCH_BASES);
      const size_t n = b1.nreads < b2.nreads ? b1.nreads : b2.nreads;
      if (!got1 && !got2 && n == 0) {
        if (b1.nreads != b2.nreads) warn("Different number of reads in pe files [%s; %s]", seq_in_path(t->f1), seq_in_path(t->f2));
        break;
      }
      work *w = work_new(R, ti);
      mate_alloc(w, 2 * n);
      for (size_t i = 0; i < n; i++) {
        read_batch_append(&w->b, &b1, i);
        if (read_len(&b2, i)) { /* (ctx_reads.c:225: a second read without sequence is no read) */
          w->mate[w->b.nreads - 1] = 1;
          read_batch_append(&w->b, &b2, i);
        }
      }
      keep_tail(&b1, n, R->want_quals);
      keep_tail(&b2, n, R->want_quals);
      emit(R, w);
    }
  } else { /* interleaved: two consecutive reads are a pair iff their names say so */
    for (;;) {
      const bool eof = seq_in_fill(t->f1, &b1, b1.nbases + READS_BATCH_BASES) == 0;
      if (!b1.nreads) break;
      work *w = work_new(R, ti);
      mate_alloc(w, b1.nreads);
      size_t i = 0;
      while (i < b1.nreads) {
        if (i + 1 == b1.nreads && !eof) break; /* its mate may be the next batch's first read */
        read_batch_append(&w->b, &b1, i);
        if (i + 1 < b1.nreads && seq_names_match(b1.names + b1.name_off[i], (size_t)(b1.name_off[i + 1] - b1.name_off[i]),
                                                 b1.names + b1.name_off[i + 1], (size_t)(b1.name_off[i + 2] - b1.name_off[i + 1]))) {
          if (read_len(&b1, i + 1)) {
            w->mate[w->b.nreads - 1] = 1;
            read_batch_append(&w->b, &b1, i + 1);
          }
          i += 2;
        } else {
          i++;
        }
      }
      keep_tail(&b1, i, R->want_quals);
      emit(R, w);
      if (eof && !b1.nreads) break;
    }
  }
  read_batch_free(&b1);
  read_batch_free(&b2);
}

static void *reader_main(void *arg)
{
  reads_run *R = arg;
  for (size_t i = 0; i < R->ntasks; i++) produce_task(R, i);
  pthread_mutex_lock(&R->mu);
  R->done = true;
  pthread_cond_broadcast(&R->cv);
  pthread_mutex_unlock(&R->mu);
  return NULL;
}

void reads_run_tasks(reads_run *R, unsigned nthreads)
{
  R->threaded = nthreads > 1;
  R->done = false;
  R->slot = NULL;
  if (R->threaded) { /* the reader fills batch n + 1 while the device works on batch n and its output is written */
    pthread_t th;
    pthread_mutex_init(&R->mu, NULL);
    pthread_cond_init(&R->cv, NULL);
    if (pthread_create(&th, NULL, reader_main, R) != 0) die("Cannot start the reader thread");
    for (;;) {
      pthread_mutex_lock(&R->mu);
      while (!R->slot && !R->done) pthread_cond_wait(&R->cv, &R->mu);
      work *w = R->slot;
      R->slot = NULL;
      pthread_cond_broadcast(&R->cv);
      pthread_mutex_unlock(&R->mu);
      if (!w) break;
      R->process(R, w);
      work_free(w);
    }
    pthread_join(th, NULL);
    pthread_mutex_destroy(&R->mu);
    pthread_cond_destroy(&R->cv);
  } else {
    for (size_t i = 0; i < R->ntasks; i++) produce_task(R, i);
  }
}

int ctx_reads(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, invert = false;
  unsigned nthreads = 0, device = 0;
  seq_fmt fmt = SEQ_FMT_FASTQ;
  reads_task *tasks = NULL;
  size_t ntasks = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "hfm:n:t:F:v1:2:i:", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(reads_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 't': cmd_threads_arg(&nthreads, reads_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, reads_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, reads_usage, optarg); break;
      case 'F': /* cmd_check(fmt == SEQ_FMT_FASTQ, cmd): only while the format is still the default */
        ONCE(fmt != SEQ_FMT_FASTQ);
        if (!strcasecmp(optarg, "fq") || !strcasecmp(optarg, "fastq")) fmt = SEQ_FMT_FASTQ;
        else if (!strcasecmp(optarg, "fa") || !strcasecmp(optarg, "fasta")) fmt = SEQ_FMT_FASTA;
        else if (!strcasecmp(optarg, "plain") || !strcasecmp(optarg, "txt")) fmt = SEQ_FMT_PLAIN;
        else print_usage(reads_usage, "Invalid %s {FASTA,FASTQ,PLAIN} option: %s", cmd, optarg);
        break;
      case 'v': ONCE(invert); invert = true; break;
      case '1': case '2': case 'i':
        tasks = realloc(tasks, (ntasks + 1) * sizeof(*tasks));
        if (!tasks) die("Out of memory");
        reads_task_parse(&tasks[ntasks++], c, optarg);
        break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(reads_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " reads -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (nthreads == 0) nthreads = 2;
  if (ntasks == 0) print_usage(reads_usage, "Please specify at least one sequence file (-1, -2 or -i)");
  if (optind >= argc) print_usage(reads_usage, "Please specify input graph file(s)");

  /* graph_files_open, then file_filter_flatten(.., 0): every colour of every file goes into colour 0 */
  graph_files in;
  graph_files_open(argv + optind, (size_t)(argc - optind), reads_usage, &in);
  graph_files_flatten(&in);
  const size_t kmer_size = in.files[0].kmer_size, W = in.files[0].num_words;

  /* inputs_attempt_open: every output before anything is loaded; on a failure nothing of this run stays behind */
  for (size_t i = 0; i < ntasks; i++) {
    tasks[i].out = seq_out_open(tasks[i].out_base, fmt, tasks[i].kind != '1', force);
    if (!tasks[i].out) {
      for (size_t j = 0; j < i; j++) seq_out_close(tasks[j].out, true);
      die("Error creating output files");
    }
  }

  const size_t bits_per_kmer = W * 64; /* sizeof(BinaryKmer) * 8 */
  /* a table that cannot be sized or a machine without a device: the outputs created above go away again */
  table_plan plan;
  mcx_graph *g = NULL;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (!err) {
    table_plan_status(&plan);
    err = graph_table_create(&g, &plan, kmer_size, 1, device);
  }
  if (err) {
    for (size_t j = 0; j < ntasks; j++) seq_out_close(tasks[j].out, true);
    die("%s", err);
  }
  for (size_t i = 0; i < in.n; i++) { ctx_load_graph_file(g, &in.files[i]); ctx_reader_close(&in.files[i]); }
  free(in.files);
  hasht_status(g);

  status("Printing reads that do %stouch the graph\n", invert ? "not " : "");

  reads_filter F;
  memset(&F, 0, sizeof(F));
  F.g = g; F.invert = invert;
  reads_run R;
  memset(&R, 0, sizeof(R));
  R.tasks = tasks; R.ntasks = ntasks;
  R.want_quals = fmt == SEQ_FMT_FASTQ;
  R.process = process; R.user = &F;
  reads_run_tasks(&R, nthreads);
  free(F.hit);

  size_t total_printed = 0;
  for (size_t i = 0; i < ntasks; i++) {
    total_printed += tasks[i].printed;
    seq_out_close(tasks[i].out, false);
    seq_in_close(tasks[i].f1);
    if (tasks[i].f2) seq_in_close(tasks[i].f2);
  }
  free(tasks);
  status("Total printed %zu / %zu (%.2f%%) reads\n", total_printed, F.total_reads,
         F.total_reads ? (100.0 * (double)total_printed) / (double)F.total_reads : 0.0);
  mcx_graph_destroy(g);
  return EXIT_SUCCESS;
}
