/* cmd_contigs.c -- `mccortex<K> contigs` (src/commands/ctx_contigs.c, src/tools/assemble_contigs.c): the graph file is
 * loaded as the other graph commands load it, the links of one .ctp go onto the handle piece by piece
 * (mcx_graph_links_load_text), the confidence table is computed on the host from the contig histogram of the .ctp header
 * (conf_table.c) and every seed is walked on the MI355X (mcx_graph_contigs).  The host writes the reference's FASTA
 * header from each record and the bases the device made behind it, then the summary from the stats.
 *
 * Where this differs from the reference (DESIGN.md lists it): the contigs come in key order, or in the order of the seed
 * reads, under the sequential seeding rule of include/mcx_gpu.h (the reference walks its hash table with racing
 * threads); -P, more than one -p, more than one graph file and a .ctp of several colours are refused; --device picks the
 * GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include "../../include/mcx_gpu.h"
#include "conf_table.h"

static const char contigs_usage[] =
"usage: " CMD_NAME " contigs [options] <in.ctx>\n"
"\n"
"  Assemble contigs from the graph of a sample with its links.\n"
"\n"
"  -h, --help            This help message\n"
"  -q, --quiet           Silence status output normally printed to STDERR\n"
"  -f, --force           Overwrite output files\n"
"  -o, --out <out.fa>    Print contigs in FASTA [default: no output, statistics only]\n"
"  -m, --memory <mem>    Memory to use (e.g. 1M, 20GB)\n"
"  -n, --nkmers <N>      Number of hash table entries (e.g. 1G ~ 1 billion)\n"
"  -t, --threads <T>     Accepted as the reference takes it; the walks run on the device\n"
"  -p, --paths <in.ctp>  Load the link file [required]\n"
"  -c, --colour <c>      Colour of the graph to assemble [default: 0]\n"
"  -N, --ncontigs <N>    Stop after N contigs [default: no limit]\n"
"  -s, --seed <in.fa>    Use the k-mers of this file as seeds (one k-mer per read)\n"
"  -r, --reseed          A k-mer of an earlier contig may seed a contig of its own\n"
"  -R, --no-reseed       It may not [default]\n"
"  -G, --genome <G>      Genome size in bases [default: the number of k-mers of the graph]\n"
"  -C, --confid-cumul <c> Stop when the cumulative confidence falls below c, 0 <= c <= 1\n"
"  -T, --confid-step <c> Stop at a step whose confidence is below c, 0 <= c <= 1\n"
"  -S, --confid-save <o.csv> Save the confidence table\n"
"  -M, --no-missing-check Do not use the missing-information check\n"
"  -P, --use-seed-paths  Seed with links that no contig used (not part of this build)\n"
"      --device <N>      GPU to run on [default: 0]\n"
"\n";

enum { OPT_DEVICE = 1000 };

static struct option longopts[] = {
  {"help", no_argument, NULL, 'h'},           {"out", required_argument, NULL, 'o'},          {"force", no_argument, NULL, 'f'},
  {"memory", required_argument, NULL, 'm'},   {"nkmers", required_argument, NULL, 'n'},       {"threads", required_argument, NULL, 't'},
  {"paths", required_argument, NULL, 'p'},    {"colour", required_argument, NULL, 'c'},       {"color", required_argument, NULL, 'c'},
  {"ncontigs", required_argument, NULL, 'N'}, {"seed", required_argument, NULL, 's'},         {"reseed", no_argument, NULL, 'r'},
  {"no-reseed", no_argument, NULL, 'R'},      {"genome", required_argument, NULL, 'G'},       {"confid-cumul", required_argument, NULL, 'C'},
  {"confid-step", required_argument, NULL, 'T'}, {"confid-save", required_argument, NULL, 'S'}, {"no-missing-check", no_argument, NULL, 'M'},
  {"use-seed-paths", no_argument, NULL, 'P'}, {"device", required_argument, NULL, OPT_DEVICE}, {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(contigs_usage, "%s given twice", cmd); } while (0)

static const char *const stop_names[9] = {"StopUnknown", "StopNoCovg", "StopPopForkNoColCovg", "StopForkNoPaths", "StopForkInPaths", "StopMissingPaths",
                                          "StopHitLoop", "StopLowStepConfidence", "StopLowCumulativeConfidence"};
static const char *const step_names[9] = {"GoPopForward", "GoColForward", "GoPopForkColForward", "FailNoCovg", "FailNoColCovg", "FailNoLinks",
                                          "FailSplitLinks", "FailMissingLinks", "GoUseLinks"};

static int gz_read(void *ctx, void *dst, unsigned n) { return gzread((gzFile)ctx, dst, n); }
static char *grow_heap(void *ctx, size_t bytes)
{
  char **held = ctx;
  free(*held);
  if (!(*held = malloc(bytes))) die("Out of memory");
  return *held;
}

/* what the two sinks share: the records of the batch wait until their bases come */
typedef struct {
  FILE *fh;
  unsigned kmer_size;
  mcx_contig_rec *recs;
  size_t nrecs, next, cap;
  bool in_line;
  uint64_t contig_id;
  size_t *lens, nlens, cap_lens;
} fasta_out;

static int rec_sink(void *ctx, const void *data, size_t nbytes)
{
  fasta_out *o = ctx;
  const size_t n = nbytes / sizeof(mcx_contig_rec);
  if (o->next == o->nrecs || !o->fh) o->next = o->nrecs = 0; /* (without an output file only the lengths are kept) */
  if (o->nrecs + n > o->cap) {
    o->cap = 2 * (o->nrecs + n);
    if (!(o->recs = realloc(o->recs, o->cap * sizeof(*o->recs)))) return 1;
  }
  memcpy(o->recs + o->nrecs, data, n * sizeof(mcx_contig_rec));
  o->nrecs += n;
  if (o->nlens + n > o->cap_lens) {
    o->cap_lens = 2 * (o->nlens + n);
    if (!(o->lens = realloc(o->lens, o->cap_lens * sizeof(*o->lens)))) return 1;
  }
  for (size_t i = 0; i < n; i++) o->lens[o->nlens++] = (size_t)((const mcx_contig_rec *)data)[i].len_nodes;
  return 0;
}

/* _dump_contig:184-191 */
static void put_header(fasta_out *o, const mcx_contig_rec *r)
{
  unsigned char key[32];
  char kmer[MAX_KMER_SIZE + 1], rc[MAX_KMER_SIZE + 1];
  memcpy(key, r->seed_key, sizeof(key));
  kmer_words_to_str(key, o->kmer_size, kmer);
  for (unsigned i = 0; i < o->kmer_size; i++) {
    const char c = kmer[o->kmer_size - 1 - i];
    rc[i] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
  }
  rc[o->kmer_size] = 0;
  fprintf(o->fh, ">contig%llu len=%llu seed=%s seedkmers=1 lf.status=%s lf.paths.held=%u lf.paths.cntr=%u lf.max_gap=%llu lf.conf=%f "
          "rt.status=%s rt.paths.held=%u rt.paths.cntr=%u rf.max_gap=%llu rf.conf=%f\n",
          (unsigned long long)o->contig_id++, (unsigned long long)r->len_nodes, rc, stop_names[r->stop_causes[0] % 9], r->paths_held[0], r->paths_cntr[0],
          (unsigned long long)r->max_step_gap[0], r->gap_conf[0], stop_names[r->stop_causes[1] % 9], r->paths_held[1], r->paths_cntr[1],
          (unsigned long long)r->max_step_gap[1], r->gap_conf[1]);
}

static int seq_sink(void *ctx, const void *data, size_t nbytes)
{
  fasta_out *o = ctx;
  const char *p = data, *end = p + nbytes;
  while (p < end) {
    if (!o->in_line) {
      if (o->next >= o->nrecs) return 1;
      put_header(o, &o->recs[o->next++]);
      o->in_line = true;
    }
    const char *nl = memchr(p, '\n', (size_t)(end - p));
    const size_t n = (size_t)((nl ? nl + 1 : end) - p);
    if (fwrite(p, 1, n, o->fh) != n) return 1;
    if (nl) o->in_line = false;
    p += n;
  }
  return 0;
}

static int size_cmp(const void *a, const void *b)
{
  const size_t x = *(const size_t *)a, y = *(const size_t *)b;
  return x < y ? -1 : x > y;
}

/* the numbers of a JSON array [a, b, ..] between vb and ve */
static size_t json_numbers(const char *vb, const char *ve, uint64_t **out)
{
  size_t n = 0, cap = 16;
  uint64_t *v = malloc(cap * sizeof(*v));
  if (!v) die("Out of memory");
  for (const char *p = vb; p < ve;) {
    if (*p < '0' || *p > '9') { p++; continue; }
    char *e;
    const uint64_t x = strtoull(p, &e, 10);
    if (n == cap && !(v = realloc(v, (cap *= 2) * sizeof(*v)))) die("Out of memory");
    v[n++] = x;
    p = e;
  }
  *out = v;
  return n;
}

static double confid_arg(const char *cmd, const char *arg)
{
  char *end;
  const double v = strtod(arg, &end);
  if (end == arg || *end) print_usage(contigs_usage, "%s requires a double: %s", cmd, arg);
  if (v < 0 || v > 1) die("%s must be 0 <= x <= 1", cmd);
  return v;
}

int ctx_contigs(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, reseed = false, no_reseed = false, missing_check = true;
  unsigned nthreads = 0, device = 0, colour = 0;
  bool colour_set = false;
  size_t contig_limit = 0, genome_size = 0, nseed_files = 0;
  double min_cumul = -1.0, min_step = -1.0;
  const char *out_path = NULL, *ctp_path = NULL, *conf_path = NULL;
  char **seed_paths = NULL;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:t:p:c:N:s:rRG:C:T:S:MP", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(contigs_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 't': cmd_threads_arg(&nthreads, contigs_usage, cmd, optarg); break;
      case 'm': cmd_mem_set_memory(&mem, contigs_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, contigs_usage, optarg); break;
      case 'p':
        if (ctp_path) die("-p, --paths <in.ctp> given twice: this build's `contigs` takes the links of one file");
        ctp_path = optarg; break;
      case 's':
        if (!(seed_paths = realloc(seed_paths, (nseed_files + 1) * sizeof(*seed_paths)))) die("Out of memory");
        seed_paths[nseed_files++] = optarg; break;
      case 'r': ONCE(reseed); reseed = true; break;
      case 'R': ONCE(no_reseed); no_reseed = true; break;
      case 'N': ONCE(contig_limit); if (!parse_entire_size(optarg, &contig_limit) || !contig_limit) print_usage(contigs_usage, "%s requires an int x > 0: %s", cmd, optarg); break;
      case 'c': ONCE(colour_set); colour_set = true; if (!parse_entire_uint(optarg, &colour)) print_usage(contigs_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case 'G': ONCE(genome_size); if (!mem_to_integer(optarg, &genome_size) || !genome_size) print_usage(contigs_usage, "%s requires a number of bases: %s", cmd, optarg); break;
      case 'S': ONCE(conf_path); conf_path = optarg; break;
      case 'M': ONCE(!missing_check); missing_check = false; break;
      case 'P': die("-P, --use-seed-paths: seeding with the links that no contig used is not part of this build's `contigs`");
      case 'C': ONCE(min_cumul >= 0); min_cumul = confid_arg(cmd, optarg); break;
      case 'T': ONCE(min_step >= 0); min_step = confid_arg(cmd, optarg); break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(contigs_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " contigs -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (no_reseed && reseed) print_usage(contigs_usage, "Cannot specify both -r and -R");
  if (!nseed_files && !contig_limit && reseed) print_usage(contigs_usage, "Please specify one or more of: --no-reseed | --ncontigs | --seed <in.fa>");
  if (optind >= argc) print_usage(contigs_usage, "Require input graph files (.ctx)");
  if (optind + 1 < argc) die("This build's `contigs` takes one graph file. What is this: '%s'", argv[optind + 1]);
  if (!ctp_path) print_usage(contigs_usage, "-p, --paths <in.ctp> is required");
  if (out_path && strcmp(out_path, "-") && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);
  if (conf_path && !force && access(conf_path, F_OK) == 0) die("File already exists: %s", conf_path);

  graph_files in;
  graph_files_open(argv + optind, 1, contigs_usage, &in);
  const size_t kmer_size = in.files[0].kmer_size, W = in.files[0].num_words, ncols = in.ncols;
  if (colour >= ncols) die("-c, --colour %u: the graph file loads into %zu colour%s", colour, ncols, plural(ncols));

  /* gpath_reader_open: the header of the .ctp */
  gzFile gz = strcmp(ctp_path, "-") == 0 ? gzdopen(dup(STDIN_FILENO), "r") : gzopen(ctp_path, "r");
  if (!gz) die("Cannot open file: %s", ctp_path);
  gzbuffer(gz, 1u << 20);
  ctp_str raw = {NULL, 0, 0};
  size_t hdr_len = 0;
  while (true) {
    char tmp[4096];
    const int got = gzread(gz, tmp, sizeof(tmp));
    if (got < 0) die("Cannot read file: %s", ctp_path);
    if (got > 0) ctp_str_add(&raw, tmp, (size_t)got);
    hdr_len = raw.len ? ctp_hdr_span(raw.b, raw.len) : 0;
    if (hdr_len == (size_t)-1) die("Expected JSON header: %s", ctp_path);
    if (hdr_len) break;
    if (got == 0) die("Cannot find end of JSON header: %s", ctp_path);
  }
  uint64_t version = 0, pcols = 0, pk = 0;
  if (!ctp_hdr_number(raw.b, hdr_len, "format_version", NULL, &version) || version != 4) die("Only link files of format version 4 are read: %s", ctp_path);
  if (!ctp_hdr_number(raw.b, hdr_len, "graph", "num_colours", &pcols) || !ctp_hdr_number(raw.b, hdr_len, "graph", "kmer_size", &pk))
    die("Cannot find graph.num_colours and graph.kmer_size in header: %s", ctp_path);
  if (pcols != 1) die("This build's `contigs` takes a link file of one colour, this one has %llu: %s", (unsigned long long)pcols, ctp_path);
  if (pk != kmer_size) die("Kmer sizes don't match: the graph has %zu, the link file %llu [%s]", kmer_size, (unsigned long long)pk, ctp_path);
  /* paths.contig_hists[0]: lengths and counts */
  uint64_t *hl = NULL, *hc = NULL;
  size_t nh = 0;
  const char *pb, *pe, *cb, *ce, *vb, *ve;
  if (ctp_json_member(raw.b, raw.b + hdr_len, "paths", &pb, &pe) && ctp_json_member(pb, pe, "contig_hists", &cb, &ce)) {
    const char *ob = memchr(cb, '{', (size_t)(ce - cb));
    if (ob) {
      const size_t span = ctp_hdr_span(ob, (size_t)(ce - ob));
      if (span && span != (size_t)-1 && ctp_json_member(ob, ob + span, "lengths", &vb, &ve)) {
        nh = json_numbers(vb, ve, &hl);
        if (!ctp_json_member(ob, ob + span, "counts", &vb, &ve) || json_numbers(vb, ve, &hc) != nh) die("Bad contig histogram in header: %s", ctp_path);
      }
    }
  }

  const size_t bits_per_kmer = 64 * W + 40 * ncols;
  table_plan plan;
  const char *err = table_plan_for_args(&mem, bits_per_kmer, (int64_t)in.sum_kmers, &plan);
  if (err) die("%s", err);
  table_plan_status(&plan);
  mcx_graph *g = NULL;
  if ((err = graph_table_create(&g, &plan, kmer_size, ncols, device))) die("%s", err);
  ctx_load_graph_file(g, &in.files[0]);
  ctx_reader_close(&in.files[0]);
  free(in.files);
  hasht_status(g);
  uint64_t nkmers = 0;
  mcx_check(mcx_graph_nkmers(g, &nkmers), "contigs");
  if (!genome_size) {
    char nk[50];
    genome_size = (size_t)nkmers;
    status("Taking number of kmers as genome size: %s", ulong_to_str(genome_size, nk));
  }

  /* the links, in pieces of whole k-mer blocks */
  size_t cap = 64u << 20;
  if (getenv("MCX_LINKS_PIECE")) cap = strtoul(getenv("MCX_LINKS_PIECE"), NULL, 10); /* (tests: pieces of a few hundred bytes) */
  if (cap < 64) cap = 64;
  char *piece = NULL;
  ctp_pieces P;
  ctp_pieces_init(&P, grow_heap(&piece, cap), cap, gz_read, gz, grow_heap, &piece);
  ctp_pieces_preload(&P, raw.b + hdr_len, raw.len - hdr_len);
  uint64_t nlinks = 0;
  long long n;
  while ((n = ctp_pieces_next(&P)) != 0) {
    if (n < 0) die("Cannot read file: %s", ctp_path);
    uint64_t nl = 0, nmiss = 0;
    const int rc = mcx_graph_links_load_text(g, P.buf, (uint64_t)n, &nl, &nmiss);
    if (rc == MCX_ERR_INVAL && nmiss) die("%llu k-mers of the link file are not in the graph [%s]: was it made from this graph?", (unsigned long long)nmiss, ctp_path);
    mcx_check(rc, "contigs");
    nlinks += nl;
  }
  gzclose(gz);
  free(piece);
  mcx_links_info info;
  mcx_check(mcx_graph_links_info(g, &info), "contigs");
  char s0[50], s1[50];
  status("Loaded %s links on %s k-mers from %s", ulong_to_str(info.num_paths, s0), ulong_to_str(info.num_kmers_with_paths, s1), ctp_path);

  /* the confidence table (ctx_contigs.c: conf_table_update_hist over the histogram of the link file) */
  conf_table conf;
  conf_table_init(&conf);
  size_t hist_len = 1;
  for (size_t i = 0; i < nh; i++)
    if (hl[i] + 1 > hist_len) hist_len = (size_t)hl[i] + 1;
  size_t *hist = calloc(hist_len, sizeof(*hist));
  if (!hist) die("Out of memory");
  for (size_t i = 0; i < nh; i++) hist[hl[i]] += (size_t)hc[i];
  if (!conf_table_update_hist(&conf, genome_size, hist, hist_len)) die("Out of memory");
  free(hist); free(hl); free(hc);
  if (conf_path) {
    FILE *fh = fopen(conf_path, "w");
    if (!fh) die("Cannot open file: %s [%s]", conf_path, strerror(errno));
    conf_table_print(&conf, fh);
    fclose(fh);
    status("Saved the confidence table to %s", conf_path);
  }

  /* the seed reads */
  read_batch seeds;
  read_batch_init(&seeds, false);
  for (size_t i = 0; i < nseed_files; i++) {
    seq_in *f = seq_in_open(seed_paths[i]);
    if (!f) die("Cannot read --seed file: %s", seed_paths[i]);
    while (seq_in_fill(f, &seeds, (size_t)-1) > 0) {}
    seq_in_close(f);
  }

  fasta_out out;
  memset(&out, 0, sizeof(out));
  out.kmer_size = (unsigned)kmer_size;
  if (out_path) {
    out.fh = strcmp(out_path, "-") == 0 ? stdout : fopen(out_path, "w");
    if (!out.fh) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
    status("Writing contigs to %s", outpath(out_path));
  }
  mcx_contigs_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.colour = colour;
  prm.flags = (reseed ? MCX_CONTIGS_RESEED : 0u) | (missing_check ? 0u : MCX_CONTIGS_NO_MISSING_CHECK);
  prm.ncontigs = contig_limit;
  prm.min_step_confid = min_step; prm.min_cumul_confid = min_cumul;
  prm.conf = conf.b; prm.nconf = conf.len;
  mcx_contigs_stats st;
  memset(&st, 0, sizeof(st));
  static const uint64_t no_offsets[1] = {0};
  const int rc = mcx_graph_contigs(g, seeds.bases, nseed_files ? (seeds.nreads ? seeds.offsets : no_offsets) : NULL, nseed_files ? seeds.nreads : 0, &prm, rec_sink,
                                   &out, out.fh ? seq_sink : NULL, &out, &st);
  if (rc == MCX_ERR_INVAL) die("A seed is not %zu bases of ACGT: %s", kmer_size, mcx_last_error());
  mcx_check(rc, "contigs");
  if (out.fh && out.fh != stdout && fclose(out.fh) != 0) die("Cannot write to file: %s", out_path);

  /* the summary (assemble_contigs_stats_print) */
  char t[4][50];
  status("[Assemble] pulled out %s contigs, %s from seed kmers", ulong_to_str(st.contigs, t[0]), ulong_to_str(st.contigs, t[1]));
  status("[Assemble] no-reseed aborted %s times; seeds not found: %s", ulong_to_str(st.num_reseed_abort, t[0]), ulong_to_str(st.seeds_not_found, t[1]));
  if (out.nlens) {
    qsort(out.lens, out.nlens, sizeof(size_t), size_cmp);
    size_t sum = 0, acc = 0, n50 = 0;
    for (size_t i = 0; i < out.nlens; i++) sum += out.lens[i];
    for (size_t i = out.nlens; i-- > 0;) { acc += out.lens[i]; if (2 * acc >= sum) { n50 = out.lens[i]; break; } }
    const size_t med = out.nlens & 1 ? out.lens[out.nlens / 2] : (out.lens[out.nlens / 2 - 1] + out.lens[out.nlens / 2]) / 2;
    status("[Assemble] Lengths: mean: %.2f  median: %zu  N50: %zu  min: %zu  max: %zu  total: %zu  [kmers]", (double)sum / out.nlens, med, n50, out.lens[0],
           out.lens[out.nlens - 1], sum);
    status("[Assemble] Junctions: %s in total, %.4f per contig", ulong_to_str(st.total_junc, t[0]), (double)st.total_junc / out.nlens);
  }
  for (int i = 0; i < 9; i++)
    if (st.stop_causes[i]) status("[Assemble]   %s: %s", stop_names[i], ulong_to_str(st.stop_causes[i], t[0]));
  for (int i = 0; i < 9; i++)
    if (st.wlk_steps[i]) status("[Assemble]   %s: %s", step_names[i], ulong_to_str(st.wlk_steps[i], t[0]));
  if (st.corrupt_links) warn("%s walks stopped at a link that names a base its fork has not: was the link file made from this graph?", ulong_to_str(st.corrupt_links, t[0]));
  status("[Assemble] walks run again with larger ranges: %s", ulong_to_str(st.reruns, t[0]));

  free(out.recs); free(out.lens); free(raw.b); free(seed_paths);
  read_batch_free(&seeds);
  conf_table_free(&conf);
  mcx_graph_destroy(g);
  (void)nlinks;
  return EXIT_SUCCESS;
}
