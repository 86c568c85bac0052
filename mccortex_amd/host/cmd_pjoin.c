/* cmd_pjoin.c -- `mccortex<K> pjoin` (src/commands/ctx_pjoin.c): merge link files, a colour per file or several files
 * into one colour.  The reference's usage text, option table, argument checks and closing lines; its hash table of
 * k-mers with lists of links is a sort and a segmented reduce on the MI355X (mcx_pjoin_add_text, mcx_pjoin_finish), the
 * body of every input streaming through it in pieces of whole k-mer blocks (ctp_hdr.c).  The header is merged from the
 * inputs' headers as text (ctp_merge.c).
 *
 * Where this differs from the reference (DESIGN.md lists it): format version 4 only; the k-mers of the output come in
 * ascending order of their text, not in hash-table order; -n is checked, reported and otherwise unused (there is no
 * table); -m is the ceiling of the link store in HBM; -r is accepted and changes nothing, as in the reference, and says
 * so; the "mccortex" field of the command names this build and there is no "htslib" field; --device picks the GPU. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include "../../include/mcx_gpu.h"

static const char pjoin_usage[] =
"usage: " CMD_NAME " pjoin [options] <in1.ctp.gz> [[offset:]in2.ctp[:0,2-4] ...]\n"
"\n"
"  Merge cortex link files.\n"
"\n"
"  -h, --help             This help message\n"
"  -q, --quiet            Silence status output normally printed to STDERR\n"
"  -f, --force            Overwrite output files\n"
"  -o, --out <out.ctp.gz> Output file [required]\n"
"  -m, --memory <mem>     Memory the link store may take on the GPU [default: what is free]\n"
"  -n, --nkmers <nkmers>  Checked and reported; there is no hash table to size\n"
"  -t, --threads <T>      Number of threads to use [default: 2]\n"
"  -g, --graph <in.ctx>   Check the link files against a graph file\n"
"  -c, --outcols <C>      How many 'colours' should the output file have\n"
"  -r, --noredundant      Accepted; changes nothing (nor does it in the reference)\n"
"      --device <N>       GPU to run on [default: 0]\n"
"\n"
"  Files can be specified with specific colours: samples.ctp:2,3\n"
"  Offset specifies where to load the first colour: 3:samples.ctp\n"
"\n";

static const char ctp_comment[] = /* ctp_explanation_comment, as `thread` writes it */
"# Links merged by " CMD_NAME " pjoin\n"
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
  {"help", no_argument, NULL, 'h'},          {"out", required_argument, NULL, 'o'},     {"force", no_argument, NULL, 'f'},
  {"memory", required_argument, NULL, 'm'},  {"nkmers", required_argument, NULL, 'n'},  {"threads", required_argument, NULL, 't'},
  {"graph", required_argument, NULL, 'g'},   {"outcols", required_argument, NULL, 'c'}, {"noredundant", no_argument, NULL, 'r'},
  {"device", required_argument, NULL, OPT_DEVICE}, {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(pjoin_usage, "%s given twice", cmd); } while (0)

typedef struct {
  const char *input;
  char *path;
  gzFile gz;
  ctp_str raw; /* the header and what was read behind it */
  size_t hdr_len;
  uint64_t ncols, kmer_size, nkmers, nlinks;
  col_filter *filter;
  size_t nfilter, into_ncols;
} pjoin_file;

static int gz_read(void *ctx, void *dst, unsigned n) { return gzread((gzFile)ctx, dst, n); }
static char *grow_pinned(void *ctx, size_t bytes)
{
  void *p = NULL;
  mcx_check(mcx_pjoin_buffer((mcx_pjoin *)ctx, bytes, &p), "pjoin");
  return p;
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

/* gpath_reader_open2: the header object of a version-4 file; the body stays in the stream */
static void pjoin_open(pjoin_file *f, const char *input, size_t into_offset)
{
  memset(f, 0, sizeof(*f));
  f->input = input;
  f->path = ctx_arg_path(input);
  f->gz = strcmp(f->path, "-") == 0 ? gzdopen(dup(STDIN_FILENO), "r") : gzopen(f->path, "r");
  if (!f->gz) die("Cannot open file: %s", f->path);
  gzbuffer(f->gz, 1u << 20);
  while (true) {
    char tmp[4096];
    const int got = gzread(f->gz, tmp, sizeof(tmp));
    if (got < 0) die("Cannot read file: %s", f->path);
    if (got > 0) ctp_str_add(&f->raw, tmp, (size_t)got);
    f->hdr_len = f->raw.len ? ctp_hdr_span(f->raw.b, f->raw.len) : 0;
    if (f->hdr_len == (size_t)-1) die("Expected JSON header: %s", f->path);
    if (f->hdr_len) break;
    if (got == 0) die("Cannot find end of JSON header: %s", f->path);
  }
  uint64_t version = 0, nbytes = 0;
  const char *fb, *fe;
  if (!ctp_json_member(f->raw.b, f->raw.b + f->hdr_len, "file_format", &fb, &fe) || fe - fb != 5 || memcmp(fb, "\"ctp\"", 5))
    die("File is not a link file (file_format is not \"ctp\"): %s", f->path);
  if (!ctp_hdr_number(f->raw.b, f->hdr_len, "format_version", NULL, &version)) die("Cannot find format_version in header: %s", f->path);
  if (version != 4) die("Only link files of format version 4 are read, this one has version %llu: %s", (unsigned long long)version, f->path);
  if (!ctp_hdr_number(f->raw.b, f->hdr_len, "graph", "num_colours", &f->ncols) || !ctp_hdr_number(f->raw.b, f->hdr_len, "graph", "kmer_size", &f->kmer_size))
    die("Cannot find graph.num_colours and graph.kmer_size in header: %s", f->path);
  if (!f->ncols || f->ncols > (1u << 20)) die("Bad number of colours %llu: %s", (unsigned long long)f->ncols, f->path);
  if (!ctp_hdr_number(f->raw.b, f->hdr_len, "paths", "num_kmers_with_paths", &f->nkmers) || !ctp_hdr_number(f->raw.b, f->hdr_len, "paths", "num_paths", &f->nlinks) ||
      !ctp_hdr_number(f->raw.b, f->hdr_len, "paths", "path_bytes", &nbytes))
    die("Cannot find required header entries: %s", f->path);
  ctx_arg_filter(input, (uint32_t)f->ncols, into_offset, &f->filter, &f->nfilter, &f->into_ncols);
}

/* a name as ctp_hdr.c writes a JSON string, to be held against a sample name as it stands in a header */
static void json_name(ctp_str *s, const char *p)
{
  char tmp[8];
  ctp_str_add(s, "\"", 1);
  for (; *p; p++) {
    const unsigned char ch = (unsigned char)*p;
    if (ch == '"' || ch == '\\') { tmp[0] = '\\'; tmp[1] = (char)ch; ctp_str_add(s, tmp, 2); }
    else if (ch == '\n') ctp_str_add(s, "\\n", 2);
    else if (ch == '\t') ctp_str_add(s, "\\t", 2);
    else if (ch < 0x20) { snprintf(tmp, sizeof(tmp), "\\u%04x", ch); ctp_str_add(s, tmp, 6); }
    else ctp_str_add(s, p, 1);
  }
  ctp_str_add(s, "\"", 1);
}

/* graphs_gpaths_compatible with one graph file: k, k-mers, colours, sample names */
static void check_graph(const char *graph_path, const pjoin_file *files, size_t nfiles, size_t ctp_max_cols, uint64_t ctp_max_kmers)
{
  ctx_reader g;
  ctx_reader_open(&g, graph_path, 0, MIN_KMER_SIZE, MAX_KMER_SIZE);
  for (size_t i = 0; i < nfiles; i++)
    if (files[i].kmer_size != g.kmer_size) die("Kmer-size doesn't match between files [%zu vs %zu]: %s", (size_t)g.kmer_size, (size_t)files[i].kmer_size, files[i].input);
  if (g.num_kmers > 0 && ctp_max_kmers > (uint64_t)g.num_kmers) die("More kmers in link files than in graph files! (%zu > %zu)", (size_t)ctp_max_kmers, (size_t)g.num_kmers);
  if (ctp_max_cols > g.into_ncols) die("More colours in link files than in graph files! (%zu > %zu)", ctp_max_cols, g.into_ncols);
  for (size_t i = 0; i < nfiles; i++)
    for (size_t j = 0; j < files[i].nfilter; j++)
      for (size_t m = 0; m < g.nfilter; m++) {
        if (g.filter[m].into != files[i].filter[j].into) continue;
        const char *b, *e;
        ctp_str name = {NULL, 0, 0};
        json_name(&name, g.ginfo[g.filter[m].from].name);
        if (ctp_hdr_sample(files[i].raw.b, files[i].hdr_len, files[i].filter[j].from, &b, &e) && ((size_t)(e - b) != name.len || memcmp(b, name.b, name.len)))
          die("Sample names don't match\n%s:%u%s\n%s:%u%.*s\n", graph_path, g.filter[m].from, name.b, files[i].input, files[i].filter[j].from, (int)(e - b), b);
        free(name.b);
      }
  ctx_reader_close(&g);
}

int ctx_pjoin(int argc, char **argv)
{
  cmd_mem_args mem = CMD_MEM_ARGS_INIT;
  bool force = false, noredundant = false;
  unsigned nthreads = 0, device = 0, output_ncols = 0;
  const char *out_path = NULL, *graph_path = NULL;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fm:n:t:g:c:r", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(pjoin_usage, NULL);
      case 'f': ONCE(force); force = true; break;
      case 'o': ONCE(out_path); out_path = optarg; break;
      case 'm': cmd_mem_set_memory(&mem, pjoin_usage, optarg); break;
      case 'n': cmd_mem_set_nkmers(&mem, pjoin_usage, optarg); break;
      case 't': cmd_threads_arg(&nthreads, pjoin_usage, cmd, optarg); break;
      case 'g': ONCE(graph_path); graph_path = optarg; break;
      case 'c':
        ONCE(output_ncols);
        if (!parse_entire_uint(optarg, &output_ncols) || !output_ncols) print_usage(pjoin_usage, "%s requires an int x > 0", cmd);
        break;
      case 'r': ONCE(noredundant); noredundant = true; break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(pjoin_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " pjoin -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (!out_path) print_usage(pjoin_usage, "--out <out.ctp.gz> required");
  if (optind >= argc) print_usage(pjoin_usage, "Please specify at least one input file");

  /* ---- open all link files: each loads into the colours from the running maximum on unless it names an offset ---- */
  const size_t nfiles = (size_t)(argc - optind);
  pjoin_file *files = calloc(nfiles, sizeof(pjoin_file));
  if (!files) die("Out of memory");
  size_t ctp_max_cols = 0;
  uint64_t ctp_max_kmers = 0, ctp_sum_kmers = 0;
  for (size_t i = 0; i < nfiles; i++) {
    pjoin_open(&files[i], argv[optind + i], ctp_max_cols);
    if (files[i].into_ncols > ctp_max_cols) ctp_max_cols = files[i].into_ncols;
    if (files[i].nkmers > ctp_max_kmers) ctp_max_kmers = files[i].nkmers;
    ctp_sum_kmers += files[i].nkmers;
    status("[FileFilter] Loading file %s [%llu colour%s] into colour%s %u..", files[i].path, (unsigned long long)files[i].ncols, plural(files[i].ncols),
           plural(files[i].nfilter), files[i].nfilter ? files[i].filter[0].into : 0);
  }
  if (!output_ncols) output_ncols = (unsigned)ctp_max_cols;
  else if (ctp_max_cols > output_ncols) print_usage(pjoin_usage, "You specified --outcols %u but inputs need at %zu colours", output_ncols, ctp_max_cols);
  const size_t kmer_size = (size_t)files[0].kmer_size;
  for (size_t i = 0; i < nfiles; i++) /* graphs_gpaths_compatible */
    if (files[i].kmer_size != kmer_size) die("Kmer-size doesn't match between files [%zu vs %zu]: %s", kmer_size, (size_t)files[i].kmer_size, files[i].input);
  if (kmer_size < MIN_KMER_SIZE || kmer_size > MAX_KMER_SIZE || !(kmer_size & 1))
    die("kmer size %zu is not an odd number within %d..%d: %s", kmer_size, MIN_KMER_SIZE, MAX_KMER_SIZE, files[0].path);
  if (graph_path) check_graph(graph_path, files, nfiles, ctp_max_cols, ctp_max_kmers);
  if (mem.nkmers_set) {
    char a[64], b[64];
    if (mem.num_kmers > ctp_sum_kmers) warn("Using %s kmers instead of (-n) %s", ulong_to_str(ctp_sum_kmers, a), ulong_to_str(mem.num_kmers, b));
    status("-n, --nkmers is not used: the links are merged by a sort, not in a hash table");
  }
  if (noredundant) status("-r, --noredundant changes nothing: the reference parses it and never uses it, and so does this build");

  /* the header is put together once before anything is loaded: a clash of sample names ends the command here */
  char file_key[17], cmd_key[9], errbuf[1024];
  ctp_str command = {NULL, 0, 0}, hdr = {NULL, 0, 0};
  ctp_merge_input *min = calloc(nfiles, sizeof(ctp_merge_input));
  if (!min) die("Out of memory");
  for (size_t i = 0; i < nfiles; i++) min[i] = (ctp_merge_input){files[i].raw.b, files[i].hdr_len, files[i].filter, files[i].nfilter, files[i].path};
  ctp_hex_key(file_key, 16);
  ctp_hex_key(cmd_key, 8);
  ctp_hdr_command(&command, cmd_key, argc, argv, out_path, file_key, NULL);
  const char *why = ctp_merge_header(&hdr, min, nfiles, kmer_size, output_ncols, file_key, command.b, 0, 0, 0, errbuf, sizeof(errbuf));
  if (why) die("%s", why);

  const bool to_stdout = !strcmp(out_path, "-");
  if (!to_stdout && !force && access(out_path, F_OK) == 0) die("File already exists: %s", out_path);

  /* ---- the device ---- */
  if (mcx_device_count() < 1) die("No MI355X / HIP device found: %s has no CPU build path", CMD_NAME);
  mcx_pjoin *P = NULL;
  mcx_check(mcx_pjoin_create(&P, (int)kmer_size, (int)output_ncols, (int)device), "Cannot set up the merge");
  if (mem.mem_set) {
    char a[64];
    mcx_check(mcx_pjoin_configure(P, "max_bytes", mem.mem_to_use), "pjoin");
    status("[memory] paths: at most %s of HBM for the link store", bytes_to_str(mem.mem_to_use, 1, a));
  }
  size_t cap = 64u << 20;
  if (getenv("MCX_LINKS_PIECE")) cap = strtoul(getenv("MCX_LINKS_PIECE"), NULL, 10); /* (tests: pieces of a few hundred bytes) */
  if (cap < 64) cap = 64;
  for (size_t i = 0; i < nfiles; i++) {
    pjoin_file *f = &files[i];
    int32_t *flt = malloc((f->nfilter ? f->nfilter : 1) * 2 * sizeof(int32_t));
    if (!flt) die("Out of memory");
    for (size_t j = 0; j < f->nfilter; j++) { flt[2 * j] = (int32_t)f->filter[j].from; flt[2 * j + 1] = (int32_t)f->filter[j].into; }
    ctp_pieces pc;
    ctp_pieces_init(&pc, grow_pinned(P, cap), cap, gz_read, f->gz, grow_pinned, P);
    ctp_pieces_preload(&pc, f->raw.b + f->hdr_len, f->raw.len - f->hdr_len);
    uint64_t base = 0, seen_kmers = 0, seen_links = 0, kept = 0, bad_n = 0;
    long long n;
    while ((n = ctp_pieces_next(&pc)) != 0) {
      if (n < 0) die("Cannot read file: %s", f->path);
      mcx_pjoin_piece_stats ps;
      const int rc = mcx_pjoin_add_text(P, pc.buf, (uint64_t)n, (int)f->ncols, flt, (int)f->nfilter, &ps);
      if (rc == MCX_ERR_INVAL) {
        int code = 0;
        uint64_t off = 0;
        mcx_pjoin_error(P, &code, &off);
        const char *line = pc.buf + off, *nl = memchr(line, '\n', (size_t)n - off);
        const long len = (nl ? nl : pc.buf + n) - line;
        die("[LoadPathError] Bad line (refusal %d) [%s, byte %llu behind the header]: %.*s", code, f->path, (unsigned long long)(base + off), (int)(len > 200 ? 200 : len), line);
      }
      if (rc == MCX_ERR_NOMEM) die("Not enough memory for the links (-m, --memory <mem>): %s", mcx_last_error());
      mcx_check(rc, "pjoin");
      seen_kmers += ps.kmer_lines; seen_links += ps.link_lines; kept += ps.links_kept; bad_n += ps.kmers_n_mismatch;
      base += (uint64_t)n;
    }
    gzclose(f->gz);
    f->gz = NULL;
    free(flt);
    if (bad_n) warn("Number of links mismatches: %llu k-mer line%s with a number other than the link lines that follow [%s]", (unsigned long long)bad_n, plural(bad_n), f->path);
    if (f->nkmers != seen_kmers) die("[LoadPathError] header number of kmers don't match seen (exp %zu vs %zu)", (size_t)f->nkmers, (size_t)seen_kmers);
    if (f->nlinks != seen_links) die("[LoadPathError] header number of links don't match seen (exp %zu vs %zu)", (size_t)f->nlinks, (size_t)seen_links);
    char a[64], b[64], k[64];
    status("[GPathReader] Loaded %s of %s links on %s kmers from %s", ulong_to_str(kept, a), ulong_to_str(seen_links, b), ulong_to_str(seen_kmers, k), f->path);
  }

  /* ---- the totals, then header, comment block and body ---- */
  mcx_pjoin_stats st;
  mcx_check(mcx_pjoin_finish(P, NULL, NULL, &st), "pjoin");
  status("Got %zu path bytes", (size_t)st.path_bytes);
  hdr.len = 0;
  why = ctp_merge_header(&hdr, min, nfiles, kmer_size, output_ncols, file_key, command.b, st.kmers, st.links, st.path_bytes, errbuf, sizeof(errbuf));
  if (why) die("%s", why);
  gzFile out = to_stdout ? gzdopen(dup(STDOUT_FILENO), "w") : gzopen(out_path, "w");
  if (!out) die("Cannot open output file: %s [%s]", out_path, strerror(errno));
  if (gz_sink(out, hdr.b, hdr.len) || gzputs(out, "\n\n") < 0 || gzputs(out, ctp_comment) < 0) die("Cannot write to output: %s", out_path);
  mcx_check(mcx_pjoin_finish(P, gz_sink, out, &st), "pjoin");
  if (gzclose(out) != Z_OK) die("Cannot write to output: %s", out_path);

  char pnum[64], pbytes[64], pkmers[64];
  status("Paths written to: %s\n", outpath(out_path));
  status("  %s paths, %s path-bytes, %s kmers", ulong_to_str(st.links, pnum), bytes_to_str(st.path_bytes, 1, pbytes), ulong_to_str(st.kmers, pkmers));

  mcx_pjoin_destroy(P);
  for (size_t i = 0; i < nfiles; i++) { free(files[i].path); free(files[i].raw.b); free(files[i].filter); }
  free(files); free(min); free(command.b); free(hdr.b);
  return EXIT_SUCCESS;
}
