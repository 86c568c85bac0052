/* cmd_links.c -- `mccortex<K> links` (src/commands/ctx_links.c): clean, list and count the links of a .ctp file.  The
 * reference's usage text, option table, argument checks and output files; the per-k-mer tree of src/paths/link_tree.c
 * is computed on the MI355X (mcx_links_add_text), the body streaming through it in pieces of whole k-mer blocks
 * (ctp_hdr.c).  As the reference does, the cleaned body goes to an unlinked temporary file next to the output and the
 * edited header, an empty line, a comment block and the body are written at the end, when the totals are known.
 *
 * Where this differs from the reference (DESIGN.md lists it): format version 4 only; -P, --plot is refused; -T is
 * refused together with -D below 6 or -C below 10 (the reference reads six distances whatever -D says and asserts ten
 * coverage bins); without -o nothing is saved (the usage's "default: STDOUT" is not what the reference does either);
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

#define DEFAULT_MAX_DIST 6
#define DEFAULT_MAX_COVG 100

static const char links_usage[] =
"usage: " CMD_NAME " links [options] <in.ctp.gz>\n"
"\n"
"  Clean, minimise and list cortex links. Works on a stream of input only,\n"
"  so memory usage is very low.\n"
"\n"
"  -h,--help               This help message\n"
"  -q,--quiet              Silence status output normally printed to STDERR\n"
"  -f,--force              Overwrite output files\n"
"  -o,--out <out.ctp.gz>   Save output link file [default: STDOUT]\n"
"\n"
"  -L,--limit <N>          Only use links from first N kmers\n"
"\n"
"One or more of:\n"
"  -l,--list <out.txt>     List as CSV links\n"
"  -P,--plot <out.dot>     Plot last from limit\n"
"  -c,--clean <N>          Remove junction choices with coverage < N\n"
"  -T,--threshold <t.txt>  Calculate the cleaning threshold, write to file\n"
"  -H,--covg-hist <f.csv>  Write link coverage matrix to a csv file\n"
"  -D,--max-dist <max>     Set max dist when using --covg-hist ...\n"
"  -C,--max-covg <max>     Set max covg when using --covg-hist ...\n"
"      --device <N>        GPU to run on [default: 0]\n"
"\n";

static const char ctp_comment[] =
"# Links cleaned by " CMD_NAME " links\n"
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
  {"help", no_argument, NULL, 'h'},           {"out", required_argument, NULL, 'o'},       {"force", no_argument, NULL, 'f'},
  {"list", required_argument, NULL, 'l'},     {"clean", required_argument, NULL, 'c'},     {"plot", required_argument, NULL, 'P'},
  {"threshold", required_argument, NULL, 'T'}, {"covg-hist", required_argument, NULL, 'H'}, {"max-dist", required_argument, NULL, 'D'},
  {"max-covg", required_argument, NULL, 'C'}, {"limit", required_argument, NULL, 'L'},     {"device", required_argument, NULL, OPT_DEVICE},
  {NULL, 0, NULL, 0}};

#define ONCE(seen) do { if (seen) print_usage(links_usage, "%s given twice", cmd); } while (0)

static size_t size_arg(const char *cmd, const char *arg)
{
  size_t v;
  if (!parse_entire_size(arg, &v)) print_usage(links_usage, "%s requires an int x >= 0: %s", cmd, arg);
  return v;
}

static bool check_outfile(const char *path, bool force)
{
  const bool err = path && !force && access(path, F_OK) != -1;
  if (err) warn("File already exists: %s", path);
  return err;
}

static int file_sink(void *ctx, const void *data, size_t nbytes) { return fwrite(data, 1, nbytes, (FILE *)ctx) != nbytes; }
static int gz_read(void *ctx, void *dst, unsigned n) { return gzread((gzFile)ctx, dst, n); }
static char *grow_pinned(void *ctx, size_t bytes)
{
  void *p = NULL;
  mcx_check(mcx_links_buffer((mcx_links *)ctx, bytes, &p), "links");
  return p;
}

/* create_tmp_file: <base>.tmp.<rand>, unlinked at once */
static FILE *create_tmp_file(const char *base, char *path, size_t pathlen)
{
  size_t i;
  for (i = 0; i < 100; i++) {
    snprintf(path, pathlen, "%s.tmp.%04zu", base, (size_t)(rand() % 9999));
    if (access(path, F_OK) == -1) break;
  }
  if (i == 100) die("Temporary files already exist (%zu tries): %s", (size_t)100, path);
  FILE *fh = fopen(path, "w+");
  if (!fh) die("Cannot write temporary file: %s [%s]", path, strerror(errno));
  unlink(path);
  return fh;
}

static int size_cmp(const void *a, const void *b)
{
  const size_t x = *(const size_t *)a, y = *(const size_t *)b;
  return x < y ? -1 : x > y;
}

/* print_suggest_cutoff (ctx_links.c:82-115) over distances 1 .. distsize - 1 */
static void print_suggest_cutoff(size_t distsize, size_t covgsize, const uint64_t *hists, FILE *fh)
{
  size_t cutoffs[distsize], sumcovgs[distsize], nfailed = 0;
  memset(cutoffs, 0, sizeof(cutoffs));
  memset(sumcovgs, 0, sizeof(sumcovgs));
  for (size_t dist = 1; dist < distsize; dist++) {
    int t = cleaning_pick_kmer_threshold(hists + dist * covgsize, covgsize, NULL, NULL, NULL, NULL);
    if (t < 0) { nfailed++; t = 0; }
    cutoffs[dist] = (size_t)t;
    for (size_t i = 0; i < covgsize; i++) sumcovgs[dist] += hists[dist * covgsize + i];
  }
  fprintf(fh, "sumcovgs=%zu", sumcovgs[1]);
  for (size_t i = 2; i < distsize; i++) fprintf(fh, ",%zu", sumcovgs[i]);
  fprintf(fh, "\ncutoffs=%zu", cutoffs[1]);
  for (size_t i = 2; i < distsize; i++) fprintf(fh, ",%zu", cutoffs[i]);
  fprintf(fh, "\n");
  qsort(cutoffs + 1, distsize - 1, sizeof(size_t), size_cmp); /* gca_median_size: the middle of the five */
  fprintf(fh, "suggested_cutoff=%zu\n", cutoffs[1 + (distsize - 1) / 2]);
  if (nfailed) warn("Threshold failed in %zu cases [default to 0]", nfailed);
}

static const char *const refusals[] = {
  "", "Bad kmer line", "Bad link line: the first column is not F or R", "Bad link line: a column is not a number",
  "Can only clean a single colour at a time. Sorry. (a link line counts several colours)", "Non-ACGT base in junction choices",
  "Bad link line: the number of junctions is 0 or above 32767", "Differing lengths: the junction count is not the length of the junction string",
  "Link line without seq=", "Link line without juncpos=", "Cannot parse juncpos=, or its length is not the number of junctions", "Seq too short or too long for juncpos",
  "Bad entry: seq does not hold the junction base at a junction position", "Bad link line: a link before any k-mer line"};

int ctx_links(int argc, char **argv)
{
  size_t limit = 0, hist_distsize = 0, hist_covgsize = 0, cutoff = 0;
  const char *link_out_path = NULL, *csv_out_path = NULL, *thresh_path = NULL, *hist_path = NULL;
  bool clean = false, force = false;
  unsigned device = 0;
  char cmd[100];
  int c;
  optind = 1;
  while ((c = getopt_long_only(argc, argv, "ho:fl:c:P:T:H:D:C:L:", longopts, NULL)) != -1) {
    cmd_optname(longopts, c, cmd);
    switch (c) {
      case 'h': print_usage(links_usage, NULL);
      case 'o': ONCE(link_out_path); link_out_path = optarg; break;
      case 'f': ONCE(force); force = true; break;
      case 'l': ONCE(csv_out_path); csv_out_path = optarg; break;
      case 'c': ONCE(cutoff); cutoff = size_arg(cmd, optarg); clean = true; break;
      case 'L': ONCE(limit); limit = size_arg(cmd, optarg); break;
      case 'P': die("-P, --plot <out.dot> is not part of this build's `links`");
      case 'T': ONCE(thresh_path); thresh_path = optarg; break;
      case 'H': ONCE(hist_path); hist_path = optarg; break;
      case 'C': ONCE(hist_covgsize); hist_covgsize = size_arg(cmd, optarg); break;
      case 'D': ONCE(hist_distsize); hist_distsize = size_arg(cmd, optarg); break;
      case OPT_DEVICE: if (!parse_entire_uint(optarg, &device)) print_usage(links_usage, "%s requires an int x >= 0: %s", cmd, optarg); break;
      case ':': case '?': die("`" CMD_NAME " links -h` for help. Bad option: %s", argv[optind - 1]);
      default: abort();
    }
  }
  if (hist_distsize && !hist_path) print_usage(links_usage, "--max-dist without --covg-hist");
  if (hist_covgsize && !hist_path) print_usage(links_usage, "--max-covg without --covg-hist");
  if (thresh_path && hist_distsize && hist_distsize < 6) die("-T, --threshold <t.txt> reads the distances 1 to 5: -D, --max-dist <max> must be at least 6 with it");
  if (thresh_path && hist_covgsize && hist_covgsize < 10) die("-T, --threshold <t.txt> needs ten coverage bins: -C, --max-covg <max> must be at least 10 with it");
  if (!hist_distsize) hist_distsize = DEFAULT_MAX_DIST;
  if (!hist_covgsize) hist_covgsize = DEFAULT_MAX_COVG;
  if (optind + 1 != argc) print_usage(links_usage, "Wrong number of arguments");
  const char *ctp_path = argv[optind];
  const bool list = csv_out_path != NULL, save = link_out_path != NULL, hist_covg = thresh_path != NULL || hist_path != NULL;
  if (clean && !save) print_usage(links_usage, "Need to give --out <out.ctp.gz> with --clean");
  if (!save && !list && !hist_covg) print_usage(links_usage, "Please specify one of --plot, --list or --clean");
  if (link_out_path && hist_covg && strcmp(link_out_path, "-") == 0) print_usage(links_usage, "Outputing both cleaning threshold (-T) and links (-o) to STDOUT!");
  if (hist_distsize > (1u << 20) || hist_covgsize > (1u << 20) || hist_distsize * hist_covgsize > (1u << 26)) die("--max-dist x --max-covg is too large");
  bool err = false;
  err |= check_outfile(csv_out_path, force);
  err |= check_outfile(link_out_path, force);
  err |= check_outfile(thresh_path, force);
  err |= check_outfile(hist_path, force);
  if (err) die("Use -f,--force to overwrite files");

  /* gpath_reader_open: the header object, then the body */
  gzFile in = strcmp(ctp_path, "-") == 0 ? gzdopen(dup(STDIN_FILENO), "r") : gzopen(ctp_path, "r");
  if (!in) die("Cannot open file: %s", ctp_path);
  gzbuffer(in, 1u << 20);
  ctp_str raw = {NULL, 0, 0};
  size_t hdr_len = 0;
  while (true) {
    char tmp[4096];
    const int got = gzread(in, tmp, sizeof(tmp));
    if (got < 0) die("Cannot read file: %s", ctp_path);
    if (got > 0) ctp_str_add(&raw, tmp, (size_t)got);
    hdr_len = raw.len ? ctp_hdr_span(raw.b, raw.len) : 0;
    if (hdr_len == (size_t)-1) die("Expected JSON header: %s", ctp_path);
    if (hdr_len) break;
    if (got == 0) die("Cannot find end of JSON header: %s", ctp_path);
  }
  uint64_t version = 0, ncols = 0, kmer_size = 0, nkmers0 = 0, nlinks0 = 0, nbytes0 = 0;
  const char *fb, *fe;
  if (!ctp_json_member(raw.b, raw.b + hdr_len, "file_format", &fb, &fe) || fe - fb != 5 || memcmp(fb, "\"ctp\"", 5))
    die("File is not a link file (file_format is not \"ctp\"): %s", ctp_path);
  if (!ctp_hdr_number(raw.b, hdr_len, "format_version", NULL, &version)) die("Cannot find format_version in header: %s", ctp_path);
  if (version != 4) die("Only link files of format version 4 are read, this one has version %llu: %s", (unsigned long long)version, ctp_path);
  if (!ctp_hdr_number(raw.b, hdr_len, "graph", "num_colours", &ncols) || !ctp_hdr_number(raw.b, hdr_len, "graph", "kmer_size", &kmer_size))
    die("Cannot find graph.num_colours and graph.kmer_size in header: %s", ctp_path);
  if (kmer_size < MIN_KMER_SIZE || kmer_size > MAX_KMER_SIZE || !(kmer_size & 1))
    die("kmer size %llu is not an odd number within %d..%d: %s", (unsigned long long)kmer_size, MIN_KMER_SIZE, MAX_KMER_SIZE, ctp_path);
  if (ncols != 1) die("Can only clean a single colour at a time. Sorry.");
  if (!ctp_hdr_number(raw.b, hdr_len, "paths", "num_kmers_with_paths", &nkmers0) || !ctp_hdr_number(raw.b, hdr_len, "paths", "num_paths", &nlinks0) ||
      !ctp_hdr_number(raw.b, hdr_len, "paths", "path_bytes", &nbytes0))
    die("Cannot find required header entries");

  FILE *hist_fh = NULL, *thresh_fh = NULL, *list_fh = NULL, *tmp_fh = NULL;
  gzFile out_gz = NULL;
  char tmp_path[4200];
  if (hist_path && !(hist_fh = fopen(hist_path, "w"))) die("Cannot open file: %s", hist_path);
  if (thresh_path && !(thresh_fh = fopen(thresh_path, "w"))) die("Cannot open file: %s", thresh_path);
  if (limit) status("Limiting to the first %zu kmers", limit);
  if (clean) status(" Cleaning coverage below %zu", cutoff);
  char file_key[17], cmd_key[9], prev_key[64];
  ctp_str command = {NULL, 0, 0};
  if (save) {
    const bool to_stdout = strcmp(link_out_path, "-") == 0;
    tmp_fh = create_tmp_file(to_stdout ? "links" : link_out_path, tmp_path, sizeof(tmp_path));
    status("Saving output to: %s", outpath(link_out_path));
    status("Temporary output: %s", tmp_path);
    out_gz = to_stdout ? gzdopen(dup(STDOUT_FILENO), "w") : gzopen(link_out_path, "w");
    if (!out_gz) die("Cannot open output link file: %s", link_out_path);
    ctp_hex_key(file_key, 16);
    ctp_hex_key(cmd_key, 8);
    const bool have_prev = ctp_hdr_first_command_key(raw.b, hdr_len, prev_key, sizeof(prev_key));
    ctp_hdr_command(&command, cmd_key, argc, argv, link_out_path, file_key, have_prev ? prev_key : NULL);
  }
  if (list) {
    status("Listing to %s", csv_out_path);
    if (!(list_fh = fopen(csv_out_path, "w"))) die("Cannot open output CSV file %s", csv_out_path);
    fprintf(list_fh, "SeqLen,Covg\n");
  }

  mcx_links *L = NULL;
  mcx_check(mcx_links_create(&L, (int)kmer_size, (int)device), "links");
  size_t cap = 64u << 20;
  if (getenv("MCX_LINKS_PIECE")) cap = strtoul(getenv("MCX_LINKS_PIECE"), NULL, 10); /* (tests: pieces of a few hundred bytes) */
  if (cap < 64) cap = 64;
  ctp_pieces P;
  ctp_pieces_init(&P, grow_pinned(L, cap), cap, gz_read, in, grow_pinned, L);
  ctp_pieces_preload(&P, raw.b + hdr_len, raw.len - hdr_len);
  mcx_links_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.flags = (clean ? MCX_LINKS_CLEAN : 0u) | (hist_covg ? MCX_LINKS_HIST : 0u);
  prm.cutoff = cutoff; prm.distsize = (uint32_t)hist_distsize; prm.covgsize = (uint32_t)hist_covgsize;
  mcx_links_stats st;
  memset(&st, 0, sizeof(st));
  uint64_t base = hdr_len;
  long long n;
  while ((!limit || st.kmers_read < limit) && (n = ctp_pieces_next(&P)) != 0) {
    if (n < 0) die("Cannot read file: %s", ctp_path);
    prm.max_kmers = limit ? limit - st.kmers_read : 0;
    const int rc = mcx_links_add_text(L, P.buf, (uint64_t)n, &prm, save ? file_sink : NULL, tmp_fh, list ? file_sink : NULL, list_fh);
    if (rc == MCX_ERR_INVAL) {
      int code = 0;
      uint64_t off = 0;
      mcx_links_error(L, &code, &off);
      const char *line = P.buf + off, *nl = memchr(line, '\n', (size_t)n - off);
      die("%s [%s, byte %llu behind the header]: %.*s", code > 0 && code < 14 ? refusals[code] : "Bad line", ctp_path, (unsigned long long)(base - hdr_len + off),
          (int)((nl ? nl : P.buf + n) - line > 200 ? 200 : (nl ? nl : P.buf + n) - line), line);
    }
    mcx_check(rc, "links");
    mcx_check(mcx_links_get_stats(L, &st), "links");
    base += (uint64_t)n;
  }
  gzclose(in);

  status("Number of kmers with links %llu -> %llu", (unsigned long long)nkmers0, (unsigned long long)st.kmers_with_links);
  status("Number of links %llu -> %llu", (unsigned long long)nlinks0, (unsigned long long)st.links);
  status("Number of bytes %llu -> %llu", (unsigned long long)nbytes0, (unsigned long long)st.link_bytes);

  if (save) {
    const char *why = NULL;
    size_t new_len = 0;
    char *hdr = ctp_hdr_edit(raw.b, hdr_len, file_key, command.b, st.kmers_with_links, st.links, st.link_bytes, &new_len, &why);
    if (!hdr) die("Cannot find required header entries: %s", why);
    if (gzwrite(out_gz, hdr, (unsigned)new_len) != (int)new_len) die("Cannot write ctp file to: %s", link_out_path);
    free(hdr);
    gzputs(out_gz, "\n\n");
    gzputs(out_gz, ctp_comment);
    if (fseek(tmp_fh, 0, SEEK_SET) != 0) die("fseek failed: %s", strerror(errno));
    char *tmp = malloc(4u << 20);
    if (!tmp) die("Out of memory");
    size_t s;
    while ((s = fread(tmp, 1, 4u << 20, tmp_fh)) > 0)
      if (gzwrite(out_gz, tmp, (unsigned)s) != (int)s) die("Cannot write to output: %s", link_out_path);
    free(tmp);
    if (gzclose(out_gz) != Z_OK) die("Cannot write to output: %s", link_out_path);
    fclose(tmp_fh);
  }
  if (hist_covg) {
    uint64_t *hists = calloc(hist_distsize * hist_covgsize, sizeof(uint64_t));
    if (!hists) die("Out of memory");
    if (st.links_in) mcx_check(mcx_links_hist(L, hists), "links"); /* (no link line: nothing was ever counted) */
    if (hist_fh) { /* ctx_links.c:398-411 */
      fprintf(hist_fh, "  ");
      for (size_t j = 1; j < hist_covgsize; j++) fprintf(hist_fh, ",covg.%02zu", j);
      fprintf(hist_fh, "\n");
      for (size_t i = 1; i < hist_distsize; i++) {
        fprintf(hist_fh, "dist.%02zu", i);
        for (size_t j = 1; j < hist_covgsize; j++) fprintf(hist_fh, ",%llu", (unsigned long long)hists[i * hist_covgsize + j]);
        fprintf(hist_fh, "\n");
      }
      fclose(hist_fh);
    }
    if (thresh_fh) {
      print_suggest_cutoff(6, hist_covgsize, hists, thresh_fh);
      fclose(thresh_fh);
    }
    free(hists);
  }
  if (list) fclose(list_fh);
  free(raw.b);
  free(command.b);
  mcx_links_destroy(L);
  return EXIT_SUCCESS;
}
