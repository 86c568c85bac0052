/* ctp_hdr_check.c -- the .ctp header reader / editor and the piece cutter of `links` (mccortex_amd/host/ctp_hdr.c) in a
 * program of their own, built under the address and undefined-behaviour sanitizers (test_ctp_hdr_check.py).  Every
 * buffer handed to the code under test is a malloc of exactly the bytes it may touch. */
#include "host.h"

#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "ctp_hdr_check: line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static char *exact(const char *s, size_t n)
{
  char *p = malloc(n ? n : 1);
  CHECK(p);
  memcpy(p, s, n);
  return p;
}

static const char HDR[] =
  "{\n  \"file_format\": \"ctp\",\n  \"format_version\": 4,\n  \"file_key\": \"0123456789abcdef\",\n"
  "  \"note\": \"braces } { and a quote \\\" and ] [ in a string, \\\\\",\n"
  "  \"graph\": {\"num_colours\": 1, \"kmer_size\": 31, \"colours\": [{\"sample\": \"}\\\"{\", \"total_sequence\": 12}]},\n"
  "  \"commands\": [{\"key\": \"aabbccdd\", \"cmd\": [\"x\", \"}\"], \"prev\": []}, {\"key\": \"11223344\", \"prev\": []}],\n"
  "  \"paths\": {\"num_kmers_with_paths\": 10, \"contig_hists\": [{\"lengths\": [1, 2]}], \"num_paths\": 20, \"path_bytes\": 30}\n}";

static void check_header(void)
{
  const size_t n = strlen(HDR);
  /* the span: with a tail behind it, cut short at every length, and not an object at all */
  char *withtail = exact(HDR, n);
  CHECK(ctp_hdr_span(withtail, n) == n);
  free(withtail);
  char *t2 = malloc(n + 7);
  CHECK(t2);
  memcpy(t2, HDR, n);
  memcpy(t2 + n, "\n\n# {c\n", 7);
  CHECK(ctp_hdr_span(t2, n + 7) == n);
  free(t2);
  for (size_t cut = 0; cut < n; cut++) {
    char *part = exact(HDR, cut);
    CHECK(ctp_hdr_span(part, cut) == 0);
    free(part);
  }
  CHECK(ctp_hdr_span("  [1]", 5) == (size_t)-1);
  CHECK(ctp_hdr_span("x", 1) == (size_t)-1);

  char *h = exact(HDR, n);
  uint64_t v = 0;
  CHECK(ctp_hdr_number(h, n, "format_version", NULL, &v) && v == 4);
  CHECK(ctp_hdr_number(h, n, "graph", "kmer_size", &v) && v == 31);
  CHECK(ctp_hdr_number(h, n, "graph", "num_colours", &v) && v == 1);
  CHECK(ctp_hdr_number(h, n, "paths", "path_bytes", &v) && v == 30); /* a number at the end of an object */
  CHECK(ctp_hdr_number(h, n, "paths", "num_paths", &v) && v == 20);
  CHECK(!ctp_hdr_number(h, n, "paths", "lengths", &v));              /* (deeper than one level: not a member) */
  CHECK(!ctp_hdr_number(h, n, "file_key", NULL, &v) && !ctp_hdr_number(h, n, "nothing", NULL, &v));
  char key[16];
  CHECK(ctp_hdr_first_command_key(h, n, key, sizeof(key)) && !strcmp(key, "aabbccdd"));
  char tiny[4];
  CHECK(!ctp_hdr_first_command_key(h, n, tiny, sizeof(tiny)));

  const char *why = NULL;
  size_t m = 0;
  char *e = ctp_hdr_edit(h, n, "fedcba9876543210", "{\"key\": \"99999999\", \"prev\": [\"aabbccdd\"]}", 7, 123456789012ull, 0, &m, &why);
  CHECK(e && m == strlen(e));
  CHECK(ctp_hdr_span(e, m) == m);
  CHECK(strstr(e, "\"file_key\": \"fedcba9876543210\"") && !strstr(e, "0123456789abcdef"));
  CHECK(strstr(e, "\"commands\": [{\"key\": \"99999999\", \"prev\": [\"aabbccdd\"]}, {\"key\": \"aabbccdd\""));
  CHECK(strstr(e, "{\"num_kmers_with_paths\": 7, \"contig_hists\": [{\"lengths\": [1, 2]}], \"num_paths\": 123456789012, \"path_bytes\": 0}\n}"));
  CHECK(strstr(e, "\"note\": \"braces } { and a quote \\\" and ] [ in a string, \\\\\""));
  CHECK(ctp_hdr_first_command_key(e, m, key, sizeof(key)) && !strcmp(key, "99999999"));
  free(e);
  free(h);

  /* an empty commands array; a header without one of the totals */
  static const char H2[] = "{\"file_key\":\"k\",\"commands\":[ ],\"paths\":{\"num_kmers_with_paths\":1,\"num_paths\":2,\"path_bytes\":3}}";
  h = exact(H2, strlen(H2));
  CHECK(!ctp_hdr_first_command_key(h, strlen(H2), key, sizeof(key)));
  e = ctp_hdr_edit(h, strlen(H2), "K2", "{\"key\":\"c\"}", 4, 5, 6, &m, &why);
  CHECK(e && !strcmp(e, "{\"file_key\":\"K2\",\"commands\":[{\"key\":\"c\"} ],\"paths\":{\"num_kmers_with_paths\":4,\"num_paths\":5,\"path_bytes\":6}}"));
  free(e);
  free(h);
  static const char H3[] = "{\"file_key\":\"k\",\"commands\":[],\"paths\":{\"num_kmers_with_paths\":1,\"num_paths\":2}}";
  h = exact(H3, strlen(H3));
  CHECK(!ctp_hdr_edit(h, strlen(H3), "K2", "{}", 4, 5, 6, &m, &why) && !strcmp(why, "path_bytes"));
  free(h);
  ctp_str cmd = {NULL, 0, 0};
  char *argv[2] = {"links", "a \"quoted\" arg"};
  ctp_hdr_command(&cmd, "12345678", 2, argv, "no/such/dir/out.ctp.gz", "fedcba9876543210", "aabbccdd");
  CHECK(ctp_hdr_span(cmd.b, cmd.len) == cmd.len && strstr(cmd.b, "\"prev\": [\"aabbccdd\"]") && strstr(cmd.b, "\"a \\\"quoted\\\" arg\""));
  const char *b, *en;
  CHECK(ctp_json_member(cmd.b, cmd.b + cmd.len, "out_key", &b, &en) && en - b == 18);
  free(cmd.b);
}

/* ---- pieces ---- */
typedef struct { const char *data; size_t n, at, step; } src;
static int src_read(void *ctx, void *dst, unsigned want)
{
  src *s = ctx;
  size_t m = s->n - s->at;
  if (m > want) m = want;
  if (m > s->step) m = s->step; /* short reads, as a gzip stream gives them */
  memcpy(dst, s->data + s->at, m);
  s->at += m;
  return (int)m;
}
static char *cur_buf = NULL;
static int ngrown = 0;
static char *grow(void *ctx, size_t bytes)
{
  (void)ctx;
  free(cur_buf); /* the old buffer is gone, as with the pinned one */
  cur_buf = malloc(bytes);
  CHECK(cur_buf);
  ngrown++;
  return cur_buf;
}

/* the body through pieces of `cap` bytes: the pieces add up to the body (plus the newline a file may lack), each is
 * whole k-mer blocks, ends behind a newline and begins with a k-mer line or what precedes the first */
static int run_pieces(const char *body, size_t n, size_t cap, size_t step, size_t preload)
{
  src s = {body, n, preload, step};
  ctp_pieces P;
  ngrown = 0;
  ctp_pieces_init(&P, grow(NULL, cap), cap, src_read, &s, grow, NULL);
  ctp_pieces_preload(&P, body, preload);
  char *all = malloc(n + 2);
  CHECK(all);
  size_t at = 0;
  int npieces = 0;
  long long len;
  while ((len = ctp_pieces_next(&P)) != 0) {
    CHECK(len > 0 && at + (size_t)len <= n + 1);
    CHECK(P.buf[len - 1] == '\n');
    if (npieces) CHECK(strchr("ACGT", P.buf[0]) && P.buf[0]);
    for (long long i = 1; i < len; i++) /* no piece ends inside a line */
      CHECK(P.buf[i - 1] == '\n' || P.buf[i - 1] != '\0');
    memcpy(all + at, P.buf, (size_t)len);
    at += (size_t)len;
    npieces++;
  }
  const bool lacks = n && body[n - 1] != '\n';
  CHECK(at == n + (lacks ? 1 : 0) && !memcmp(all, body, n) && (!lacks || all[n] == '\n'));
  free(all);
  free(cur_buf);
  cur_buf = NULL;
  return npieces;
}

static void check_pieces(void)
{
  CHECK(ctp_cut("ACGTA 1\nF 1\nCC", 14) == 12);  /* the piece ends before a k-mer line that is not whole */
  CHECK(ctp_cut("ACGTA 1\nF 1\n", 12) == 0);     /* one block: nothing to cut at */
  CHECK(ctp_cut("# c\n\nACGTA 1\nF 1\n", 17) == 5);
  CHECK(ctp_cut("", 0) == 0 && ctp_cut("A", 1) == 0);
  char *one = exact("\nA", 2);
  CHECK(ctp_cut(one, 2) == 1);
  free(one);

  ctp_str body = {NULL, 0, 0};
  ctp_str_add(&body, "# head\n\n", 8);
  for (int i = 0; i < 40; i++) {
    char line[600];
    snprintf(line, sizeof(line), "ACGT%c 2\nF 1 %d A seq=ACGTAA juncpos=0\n# c\nR 1 1 C seq=TACGTC juncpos=0\n\n", "ACGT"[i & 3], i);
    ctp_str_add(&body, line, strlen(line));
    if (i == 17) { /* a block larger than any of the small buffers */
      ctp_str_add(&body, "GGGGG 60\n", 9);
      for (int j = 0; j < 60; j++) ctp_str_add(&body, "F 1 1 A seq=GGGGGA juncpos=0\n", 29);
    }
  }
  char *b = exact(body.b, body.len);
  CHECK(run_pieces(b, body.len, 1u << 20, 1u << 20, 0) == 1 && ngrown == 1);
  CHECK(run_pieces(b, body.len, 100, 7, 0) > 10 && ngrown > 1);   /* the buffer grows for the large block */
  CHECK(run_pieces(b, body.len, 64, 1, 30) > 2);
  CHECK(run_pieces(b, body.len, 200, 1000, 150) > 5);              /* bytes the header reader had already */
  for (size_t cap = 64; cap < 140; cap++) CHECK(run_pieces(b, body.len, cap, 13, cap % 9) > 1);
  free(b);
  /* a file without a trailing newline; a file that ends inside a k-mer line; an empty body */
  b = exact(body.b, body.len - 2);
  CHECK(run_pieces(b, body.len - 2, 90, 5, 0) > 2);
  free(b);
  static const char T[] = "ACGTA 1\nF 1 1 A seq=ACGTAA juncpos=0\nCCC";
  b = exact(T, strlen(T));
  CHECK(run_pieces(b, strlen(T), 64, 3, 0) == 1);  /* the end of the input: the rest is the last piece, the engine refuses the half line */
  CHECK(run_pieces(b, strlen(T), 41, 3, 0) == 2);  /* the newline that is added has its byte */
  CHECK(run_pieces(b, 0, 64, 3, 0) == 0);
  free(b);
  free(body.b);
}

int main(void)
{
  msg_out = NULL;
  check_header();
  check_pieces();
  puts("ctp_hdr_check: ok");
  return 0;
}
