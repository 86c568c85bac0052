/* ctp_merge_check.c -- the header merger of `pjoin` (mccortex_amd/host/ctp_merge.c over ctp_hdr.c) in a program of its
 * own, built under the address and undefined-behaviour sanitizers (test_ctp_merge_check.py).  Every header handed to the
 * code under test is a malloc of exactly its bytes. */
#define _GNU_SOURCE
#include "host.h"

#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "ctp_merge_check: line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

static char *exact(const char *s, size_t n)
{
  char *p = malloc(n ? n : 1);
  CHECK(p);
  memcpy(p, s, n);
  return p;
}
static bool is(const char *b, const char *e, const char *want) { return (size_t)(e - b) == strlen(want) && !memcmp(b, want, strlen(want)); }
static bool has(const ctp_str *s, const char *want) { return s->b && strstr(s->b, want) != NULL; }
static size_t count(const ctp_str *s, const char *want)
{
  size_t n = 0;
  for (const char *p = s->b; (p = strstr(p, want)) != NULL; p += strlen(want)) n++;
  return n;
}

/* quotes and braces inside sample names, a colour without a histogram entry's worth of contigs, three commands */
static const char A[] =
  "{\n  \"file_format\": \"ctp\",\n  \"format_version\": 4,\n  \"file_key\": \"0123456789abcdef\",\n"
  "  \"graph\": {\"num_colours\": 2, \"kmer_size\": 9, \"colours\": [{\"colour\": 0, \"sample\": \"s0 {\\\"} ]\", \"total_sequence\": 12},"
  " {\"sample\": \"}\\\\\", \"colour\": 1}]},\n"
  "  \"commands\": [{\"key\": \"cccc\", \"cmd\": [\"links\", \"]\"], \"prev\": [\"aaaa\"]}, {\"key\": \"aaaa\", \"prev\": []}, {\"nokey\": 1}, {\"key\": \"bbbb\"}],\n"
  "  \"paths\": {\"num_kmers_with_paths\": 10, \"num_paths\": 20, \"path_bytes\": 30,"
  " \"contig_hists\": [{\"lengths\": [0, 20, 31], \"counts\": [9, 2, 4]}, {\"lengths\": [], \"counts\": []}]}\n}";
/* an empty commands array; the same name for colour 0 */
static const char B[] =
  "{\"file_format\": \"ctp\", \"format_version\": 4, \"file_key\": \"x\", \"graph\": {\"num_colours\": 1, \"kmer_size\": 9,"
  " \"colours\": [{\"colour\": 0, \"sample\": \"s0 {\\\"} ]\"}]}, \"commands\": [],"
  " \"paths\": {\"num_kmers_with_paths\": 1, \"num_paths\": 1, \"path_bytes\": 1, \"contig_hists\": [{\"lengths\": [40,31 , 20], \"counts\": [5, 1,0]}]}}";
/* a command key both have; another name */
static const char C[] =
  "{\"file_format\": \"ctp\", \"format_version\": 4, \"file_key\": \"x\", \"graph\": {\"num_colours\": 1, \"kmer_size\": 9,"
  " \"colours\": [{\"colour\": 0, \"sample\": \"other\"}]}, \"commands\": [{\"key\": \"aaaa\", \"prev\": []}, {\"key\": \"dddd\", \"prev\": []}],"
  " \"paths\": {\"num_kmers_with_paths\": 1, \"num_paths\": 1, \"path_bytes\": 1, \"contig_hists\": [{\"lengths\": [7], \"counts\": [3, 4]}]}}";

static const char COMMAND[] = "{\n      \"key\": \"kkkk\",\n      \"cmd\": [\"mccortex31\", \"pjoin\"],\n      \"prev\": []\n    }";

int main(void)
{
  char *a = exact(A, strlen(A)), *b = exact(B, strlen(B)), *c = exact(C, strlen(C));
  const size_t na = strlen(A), nb = strlen(B), nc = strlen(C);
  const char *vb, *ve, *kb, *ke;

  CHECK(ctp_hdr_sample(a, na, 0, &vb, &ve) && is(vb, ve, "\"s0 {\\\"} ]\""));
  CHECK(ctp_hdr_sample(a, na, 1, &vb, &ve) && is(vb, ve, "\"}\\\\\""));
  CHECK(!ctp_hdr_sample(a, na, 2, &vb, &ve));
  CHECK(ctp_hdr_sample(b, nb, 0, &vb, &ve) && !ctp_hdr_sample(b, nb, 1, &vb, &ve));

  ctp_hist h = {NULL, NULL, 0, 0};
  CHECK(ctp_hdr_hist_add(a, na, 0, &h) && h.n == 2 && h.len[0] == 20 && h.cnt[0] == 2 && h.len[1] == 31 && h.cnt[1] == 4); /* length 0 is left out */
  CHECK(ctp_hdr_hist_add(b, nb, 0, &h) && h.n == 3 && h.cnt[0] == 2 && h.cnt[1] == 5 && h.len[2] == 40 && h.cnt[2] == 5);  /* a zero count adds nothing */
  CHECK(ctp_hdr_hist_add(a, na, 1, &h) && h.n == 3);  /* a histogram with no entries */
  CHECK(!ctp_hdr_hist_add(a, na, 2, &h));             /* no such colour */
  CHECK(!ctp_hdr_hist_add(c, nc, 0, &h));             /* lists of two lengths */
  ctp_hist_free(&h);
  CHECK(h.n == 0 && h.len == NULL);

  CHECK(ctp_hdr_command_at(a, na, 0, &vb, &ve, &kb, &ke) && is(kb, ke, "\"cccc\"") && *vb == '{' && ve[-1] == '}');
  CHECK(ctp_hdr_command_at(a, na, 2, &vb, &ve, &kb, &ke) && kb == NULL);
  CHECK(ctp_hdr_command_at(a, na, 3, &vb, &ve, &kb, &ke) && is(kb, ke, "\"bbbb\"") && is(vb, ve, "{\"key\": \"bbbb\"}"));
  CHECK(!ctp_hdr_command_at(a, na, 4, &vb, &ve, &kb, &ke));
  CHECK(!ctp_hdr_command_at(b, nb, 0, &vb, &ve, &kb, &ke)); /* an empty array */

  /* a.ctp (two colours) into 0 and 1, b.ctp into 0, colour 2 filled by nobody, c.ctp into 3 */
  const col_filter fa[2] = {{0, 0}, {1, 1}}, fb[1] = {{0, 0}}, fc[1] = {{0, 3}};
  ctp_merge_input in[3] = {{a, na, fa, 2, "a.ctp"}, {b, nb, fb, 1, "b.ctp"}, {c, nc, fc, 1, "c.ctp"}};
  char err[512];
  ctp_str out = {NULL, 0, 0};
  CHECK(ctp_merge_header(&out, in, 3, 9, 4, "fedcba9876543210", COMMAND, 4, 8, 8, err, sizeof(err)) == err); /* c's histogram is broken */
  CHECK(strstr(err, "contig histogram") && strstr(err, "c.ctp"));
  free(out.b);
  out = (ctp_str){NULL, 0, 0};
  CHECK(ctp_merge_header(&out, in, 2, 9, 3, "fedcba9876543210", COMMAND, 4, 8, 8, err, sizeof(err)) == NULL);
  CHECK(ctp_hdr_span(out.b, out.len) == out.len);
  uint64_t v = 0;
  CHECK(ctp_hdr_number(out.b, out.len, "format_version", NULL, &v) && v == 4);
  CHECK(ctp_hdr_number(out.b, out.len, "graph", "num_colours", &v) && v == 3);
  CHECK(ctp_hdr_number(out.b, out.len, "graph", "kmer_size", &v) && v == 9);
  CHECK(ctp_hdr_number(out.b, out.len, "graph", "num_kmers_in_graph", &v) && v == 4);
  CHECK(ctp_hdr_number(out.b, out.len, "paths", "num_paths", &v) && v == 8);
  CHECK(ctp_hdr_sample(out.b, out.len, 0, &vb, &ve) && is(vb, ve, "\"s0 {\\\"} ]\""));
  CHECK(ctp_hdr_sample(out.b, out.len, 1, &vb, &ve) && is(vb, ve, "\"}\\\\\""));
  CHECK(ctp_hdr_sample(out.b, out.len, 2, &vb, &ve) && is(vb, ve, "\"undefined\""));
  CHECK(has(&out, "\"file_key\": \"fedcba9876543210\""));
  /* this command first, its prev the first key of every input that has one; then a's commands that have a key */
  CHECK(ctp_hdr_command_at(out.b, out.len, 0, &vb, &ve, &kb, &ke) && is(kb, ke, "\"kkkk\""));
  CHECK(has(&out, "\"prev\": [\"cccc\"]\n    }"));
  CHECK(ctp_hdr_command_at(out.b, out.len, 1, &vb, &ve, &kb, &ke) && is(kb, ke, "\"cccc\""));
  CHECK(ctp_hdr_command_at(out.b, out.len, 2, &vb, &ve, &kb, &ke) && is(kb, ke, "\"aaaa\""));
  CHECK(ctp_hdr_command_at(out.b, out.len, 3, &vb, &ve, &kb, &ke) && is(kb, ke, "\"bbbb\""));
  CHECK(!ctp_hdr_command_at(out.b, out.len, 4, &vb, &ve, &kb, &ke));
  h = (ctp_hist){NULL, NULL, 0, 0};
  CHECK(ctp_hdr_hist_add(out.b, out.len, 0, &h) && h.n == 3 && h.len[0] == 20 && h.cnt[0] == 2 && h.len[1] == 31 && h.cnt[1] == 5 && h.len[2] == 40 && h.cnt[2] == 5);
  ctp_hist_free(&h);
  CHECK(ctp_hdr_hist_add(out.b, out.len, 1, &h) && h.n == 0 && ctp_hdr_hist_add(out.b, out.len, 2, &h) && h.n == 0 && !ctp_hdr_hist_add(out.b, out.len, 3, &h));
  free(out.b);

  /* a duplicated command key across inputs goes in once; both first keys are previous commands */
  const col_filter f0[1] = {{0, 0}}, f1[1] = {{0, 1}};
  ctp_merge_input two[2] = {{a, na, f0, 1, "a.ctp"}, {c, nc, f1, 1, "c.ctp"}};
  char *c2 = exact(C, nc); /* c with a histogram that can be read */
  char *bad = memmem(c2, nc, "[3, 4]", 6);
  CHECK(bad);
  memcpy(bad, "[3   ]", 6);
  two[1].hdr = c2;
  out = (ctp_str){NULL, 0, 0};
  CHECK(ctp_merge_header(&out, two, 2, 9, 2, "k", COMMAND, 1, 1, 1, err, sizeof(err)) == NULL);
  CHECK(has(&out, "\"prev\": [\"cccc\", \"aaaa\"]\n    }"));
  CHECK(count(&out, "\"key\": \"aaaa\"") == 1 && count(&out, "\"key\": \"dddd\"") == 1);
  CHECK(ctp_hdr_span(out.b, out.len) == out.len);
  free(out.b);
  /* two names for one colour */
  two[1].filter = f0;
  out = (ctp_str){NULL, 0, 0};
  CHECK(ctp_merge_header(&out, two, 2, 9, 2, "k", COMMAND, 1, 1, 1, err, sizeof(err)) == err && strstr(err, "Graph/path sample names do not match [0->0]"));
  /* an into colour beyond the output */
  two[1].filter = f1;
  CHECK(ctp_merge_header(&out, two, 2, 9, 1, "k", COMMAND, 1, 1, 1, err, sizeof(err)) == err);
  free(out.b);
  free(a); free(b); free(c); free(c2);
  printf("ctp_merge_check: ok\n");
  return 0;
}
