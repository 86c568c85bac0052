/* ctp_merge.c -- the header `pjoin` writes, put together from the headers of its inputs as text (ctp_hdr.c finds the
 * members; no JSON tree is built): a colour's sample name, a colour's contig histogram, the entries of "commands" with
 * their keys, and the writer of the merged header (json_hdr_make_std of src/graph/json_hdr.c:188-270 and
 * gpath_save_mkhdr of src/graph_paths/gpath_save.c:62-112).  Strings stay as they stand in the input, escapes and all:
 * two sample names are equal when their JSON texts are, and a name goes out as it came in. */
#define _GNU_SOURCE
#include "host.h"

#include <stdlib.h>
#include <string.h>

static const char *ws(const char *p, const char *e)
{
  while (p < e && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
  return p;
}
/* p at the first byte of a value -> behind its last, or NULL */
static const char *value_end(const char *p, const char *e)
{
  if (p >= e) return NULL;
  size_t depth = 0;
  const char *q = p;
  while (q < e) {
    if (*q == '"') {
      for (q++; q < e && *q != '"'; q++)
        if (*q == '\\') q++;
      if (q >= e) return NULL;
      q++;
      if (!depth) return q;
      continue;
    }
    if (*q == '{' || *q == '[') depth++;
    else if (*q == '}' || *q == ']') {
      if (!depth) return q > p ? q : NULL; /* a bare value ends at its container's bracket */
      if (--depth == 0) return q + 1;
    } else if (!depth && (*q == ',' || *q == ' ' || *q == '\t' || *q == '\n' || *q == '\r')) return q > p ? q : NULL;
    q++;
  }
  return NULL;
}
/* element `idx` of the array [arr, arr_end) (arr at its '['), or false; idx = (size_t)-1 counts: *vbeg is left alone
 * and *count gets the number of elements */
static bool array_item(const char *arr, const char *arr_end, size_t idx, const char **vbeg, const char **vend, size_t *count)
{
  const char *p = ws(arr, arr_end);
  size_t i = 0;
  if (count) *count = 0;
  if (p >= arr_end || *p != '[') return false;
  p = ws(p + 1, arr_end);
  while (p < arr_end && *p != ']') {
    const char *ve = value_end(p, arr_end);
    if (!ve) return false;
    if (i == idx) { *vbeg = p; *vend = ve; return true; }
    i++;
    p = ws(ve, arr_end);
    if (p < arr_end && *p == ',') p = ws(p + 1, arr_end);
    else if (p >= arr_end || *p != ']') return false;
  }
  if (count) *count = i;
  return idx == (size_t)-1 && p < arr_end;
}

/* hdr["graph"]["colours"][colour]["sample"] as it stands, quotes included */
bool ctp_hdr_sample(const char *hdr, size_t n, size_t colour, const char **b, const char **e)
{
  const char *gb, *ge, *cb, *ce, *ob, *oe;
  if (!ctp_json_member(hdr, hdr + n, "graph", &gb, &ge) || !ctp_json_member(gb, ge, "colours", &cb, &ce)) return false;
  if (!array_item(cb, ce, colour, &ob, &oe, NULL) || *ob != '{') return false;
  return ctp_json_member(ob, oe, "sample", b, e) && *b < *e && **b == '"';
}

static bool next_number(const char **p, const char *e, uint64_t *v)
{
  const char *q = ws(*p, e);
  if (q < e && *q == ',') q = ws(q + 1, e);
  if (q >= e || *q < '0' || *q > '9') return false;
  uint64_t x = 0;
  for (; q < e && *q >= '0' && *q <= '9'; q++) x = x * 10 + (uint64_t)(*q - '0');
  *p = q;
  *v = x;
  return true;
}

/* count more contigs of length len; length 0 and a count of 0 are left out (gpath_save.c:38-45 writes neither) */
void ctp_hist_add(ctp_hist *h, uint64_t len, uint64_t count)
{
  if (!len || !count) return;
  size_t lo = 0, hi = h->n;
  while (lo < hi) {
    const size_t mid = (lo + hi) / 2;
    if (h->len[mid] < len) lo = mid + 1;
    else hi = mid;
  }
  if (lo < h->n && h->len[lo] == len) { h->cnt[lo] += count; return; }
  if (h->n == h->cap) {
    h->cap = h->cap ? h->cap * 2 : 16;
    h->len = realloc(h->len, h->cap * sizeof(uint64_t));
    h->cnt = realloc(h->cnt, h->cap * sizeof(uint64_t));
    if (!h->len || !h->cnt) die("Out of memory");
  }
  memmove(h->len + lo + 1, h->len + lo, (h->n - lo) * sizeof(uint64_t));
  memmove(h->cnt + lo + 1, h->cnt + lo, (h->n - lo) * sizeof(uint64_t));
  h->len[lo] = len;
  h->cnt[lo] = count;
  h->n++;
}
void ctp_hist_free(ctp_hist *h) { free(h->len); free(h->cnt); memset(h, 0, sizeof(*h)); }

/* hdr["paths"]["contig_hists"][colour] added to h length by length; false when it is not there or its two lists differ
 * in length (gpath_reader_load_contig_hist dies on both) */
bool ctp_hdr_hist_add(const char *hdr, size_t n, size_t colour, ctp_hist *h)
{
  const char *pb, *pe, *ab, *ae, *ob, *oe, *lb, *le, *cb, *ce;
  if (!ctp_json_member(hdr, hdr + n, "paths", &pb, &pe) || !ctp_json_member(pb, pe, "contig_hists", &ab, &ae)) return false;
  if (!array_item(ab, ae, colour, &ob, &oe, NULL) || *ob != '{') return false;
  if (!ctp_json_member(ob, oe, "lengths", &lb, &le) || !ctp_json_member(ob, oe, "counts", &cb, &ce) || *lb != '[' || *cb != '[') return false;
  const char *lp = lb + 1, *cp = cb + 1;
  uint64_t len, cnt;
  while (true) {
    const bool a = next_number(&lp, le, &len), b = next_number(&cp, ce, &cnt);
    if (a != b) return false;
    if (!a) break;
    ctp_hist_add(h, len, cnt);
  }
  return *ws(lp, le) == ']' && *ws(cp, ce) == ']';
}

/* entry i of hdr["commands"]: its text and, when it has one, the text of its string "key" (quotes included; *kb = NULL
 * otherwise); false behind the last entry and when there is no such array */
bool ctp_hdr_command_at(const char *hdr, size_t n, size_t i, const char **b, const char **e, const char **kb, const char **ke)
{
  const char *ab, *ae;
  *kb = *ke = NULL;
  if (!ctp_json_member(hdr, hdr + n, "commands", &ab, &ae) || !array_item(ab, ae, i, b, e, NULL)) return false;
  if (**b == '{' && ctp_json_member(*b, *e, "key", kb, ke) && **kb == '"') return true;
  *kb = *ke = NULL;
  return true;
}

static void put(ctp_str *s, const char *p) { ctp_str_add(s, p, strlen(p)); }
static void put_u64(ctp_str *s, uint64_t v)
{
  char tmp[32];
  snprintf(tmp, sizeof(tmp), "%llu", (unsigned long long)v);
  put(s, tmp);
}
static bool same(const char *a, const char *ae, const char *b, const char *be) { return ae - a == be - b && !memcmp(a, b, (size_t)(ae - a)); }

/* The merged header into `out` (no newline behind it).  command: the object ctp_hdr_command wrote with no previous key
 * (it ends `"prev": []` and its closing brace); the first command key of every input goes into that list.  NULL, or
 * what is wrong, in err. */
const char *ctp_merge_header(ctp_str *out, const ctp_merge_input *in, size_t nin, size_t kmer_size, size_t out_ncols, const char *file_key, const char *command,
                             uint64_t nkmers, uint64_t npaths, uint64_t nbytes, char *err, size_t errlen)
{
  static const char undefined[] = "\"undefined\"";
  const char **nb = calloc(out_ncols, sizeof(char *)), **ne = calloc(out_ncols, sizeof(char *));
  ctp_hist *hists = calloc(out_ncols, sizeof(ctp_hist));
  if (!nb || !ne || !hists) die("Out of memory");
  const char *res = NULL;
  for (size_t c = 0; c < out_ncols; c++) { nb[c] = undefined; ne[c] = undefined + sizeof(undefined) - 1; }
  for (size_t i = 0; i < nin && !res; i++) /* gpath_reader_load_sample_names, gpath_reader_load_contig_hist */
    for (size_t j = 0; j < in[i].nfilter && !res; j++) {
      const size_t from = in[i].filter[j].from, into = in[i].filter[j].into;
      const char *b, *e;
      if (into >= out_ncols) { snprintf(err, errlen, "Colour %zu is beyond the output's %zu: %s", into, out_ncols, in[i].path); res = err; break; }
      if (!ctp_hdr_sample(in[i].hdr, in[i].len, from, &b, &e)) { snprintf(err, errlen, "Cannot find the sample name of colour %zu: %s", from, in[i].path); res = err; break; }
      if (same(nb[into], ne[into], undefined, undefined + sizeof(undefined) - 1)) { nb[into] = b; ne[into] = e; }
      else if (!same(nb[into], ne[into], b, e)) {
        snprintf(err, errlen, "Graph/path sample names do not match [%zu->%zu] %.*s vs %.*s", from, into, (int)(ne[into] - nb[into]), nb[into], (int)(e - b), b);
        res = err;
        break;
      }
      if (!ctp_hdr_hist_add(in[i].hdr, in[i].len, from, &hists[into])) { snprintf(err, errlen, "Cannot read the contig histogram of colour %zu: %s", from, in[i].path); res = err; }
    }
  if (!res) {
    put(out, "{\n  \"file_format\": \"ctp\",\n  \"format_version\": 4,\n  \"file_key\": \"");
    put(out, file_key);
    put(out, "\",\n  \"graph\": {\n    \"num_colours\": ");
    put_u64(out, out_ncols);
    put(out, ",\n    \"kmer_size\": ");
    put_u64(out, kmer_size);
    put(out, ",\n    \"num_kmers_in_graph\": ");
    put_u64(out, nkmers);
    put(out, ",\n    \"colours\": [");
    for (size_t c = 0; c < out_ncols; c++) {
      put(out, c ? ", {\n        \"colour\": " : "{\n        \"colour\": ");
      put_u64(out, c);
      put(out, ",\n        \"sample\": ");
      ctp_str_add(out, nb[c], (size_t)(ne[c] - nb[c]));
      put(out, ",\n        \"total_sequence\": 0,\n        \"cleaned_tips\": false,\n        \"cleaned_unitigs\": false\n      }");
    }
    put(out, "]\n  },\n  \"commands\": [");
    /* this command, its "prev" the first command key of every input */
    const size_t clen = strlen(command);
    const char *tail = NULL;
    for (size_t i = clen; i-- > 0 && !tail;)
      if (command[i] == '[') tail = command + i;
    if (!tail) die("ctp_merge_header: the command has no \"prev\" list");
    ctp_str_add(out, command, (size_t)(tail + 1 - command));
    bool first = true;
    for (size_t i = 0; i < nin; i++) {
      const char *b, *e, *kb, *ke;
      if (!ctp_hdr_command_at(in[i].hdr, in[i].len, 0, &b, &e, &kb, &ke) || !kb) continue;
      if (!first) put(out, ", ");
      ctp_str_add(out, kb, (size_t)(ke - kb));
      first = false;
    }
    put(out, tail + 1);
    /* the inputs' commands in input order, each key once */
    size_t nseen = 0, cap = 0;
    const char **sb = NULL, **se = NULL;
    for (size_t i = 0; i < nin; i++)
      for (size_t c = 0;; c++) {
        const char *b, *e, *kb, *ke;
        if (!ctp_hdr_command_at(in[i].hdr, in[i].len, c, &b, &e, &kb, &ke)) break;
        if (!kb) continue;
        size_t s = 0;
        while (s < nseen && !same(sb[s], se[s], kb, ke)) s++;
        if (s < nseen) continue;
        if (nseen == cap) {
          cap = cap ? cap * 2 : 16;
          sb = realloc(sb, cap * sizeof(char *));
          se = realloc(se, cap * sizeof(char *));
          if (!sb || !se) die("Out of memory");
        }
        sb[nseen] = kb; se[nseen] = ke; nseen++;
        put(out, ", ");
        ctp_str_add(out, b, (size_t)(e - b));
      }
    free(sb); free(se);
    put(out, "],\n  \"paths\": {\n    \"num_kmers_with_paths\": ");
    put_u64(out, nkmers);
    put(out, ",\n    \"num_paths\": ");
    put_u64(out, npaths);
    put(out, ",\n    \"path_bytes\": ");
    put_u64(out, nbytes);
    put(out, ",\n    \"contig_hists\": [");
    for (size_t c = 0; c < out_ncols; c++) {
      put(out, c ? ", {\n        \"lengths\": [" : "{\n        \"lengths\": [");
      for (size_t i = 0; i < hists[c].n; i++) { if (i) put(out, ", "); put_u64(out, hists[c].len[i]); }
      put(out, "],\n        \"counts\": [");
      for (size_t i = 0; i < hists[c].n; i++) { if (i) put(out, ", "); put_u64(out, hists[c].cnt[i]); }
      put(out, "]\n      }");
    }
    put(out, "]\n  }\n}");
  }
  for (size_t c = 0; c < out_ncols; c++) ctp_hist_free(&hists[c]);
  free(hists); free(nb); free(ne);
  return res;
}
