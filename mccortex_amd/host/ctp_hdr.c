/* ctp_hdr.c -- the JSON header of a .ctp file read and edited as text, and the cutter that hands the body to the
 * device in pieces of whole k-mer blocks (`links`); the two JSON helpers `thread` and `links` share.
 *
 * No JSON tree is built.  The header is one object; a value is found by walking the members of an object at depth one,
 * with strings (and their escapes) honoured, and an edit replaces the bytes of a value or inserts bytes at a place:
 * everything else of the header goes through as it came (json_hdr_add_curr_cmd of src/graph/json_hdr.c:157-181 and the
 * three totals of ctx_links.c:366-371). */
#define _GNU_SOURCE
#include "host.h"

#include <limits.h>
#include <pwd.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <sys/utsname.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

/* a JSON string with its quotes */
void ctp_put_str(gzFile gz, const char *s)
{
  gzputc(gz, '"');
  for (; *s; s++) {
    const unsigned char ch = (unsigned char)*s;
    if (ch == '"' || ch == '\\') { gzputc(gz, '\\'); gzputc(gz, ch); }
    else if (ch == '\n') gzputs(gz, "\\n");
    else if (ch == '\t') gzputs(gz, "\\t");
    else if (ch < 0x20) gzprintf(gz, "\\u%04x", ch);
    else gzputc(gz, ch);
  }
  gzputc(gz, '"');
}

/* hex_rand_str (util.c): n hex digits */
void ctp_hex_key(char *out, size_t n)
{
  static bool seeded = false;
  if (!seeded) {
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    srandom((unsigned)ts.tv_nsec ^ (unsigned)ts.tv_sec ^ ((unsigned)getpid() << 11));
    seeded = true;
  }
  for (size_t i = 0; i < n; i++) out[i] = "0123456789abcdef"[random() & 15];
  out[n] = '\0';
}

/* ---- a growing string ---- */
void ctp_str_add(ctp_str *s, const char *p, size_t n)
{
  if (s->len + n + 1 > s->cap) {
    s->cap = (s->len + n + 1) * 2;
    s->b = realloc(s->b, s->cap);
    if (!s->b) die("Out of memory");
  }
  memcpy(s->b + s->len, p, n);
  s->len += n;
  s->b[s->len] = '\0';
}
static void str_puts(ctp_str *s, const char *p) { ctp_str_add(s, p, strlen(p)); }
static void str_json(ctp_str *s, const char *p)
{
  char tmp[8];
  str_puts(s, "\"");
  for (; *p; p++) {
    const unsigned char ch = (unsigned char)*p;
    if (ch == '"' || ch == '\\') { tmp[0] = '\\'; tmp[1] = (char)ch; ctp_str_add(s, tmp, 2); }
    else if (ch == '\n') str_puts(s, "\\n");
    else if (ch == '\t') str_puts(s, "\\t");
    else if (ch < 0x20) { snprintf(tmp, sizeof(tmp), "\\u%04x", ch); str_puts(s, tmp); }
    else ctp_str_add(s, p, 1);
  }
  str_puts(s, "\"");
}

/* ---- reading ---- */
static const char *skip_ws(const char *p, const char *e)
{
  while (p < e && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
  return p;
}
/* p at the opening quote -> behind the closing one, or NULL */
static const char *skip_string(const char *p, const char *e)
{
  for (p++; p < e; p++) {
    if (*p == '\\') p++;
    else if (*p == '"') return p + 1;
  }
  return NULL;
}
/* p at the first byte of a value -> behind its last, or NULL when it does not end before e */
static const char *skip_value(const char *p, const char *e)
{
  if (p >= e) return NULL;
  if (*p == '"') return skip_string(p, e);
  if (*p == '{' || *p == '[') {
    size_t depth = 0;
    while (p < e) {
      if (*p == '"') { if (!(p = skip_string(p, e))) return NULL; continue; }
      if (*p == '{' || *p == '[') depth++;
      else if (*p == '}' || *p == ']') { if (--depth == 0) return p + 1; }
      p++;
    }
    return NULL;
  }
  const char *q = p;
  while (q < e && *q != ',' && *q != '}' && *q != ']' && *q != ' ' && *q != '\t' && *q != '\n' && *q != '\r') q++;
  return q > p ? q : NULL;
}

/* Bytes of the object that `buf` begins with (white space before it allowed): 0 while it has not ended within n
 * bytes, (size_t)-1 when the text does not begin with an object. */
size_t ctp_hdr_span(const char *buf, size_t n)
{
  const char *e = buf + n, *p = skip_ws(buf, e);
  if (p == e) return 0;
  if (*p != '{') return (size_t)-1;
  const char *q = skip_value(p, e);
  return q ? (size_t)(q - buf) : 0;
}

/* the value of member `key` of the object [obj, obj_end) (obj at its '{'): its bytes, or false */
bool ctp_json_member(const char *obj, const char *obj_end, const char *key, const char **vbeg, const char **vend)
{
  const char *p = skip_ws(obj, obj_end);
  if (p >= obj_end || *p != '{') return false;
  p++;
  const size_t klen = strlen(key);
  while (true) {
    p = skip_ws(p, obj_end);
    if (p >= obj_end || *p != '"') return false; /* '}' or broken */
    const char *ke = skip_string(p, obj_end);
    if (!ke) return false;
    const bool hit = (size_t)(ke - p) == klen + 2 && !memcmp(p + 1, key, klen);
    p = skip_ws(ke, obj_end);
    if (p >= obj_end || *p != ':') return false;
    p = skip_ws(p + 1, obj_end);
    const char *ve = skip_value(p, obj_end);
    if (!ve) return false;
    if (hit) { *vbeg = p; *vend = ve; return true; }
    p = skip_ws(ve, obj_end);
    if (p < obj_end && *p == ',') p++;
    else return false;
  }
}

/* hdr[k1] or hdr[k1][k2] (k2 may be NULL) as a non-negative integer */
bool ctp_hdr_number(const char *hdr, size_t n, const char *k1, const char *k2, uint64_t *out)
{
  const char *b, *e;
  if (!ctp_json_member(hdr, hdr + n, k1, &b, &e)) return false;
  if (k2 && !ctp_json_member(b, e, k2, &b, &e)) return false;
  if (b == e || *b < '0' || *b > '9') return false;
  uint64_t v = 0;
  for (; b < e && *b >= '0' && *b <= '9'; b++) v = v * 10 + (uint64_t)(*b - '0');
  *out = v;
  return true;
}

/* ---- editing ---- */
typedef struct { size_t at, len; const char *text; } splice;
static int splice_cmp(const void *a, const void *b)
{
  const splice *x = a, *y = b;
  return x->at < y->at ? -1 : x->at > y->at;
}

/* json_hdr_new_command: the object of this command; prev_key NULL: "prev" is empty */
void ctp_hdr_command(ctp_str *s, const char *cmd_key, int argc, char **argv, const char *out_path, const char *file_key, const char *prev_key)
{
  char cwd[PATH_MAX + 1], abspath[PATH_MAX + 1], date[50], user[1025] = "noname";
  if (!getcwd(cwd, sizeof(cwd))) strcpy(cwd, ".");
  if (!realpath(out_path, abspath)) snprintf(abspath, sizeof(abspath), "%s", out_path);
  const time_t now = time(NULL);
  strftime(date, sizeof(date), "%Y-%m-%d %H:%M:%S", localtime(&now));
  str_puts(s, "{\n      \"key\": ");
  str_json(s, cmd_key);
  str_puts(s, ",\n      \"cmd\": [");
  str_json(s, CMD_NAME);
  for (int i = 0; i < argc; i++) { str_puts(s, ", "); str_json(s, argv[i]); }
  str_puts(s, "],\n      \"cwd\": ");
  str_json(s, cwd);
  str_puts(s, ",\n      \"out_path\": ");
  str_json(s, abspath);
  str_puts(s, ",\n      \"out_key\": ");
  str_json(s, file_key);
  str_puts(s, ",\n      \"date\": ");
  str_json(s, date);
  str_puts(s, ",\n      \"mccortex\": \"" CMD_NAME " on libmcxgpu\",\n      \"zlib\": ");
  str_json(s, zlibVersion());
  struct passwd pwd, *res = NULL;
  char pwbuf[4096];
  if (getpwuid_r(geteuid(), &pwd, pwbuf, sizeof(pwbuf), &res) == 0 && res) snprintf(user, sizeof(user), "%s", res->pw_name);
  str_puts(s, ",\n      \"user\": ");
  str_json(s, user);
  struct utsname sys;
  if (uname(&sys) != -1) {
    const char *const names[5] = {"host", "os", "osrelease", "osversion", "hardware"};
    const char *const vals[5] = {sys.nodename, sys.sysname, sys.release, sys.version, sys.machine};
    for (int i = 0; i < 5; i++) { str_puts(s, ",\n      \""); str_puts(s, names[i]); str_puts(s, "\": "); str_json(s, vals[i]); }
  }
  str_puts(s, ",\n      \"prev\": [");
  if (prev_key) str_json(s, prev_key);
  str_puts(s, "]\n    }");
}

/* The key of the first entry of hdr["commands"] into key[keylen] (unescaped as far as a hex key needs: copied as it
 * stands); false when the array is empty or the entry has no string "key". */
bool ctp_hdr_first_command_key(const char *hdr, size_t n, char *key, size_t keylen)
{
  const char *b, *e, *kb, *ke;
  if (!ctp_json_member(hdr, hdr + n, "commands", &b, &e) || *b != '[') return false;
  const char *p = skip_ws(b + 1, e);
  if (p >= e || *p != '{') return false;
  const char *oe = skip_value(p, e);
  if (!oe || !ctp_json_member(p, oe, "key", &kb, &ke) || *kb != '"') return false;
  const size_t len = (size_t)(ke - kb) - 2;
  if (len + 1 > keylen) return false;
  memcpy(key, kb + 1, len);
  key[len] = '\0';
  return true;
}

/* The header with a new file_key, `command` (the text of an object) as the new first entry of "commands" and the three
 * totals of "paths" replaced.  NULL, with *why set, when one of these is not there. */
char *ctp_hdr_edit(const char *hdr, size_t n, const char *file_key, const char *command, uint64_t nkmers, uint64_t npaths, uint64_t nbytes,
                   size_t *out_len, const char **why)
{
  const char *b, *e, *pb, *pe;
  splice sp[5];
  char num[3][32], fk[64];
  ctp_str ins = {NULL, 0, 0};
  if (!ctp_json_member(hdr, hdr + n, "file_key", &b, &e) || *b != '"') { *why = "file_key"; return NULL; }
  snprintf(fk, sizeof(fk), "\"%s\"", file_key);
  sp[0] = (splice){(size_t)(b - hdr), (size_t)(e - b), fk};
  if (!ctp_json_member(hdr, hdr + n, "commands", &b, &e) || *b != '[') { *why = "commands"; return NULL; }
  const bool empty = *skip_ws(b + 1, e) == ']';
  str_puts(&ins, command);
  if (!empty) str_puts(&ins, ", ");
  sp[1] = (splice){(size_t)(b + 1 - hdr), 0, ins.b};
  if (!ctp_json_member(hdr, hdr + n, "paths", &pb, &pe) || *pb != '{') { free(ins.b); *why = "paths"; return NULL; }
  const char *const names[3] = {"num_kmers_with_paths", "num_paths", "path_bytes"};
  const uint64_t vals[3] = {nkmers, npaths, nbytes};
  for (int i = 0; i < 3; i++) {
    if (!ctp_json_member(pb, pe, names[i], &b, &e) || *b < '0' || *b > '9') { free(ins.b); *why = names[i]; return NULL; }
    snprintf(num[i], sizeof(num[i]), "%llu", (unsigned long long)vals[i]);
    sp[2 + i] = (splice){(size_t)(b - hdr), (size_t)(e - b), num[i]};
  }
  qsort(sp, 5, sizeof(sp[0]), splice_cmp);
  ctp_str out = {NULL, 0, 0};
  size_t at = 0;
  for (int i = 0; i < 5; i++) {
    ctp_str_add(&out, hdr + at, sp[i].at - at);
    str_puts(&out, sp[i].text);
    at = sp[i].at + sp[i].len;
  }
  ctp_str_add(&out, hdr + at, n - at);
  free(ins.b);
  *out_len = out.len;
  return out.b;
}

/* ---- the body in pieces ---- */
/* Where the piece buf[0, n) ends: the last line start behind byte 0 whose first byte is one of ACGT (a k-mer line:
 * everything before it is whole blocks), or 0 when there is none (one block fills the buffer). */
size_t ctp_cut(const char *buf, size_t n)
{
  for (size_t i = n; i-- > 1;)
    if (buf[i - 1] == '\n' && (buf[i] == 'A' || buf[i] == 'C' || buf[i] == 'G' || buf[i] == 'T')) return i;
  return 0;
}

void ctp_pieces_init(ctp_pieces *p, char *buf, size_t cap, ctp_read_fn rd, void *rd_ctx, ctp_grow_fn grow, void *grow_ctx)
{
  memset(p, 0, sizeof(*p));
  p->buf = buf; p->cap = cap; p->rd = rd; p->rd_ctx = rd_ctx; p->grow = grow; p->grow_ctx = grow_ctx;
}

/* twice the buffer: `grow` hands out a new one and takes the old one back, so what is held goes through a copy */
static void pieces_grow(ctp_pieces *p)
{
  char *keep = malloc(p->fill + 1);
  if (!keep) die("Out of memory");
  memcpy(keep, p->buf, p->fill);
  p->buf = p->grow(p->grow_ctx, p->cap * 2);
  p->cap *= 2;
  memcpy(p->buf, keep, p->fill);
  free(keep);
}

/* bytes the reader has seen already (behind the header) go in first */
void ctp_pieces_preload(ctp_pieces *p, const char *data, size_t n)
{
  while (p->fill + n + 1 > p->cap) pieces_grow(p);
  memcpy(p->buf + p->fill, data, n);
  p->fill += n;
}

/* The next piece: buf[0, return) is a run of whole k-mer blocks that ends behind a newline (one is added to a file
 * that ends without); 0 at the end of the input, -1 when reading failed.  The buffer is doubled through `grow` (which
 * hands out a new buffer and takes the old one back) while one block does not fit. */
long long ctp_pieces_next(ctp_pieces *p)
{
  if (p->taken) { /* the tail behind the last piece moves to the front */
    memmove(p->buf, p->buf + p->taken, p->fill - p->taken);
    p->fill -= p->taken;
    p->taken = 0;
  }
  while (true) {
    while (!p->eof && p->fill + 1 < p->cap) {
      const size_t room = p->cap - 1 - p->fill;
      const int got = p->rd(p->rd_ctx, p->buf + p->fill, room > (1u << 30) ? (1u << 30) : (unsigned)room);
      if (got < 0) return -1;
      if (got == 0) p->eof = true;
      p->fill += (size_t)got;
    }
    if (p->eof) {
      if (!p->fill) return 0;
      if (p->buf[p->fill - 1] != '\n') p->buf[p->fill++] = '\n'; /* (one byte of the buffer is kept for it) */
      p->taken = p->fill;
      return (long long)p->taken;
    }
    const size_t cut = ctp_cut(p->buf, p->fill);
    if (cut) { p->taken = cut; return (long long)cut; }
    pieces_grow(p);
  }
}
