/* seq_out.c -- gzip'd FASTQ / FASTA / plain output of `reads` (src/basic/seqout.{h,c}): <O>.fq.gz, <O>.fa.gz or
 * <O>.txt.gz, and for a paired task <O>.1.* and <O>.2.* beside it.  The unpaired file is always created.
 * Records: FASTA ">name\nseq\n", FASTQ "@name\nseq\n+\nqual\n" with the qualities cut or padded with '.' to the
 * length of the sequence (a read without qualities gets all dots), plain "seq\n".  The sequence goes out as it was
 * read, case kept, on one line. */
#define _GNU_SOURCE
#include "host.h"

#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

struct seq_out {
  seq_fmt fmt;
  bool is_pe;
  char *path[3]; /* unpaired, .1, .2 */
  gzFile gz[3];
  char *qbuf;
  size_t qcap;
};

/* futil_mkpath: every directory of the path's prefix */
static void make_dirs(const char *path)
{
  char *p = strdup(path);
  if (!p) die("Out of memory");
  for (char *s = p + 1; *s; s++)
    if (*s == '/') {
      *s = '\0';
      (void)mkdir(p, 0777);
      *s = '/';
    }
  free(p);
}

static gzFile out_open(const char *path, bool force)
{
  make_dirs(path);
  const int fd = open(path, O_CREAT | O_WRONLY | (force ? O_TRUNC : O_EXCL), 0666);
  if (fd == -1) {
    if (errno == EEXIST) warn("Output file already exists: %s", path);
    else warn("Cannot create file: %s [%s]", path, strerror(errno));
    return NULL;
  }
  gzFile gz = gzdopen(fd, "w");
  if (!gz) {
    warn("Cannot open %s", path);
    close(fd);
    unlink(path);
    return NULL;
  }
  gzbuffer(gz, 1u << 20);
  return gz;
}

seq_out *seq_out_open(const char *out_base, seq_fmt fmt, bool is_pe, bool force)
{
  const char *ext = fmt == SEQ_FMT_FASTQ ? ".fq.gz" : fmt == SEQ_FMT_FASTA ? ".fa.gz" : ".txt.gz";
  if (fmt != SEQ_FMT_FASTQ && fmt != SEQ_FMT_FASTA && fmt != SEQ_FMT_PLAIN) die("Invalid format: %i", (int)fmt);
  seq_out *o = calloc(1, sizeof(*o));
  if (!o) die("Out of memory");
  o->fmt = fmt;
  o->is_pe = is_pe;
  for (int i = 0; i < (is_pe ? 3 : 1); i++) {
    o->path[i] = malloc(strlen(out_base) + strlen(ext) + 3);
    if (!o->path[i]) die("Out of memory");
    if (i) sprintf(o->path[i], "%s.%d%s", out_base, i, ext);
    else sprintf(o->path[i], "%s%s", out_base, ext);
    if (!(o->gz[i] = out_open(o->path[i], force))) {
      seq_out_close(o, true);
      return NULL;
    }
  }
  return o;
}

void seq_out_close(seq_out *o, bool rm)
{
  if (!o) return;
  for (int i = 0; i < 3; i++) {
    if (o->gz[i]) {
      if (gzclose(o->gz[i]) != Z_OK && !rm) die("Cannot write to file: %s", o->path[i]);
      if (rm && unlink(o->path[i]) != 0) warn("Cannot delete file %s", o->path[i]);
    }
    free(o->path[i]);
  }
  free(o->qbuf);
  free(o);
}

static void put(seq_out *o, int which, const void *p, size_t n)
{
  while (n) {
    const unsigned take = n > (1u << 30) ? (1u << 30) : (unsigned)n;
    if (gzwrite(o->gz[which], p, take) != (int)take) die("Cannot write sequence");
    p = (const char *)p + take;
    n -= take;
  }
}

void seq_out_print_parts(seq_out *o, int which, const char *name, size_t nlen, const char *extra, size_t elen, const uint8_t *seq, size_t n,
                         const uint8_t *qual, char fq_zero)
{
  if (o->fmt != SEQ_FMT_PLAIN) {
    put(o, which, o->fmt == SEQ_FMT_FASTQ ? "@" : ">", 1);
    put(o, which, name, nlen);
    if (extra) put(o, which, extra, elen);
    put(o, which, "\n", 1);
  }
  put(o, which, seq, n);
  put(o, which, "\n", 1);
  if (o->fmt == SEQ_FMT_FASTQ) {
    if (n + 1 > o->qcap) {
      o->qcap = (n + 1) * 2;
      o->qbuf = realloc(o->qbuf, o->qcap);
      if (!o->qbuf) die("Out of memory");
    }
    for (size_t j = 0; j < n; j++) o->qbuf[j] = qual && qual[j] ? (char)qual[j] : fq_zero;
    o->qbuf[n] = '\n';
    put(o, which, "+\n", 2);
    put(o, which, o->qbuf, n + 1);
  }
}

void seq_out_print(seq_out *o, int which, const read_batch *b, size_t i)
{
  const size_t at = (size_t)b->offsets[i], n = (size_t)(b->offsets[i + 1] - b->offsets[i]);
  const char *name = b->want_names ? b->names + b->name_off[i] : "";
  const size_t nlen = b->want_names ? (size_t)(b->name_off[i + 1] - b->name_off[i]) : 0;
  if (o->fmt != SEQ_FMT_PLAIN) {
    put(o, which, o->fmt == SEQ_FMT_FASTQ ? "@" : ">", 1);
    put(o, which, name, nlen);
    put(o, which, "\n", 1);
  }
  put(o, which, b->bases + at, n);
  put(o, which, "\n", 1);
  if (o->fmt == SEQ_FMT_FASTQ) {
    if (n + 1 > o->qcap) {
      o->qcap = (n + 1) * 2;
      o->qbuf = realloc(o->qbuf, o->qcap);
      if (!o->qbuf) die("Out of memory");
    }
    /* (the reader leaves 0 where a record had no quality for a base) */
    for (size_t j = 0; j < n; j++) o->qbuf[j] = b->quals && b->quals[at + j] ? (char)b->quals[at + j] : '.';
    o->qbuf[n] = '\n';
    put(o, which, "+\n", 2);
    put(o, which, o->qbuf, n + 1);
  }
}
