/* conf_table.c -- the contig confidence table of `contigs` (src/graph/contig_confidence.c) for one colour, computed on
 * the host exactly as the reference computes it: calc_confid with its three exponentials in long double (expl), the
 * update of _update_table_with_length_count with its read of the old value and its loop bounds, and the %.5f table of
 * conf_table_print.  Stands alone (tests/conf_table_check.c calls it). */
#include "conf_table.h"

#include <math.h>
#include <stdlib.h>

/* calc_confid (contig_confidence.c:17-27) */
static double calc_confid(double bp_covg_depth, size_t read_length_bp, size_t kmer_size)
{
  double lambda = bp_covg_depth / read_length_bp;
  double read_kmers = read_length_bp - kmer_size + 1;
  double power = (1.0 - expl(-lambda * read_kmers)) * expl(-lambda * expl(-lambda * read_kmers));
  return power;
}

void conf_table_init(conf_table *t)
{
  t->b = NULL;
  t->len = 0;
}

void conf_table_free(conf_table *t)
{
  free(t->b);
  conf_table_init(t);
}

/* conf_table_capacity: entries up to max_read, the new ones 0.0; false when memory runs out */
static bool conf_table_capacity(conf_table *t, size_t max_read)
{
  if (max_read + 1 <= t->len) return true;
  double *b = realloc(t->b, (max_read + 1) * sizeof(double));
  if (!b) return false;
  for (size_t i = t->len; i <= max_read; i++) b[i] = 0.0;
  t->b = b;
  t->len = max_read + 1;
  return true;
}

/* conf_table_update_hist (contig_confidence.c:29-64): contig_hist[i] contigs of length i */
bool conf_table_update_hist(conf_table *t, size_t genome_size, const size_t *contig_hist, size_t hist_len)
{
  for (size_t len = 1; len < hist_len; len++) {
    const size_t num = contig_hist[len];
    if (!num) continue;
    if (!conf_table_capacity(t, len)) return false;
    for (size_t i = 1; i <= len; i++) {
      double covg = (double)(len * num) / genome_size;
      double old_conf = t->b[i];
      double new_conf = 1.0 - ((1.0 - old_conf) * (1.0 - calc_confid(covg, len, i)));
      t->b[i] = new_conf;
    }
  }
  return true;
}

/* conf_table_print for one colour */
void conf_table_print(const conf_table *t, FILE *fh)
{
  fprintf(fh, "gap_dist\tconfidence_0\n");
  for (size_t i = 1; i < t->len; i++) fprintf(fh, "%zu\t%.5f\n", i, t->b[i]);
}
