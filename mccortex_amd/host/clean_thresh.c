/* clean_thresh.c -- cleaning_pick_kmer_threshold (src/tools/clean_graph.c): pick the unitig cleaning threshold
 * from the k-mer coverage histogram, in double precision with libm, in the reference's order of operations.
 * On its own so that the tests can call it (libmcxhost.so). */
#include "host.h"

#include <float.h>
#include <stdlib.h>
#include <math.h>

/* first coverage where errors make up <= fdr of the k-mers; -1 if none */
static int cutoff_fdr(const double *e_covg, const uint64_t *kmer_covg, size_t arrlen, double fdr)
{
  for (size_t i = 1; i < arrlen; i++)
    if (e_covg[i] / kmer_covg[i] <= fdr) return (int)i;
  return -1;
}

/* first cutoff where false positives < false negatives */
static int cutoff_fp_lt_fn(const double *e_covg, double e_total, const uint64_t *kmer_covg, uint64_t d_total, size_t arrlen)
{
  double e_rem = e_total, d_rem = d_total, e_sum = 0, d_sum = 0;
  for (size_t i = 1; i < arrlen; i++) {
    e_sum += e_covg[i];
    d_sum += kmer_covg[i];
    e_rem -= e_covg[i];
    d_rem -= kmer_covg[i];
    if (1 - e_sum / d_sum > e_rem / d_rem) return (int)i;
  }
  return -1;
}

static int cutoff_loss_vs_error(const double *e_covg, double e_total, const uint64_t *kmer_covg, size_t arrlen)
{
  double e_rem = e_total, e_sum = 0, d_sum = 0;
  for (size_t i = 1; i < arrlen; i++) {
    e_sum += e_covg[i];
    d_sum += kmer_covg[i];
    e_rem -= e_covg[i];
    if (d_sum - e_sum > e_rem) return (int)i;
  }
  return -1;
}

static void cutoff_fp_fn(const double *e_covg, double e_total, const uint64_t *kmer_covg, uint64_t d_total, size_t cutoff,
                         double *fp, double *fn)
{
  double e_rem = e_total, d_rem = d_total, e_sum = 0, d_sum = 0;
  for (size_t i = 1; i < cutoff; i++) {
    e_sum += e_covg[i];
    d_sum += kmer_covg[i];
    e_rem -= e_covg[i];
    d_rem -= kmer_covg[i];
  }
  *fp = 1 - e_sum / d_sum;
  *fn = e_rem / d_rem;
}

/* at least frac_covg_kept of the coverage is kept */
static bool cutoff_good(const uint64_t *kmer_covg, size_t arrlen, size_t cutoff, double frac_covg_kept)
{
  uint64_t below = 0, above = 0;
  for (size_t i = 0; i < cutoff; i++) below += kmer_covg[i] * i;
  for (size_t i = cutoff; i < arrlen; i++) above += kmer_covg[i] * i;
  return !arrlen || ((double)above / (below + above) >= frac_covg_kept);
}

int cleaning_pick_kmer_threshold(const uint64_t *kmer_covg, size_t arrlen, double *alpha_est, double *beta_est,
                                 double *false_pos, double *false_neg)
{
  if (arrlen < 10) return -1;
  size_t min_idx = 0;
  double min_a = DBL_MAX;
  const double r1 = (double)kmer_covg[2] / kmer_covg[1];
  const double r2 = (double)kmer_covg[3] / kmer_covg[2];
  const double rr = r2 / r1;
  for (size_t i = 1; i <= 200; i++) { /* aa = 0.01 .. 2.00: the one whose faa is closest to rr */
    const double aa = i * 0.01;
    const double faa = tgamma(aa) * tgamma(aa + 2) / (2 * pow(tgamma(aa + 1), 2));
    const double t = fabs(faa - rr);
    if (t < min_a) { min_a = t; min_idx = i; }
  }
  const double a_est = min_idx * 0.01;
  double b_est = tgamma(a_est + 1.0) / (r1 * tgamma(a_est)) - 1.0;
  b_est = b_est > 1 ? b_est : 1; /* MAX2(b_est, 1) */
  const double c0 = kmer_covg[1] * pow(b_est / (1 + b_est), -a_est);
  if (alpha_est) *alpha_est = a_est;
  if (beta_est) *beta_est = b_est;

  double *e_covg = malloc(arrlen * sizeof(double));
  if (!e_covg) die("Out of memory");
  double e_total = 0;
  uint64_t d_total = 0;
  const double log_b = log(b_est), log_1b = log(1 + b_est), lgamma_a = lgamma(a_est);
  e_covg[0] = 0;
  for (size_t i = 1; i < arrlen; i++) {
    const double t = a_est * log_b - lgamma_a - lgamma(i) + lgamma(a_est + i - 1) - (a_est + i - 1) * log_1b;
    e_covg[i] = exp(t) * c0;
    e_total += e_covg[i];
    d_total += kmer_covg[i];
  }
  int cutoff = cutoff_fdr(e_covg, kmer_covg, arrlen, 0.001);
  if (cutoff < 0) cutoff = cutoff_fp_lt_fn(e_covg, e_total, kmer_covg, d_total, arrlen);
  if (cutoff < 0) cutoff = cutoff_loss_vs_error(e_covg, e_total, kmer_covg, arrlen);
  if (cutoff >= 0 && !cutoff_good(kmer_covg, arrlen, (size_t)cutoff, 0.2)) cutoff = -1;
  if (cutoff >= 0 && (false_pos || false_neg)) {
    double fp = 0, fn = 0;
    cutoff_fp_fn(e_covg, e_total, kmer_covg, d_total, (size_t)cutoff, &fp, &fn);
    if (false_pos) *false_pos = fp;
    if (false_neg) *false_neg = fn;
  }
  free(e_covg);
  return cutoff;
}
