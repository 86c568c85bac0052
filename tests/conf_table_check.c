/* conf_table_check.c -- stand-alone program over mccortex_amd/host/conf_table.c: reads histograms from its arguments,
 * `<genome size> <len>:<count>,<len>:<count>,...` (or `-` for an empty histogram) per pair of arguments, and prints the
 * %.5f table of each, a line `==` between them. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "conf_table.h"

int main(int argc, char **argv)
{
  for (int a = 1; a + 1 < argc; a += 2) {
    const size_t genome = strtoull(argv[a], NULL, 10);
    size_t hist_len = 1, *hist = calloc(1, sizeof(size_t));
    if (!hist) return 2;
    for (const char *p = argv[a + 1]; *p && strcmp(argv[a + 1], "-");) {
      char *end;
      const size_t len = strtoull(p, &end, 10);
      if (*end != ':') return 3;
      const size_t cnt = strtoull(end + 1, &end, 10);
      if (len + 1 > hist_len) {
        hist = realloc(hist, (len + 1) * sizeof(size_t));
        if (!hist) return 2;
        memset(hist + hist_len, 0, (len + 1 - hist_len) * sizeof(size_t));
        hist_len = len + 1;
      }
      hist[len] += cnt;
      p = *end == ',' ? end + 1 : end;
      if (*end && *end != ',') return 3;
    }
    conf_table t;
    conf_table_init(&t);
    if (!conf_table_update_hist(&t, genome, hist, hist_len)) return 2;
    conf_table_print(&t, stdout);
    puts("==");
    conf_table_free(&t);
    free(hist);
  }
  return 0;
}
