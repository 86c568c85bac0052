/* conf_table.h -- the contig confidence table of `contigs` (conf_table.c) */
#ifndef MCX_CONF_TABLE_H_
#define MCX_CONF_TABLE_H_

#include <stdbool.h>
#include <stddef.h>
#include <stdio.h>

typedef struct { double *b; size_t len; } conf_table; /* b[gap distance], b[0] unused */
void conf_table_init(conf_table *t);
void conf_table_free(conf_table *t);
bool conf_table_update_hist(conf_table *t, size_t genome_size, const size_t *contig_hist, size_t hist_len);
void conf_table_print(const conf_table *t, FILE *fh);

#endif
