/* include/ellhip_batch_bsearch.h as a C99 translation unit (tests/test_batch_bsearch_cpu.py: -std=c99 -pedantic -Werror) */
#include "ellhip_batch_bsearch.h"

int main(void) {
    ellhip_batch_linfeas *o = 0;
    int (*search)(ellhip_batch *, ellhip_batch_linfeas *, const double *, const double *, int64_t, double, int64_t, double,
                  int32_t *, int64_t *, double *, int64_t *, int64_t *) = ellhip_batch_linfeas_bsearch;
    ellhip_batch_linfeas_destroy(o);
    return search == ellhip_batch_linfeas_bsearch_stable;
}
