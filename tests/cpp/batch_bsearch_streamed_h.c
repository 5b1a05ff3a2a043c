/* include/ellhip_batch_bsearch_streamed.h as a C99 translation unit (tests/test_batch_bsearch_streamed_cpu.py: -std=c99
 * -pedantic -Werror) */
#include "ellhip_batch_bsearch_streamed.h"

int main(void) {
    ellhip_batch_linfeas *o = 0;
    int (*search)(ellhip_batch *, ellhip_batch_linfeas *, const double *, const double *, int64_t, double, int64_t, double,
                  int32_t *, int64_t *, double *, int64_t *, int64_t *) = ellhip_batch_linfeas_bsearch_streamed;
    int (*feas)(ellhip_batch *, ellhip_batch_linfeas *, int64_t, double, double *, int32_t *, int64_t *, int32_t *) =
        ellhip_batch_linfeas_feas_streamed;
    int (*create)(ellhip_batch_linfeas **, int64_t, int64_t, int64_t, const double *, const double *, int32_t, int) =
        ellhip_batch_linfeas_create_streamed;
    ellhip_batch_linfeas_destroy(o);
    return search == ellhip_batch_linfeas_bsearch_streamed_stable || feas == ellhip_batch_linfeas_feas_streamed_stable ||
           create == ellhip_batch_linfeas_create || ELLHIP_BATCH_LINFEAS_STREAMED_JMAX < ELLHIP_BATCH_STREAMED_NMAX;
}
