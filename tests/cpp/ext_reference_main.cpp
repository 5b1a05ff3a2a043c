// ext_reference_main.cpp -- CPU driver of tests/cpp/ext_reference.hpp for tests/test_ext_reference_cpu.py (g++, -ffp-contract=off).
// Arrays travel as raw little-endian doubles in files (numpy tofile / fromfile), results as raw doubles or one JSON line:
//   symm      n ld row0 nrows lv IN OUT      IN = Q[nrows][ld], g[lv][n]                   OUT = y.hi, y.lo, S        ([lv][n] each)
//   apply     n ld row0 nrows np IN OUT      IN = Q[nrows][ld], pend[np][n], cpend[np]     OUT = X.hi, X.lo, M ([nrows][n] each),
//                                                                                          two-roundings, fused chain ([nrows][ld] each)
//   cmp_symm  n ld row0 nrows lv nstrips nsegs IN     IN = Q, g, yhat[lv][n]               -> {"ratio": .., "index": ..}
//   cmp_apply n ld row0 nrows np IN                   IN = Q, pend, cpend, Qhat[nrows][ld] -> {"ratio": .., "index": ..}
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ext_reference.hpp"
using namespace extref;

static std::vector<double> slurp(const char* path, size_t want) {
    std::vector<double> v(want);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), 8, want, f) != want || fgetc(f) != EOF) {
        fprintf(stderr, "%s: expected exactly %zu doubles\n", path, want);
        exit(2);
    }
    fclose(f);
    return v;
}

static void put(FILE* f, const std::vector<double>& v) {
    if (fwrite(v.data(), 8, v.size(), f) != v.size()) exit(2);
}

static void print_worst(const Worst& w) {
    if (std::isinf(w.ratio)) printf("{\"ratio\": Infinity, \"index\": %lld}\n", w.index);
    else printf("{\"ratio\": %.17g, \"index\": %lld}\n", w.ratio, w.index);
}

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const std::string mode = argv[1];
    const long long n = atoll(argv[2]), ld = atoll(argv[3]), row0 = atoll(argv[4]), nrows = atoll(argv[5]);
    const int k = atoi(argv[6]);  // lv or np
    const size_t qn = (size_t)nrows * ld;
    if (mode == "symm" && argc == 9) {
        const auto in = slurp(argv[7], qn + (size_t)k * n);
        const SymmRef r = ref_symm(in.data(), ld, n, row0, nrows, in.data() + qn, n, k);
        std::vector<double> hi(r.y.size()), lo(r.y.size());
        for (size_t i = 0; i < r.y.size(); ++i) hi[i] = r.y[i].hi, lo[i] = r.y[i].lo;
        FILE* f = fopen(argv[8], "wb");
        if (!f) return 2;
        put(f, hi), put(f, lo), put(f, r.S);
        return fclose(f) ? 2 : 0;
    }
    if (mode == "apply" && argc == 9) {
        const auto in = slurp(argv[7], qn + (size_t)k * n + k);
        const double *Q = in.data(), *pend = Q + qn, *cpend = pend + (size_t)k * n;
        const ApplyRef r = ref_apply(Q, ld, pend, cpend, k, n, row0, nrows);
        std::vector<double> hi(r.X.size()), lo(r.X.size());
        for (size_t i = 0; i < r.X.size(); ++i) hi[i] = r.X[i].hi, lo[i] = r.X[i].lo;
        FILE* f = fopen(argv[8], "wb");
        if (!f) return 2;
        put(f, hi), put(f, lo), put(f, r.M);
        put(f, ref_apply_two_roundings(Q, ld, pend, cpend, k, n, row0, nrows));
        put(f, ref_apply_fused_chain(Q, ld, pend, cpend, k, n, row0, nrows));
        return fclose(f) ? 2 : 0;
    }
    if (mode == "cmp_symm" && argc == 10) {
        const long long nstrips = atoll(argv[7]), nsegs = atoll(argv[8]);
        const auto in = slurp(argv[9], qn + 2 * (size_t)k * n);
        const SymmRef r = ref_symm(in.data(), ld, n, row0, nrows, in.data() + qn, n, k);
        print_worst(cmp_products(in.data() + qn + (size_t)k * n, r.y.data(), r.S.data(), (long long)k * n, products_K(n, nstrips, nsegs)));
        return 0;
    }
    if (mode == "cmp_apply" && argc == 8) {
        const auto in = slurp(argv[7], 2 * qn + (size_t)k * n + k);
        const double *Q = in.data(), *pend = Q + qn, *cpend = pend + (size_t)k * n, *Qhat = cpend + k;
        print_worst(cmp_apply(Qhat, ld, ref_apply(Q, ld, pend, cpend, k, n, row0, nrows), k));
        return 0;
    }
    return 2;
}
