// ell_math_host.cpp -- csrc/ell_math.hpp compiled by plain g++ (-ffp-contract=off): `ell_math_host exp|log` reads raw
// little-endian doubles from stdin and writes ell_exp / ell_log of each to stdout, so that tests/test_batch_profit_cpu.py can
// compare the header bit for bit with its Python restatement and tests/test_gpu_batch_profit.py with the device.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ellalgo-rs_amd/csrc/ell_math.hpp"

int main(int argc, char** argv) {
    if (argc != 2 || (strcmp(argv[1], "exp") != 0 && strcmp(argv[1], "log") != 0)) {
        fprintf(stderr, "usage: ell_math_host exp|log < doubles > doubles\n");
        return 2;
    }
    const bool is_exp = strcmp(argv[1], "exp") == 0;
    std::vector<double> buf(1 << 16);
    size_t got;
    while ((got = fread(buf.data(), sizeof(double), buf.size(), stdin)) > 0) {
        for (size_t j = 0; j < got; ++j) buf[j] = is_exp ? ellhip::ell_exp(buf[j]) : ellhip::ell_log(buf[j]);
        if (fwrite(buf.data(), sizeof(double), got, stdout) != got) return 1;
    }
    return 0;
}
