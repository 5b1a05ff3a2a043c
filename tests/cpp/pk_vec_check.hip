// pk_vec_check.hip -- host-only (built with hipcc by tests/test_ext_reference_cpu.py, runs without a GPU): prints pk_vec(t, slot)
// of csrc/ell_kernels.hpp -- the vector that sits at slot `slot` of the 16-wide column tile t in the packed operand layout
// (k_pack_operands) -- for the 32 (t, slot) pairs, one JSON line.  The test holds it to the slot formula of the header.
#include <cstdio>

#include "../../ellalgo-rs_amd/csrc/ell_kernels.hpp"

int main() {
    printf("{\"pk_vec\": [");
    for (int t = 0; t < 2; ++t)
        for (int slot = 0; slot < 16; ++slot) printf("%s%d", (t || slot) ? ", " : "", ellhip::pk_vec(t, slot));
    printf("]}\n");
    return 0;
}
