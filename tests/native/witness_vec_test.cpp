// csrc/witness.h on the host, compiled with -fsanitize=address,undefined (Makefile): reads cases from stdin, one per line, and prints
// what the header's functions return; tests/test_witness_host.py compares the lines with Python integers.  Never loads libtrh.
//   u <field> <u64>      fe_from_u64: the four u64 Montgomery words, hex
//   i <field> <i64>      fe_from_i64: the same
//   e <u64>              even_part and odd_part, hex
//   s <u32>              spread_bits, hex
// field: 0 = Fp, 1 = Fq; integers are decimal.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../tiny-ram-halo2_amd/csrc/witness.h"

using namespace trh;

template <class F> static void print_fe(const Fe<F>& v) {
    u32 w[8];
    fe_store(v, w);
    for (int k = 0; k < 4; ++k) printf("%s%016" PRIx64, k ? " " : "", (u64)w[2 * k] | (u64)w[2 * k + 1] << 32);
    printf("\n");
}

int main() {
    char line[128];
    while (fgets(line, sizeof line, stdin)) {
        char op = 0;
        int field = 0;
        unsigned long long uv = 0;
        long long iv = 0;
        if (sscanf(line, " u %d %llu", &field, &uv) == 2) {
            if (field == 0) print_fe(fe_from_u64<FpParams>((u64)uv)); else print_fe(fe_from_u64<FqParams>((u64)uv));
        } else if (sscanf(line, " i %d %lld", &field, &iv) == 2) {
            if (field == 0) print_fe(fe_from_i64<FpParams>((i64)iv)); else print_fe(fe_from_i64<FqParams>((i64)iv));
        } else if (sscanf(line, " e %llu", &uv) == 1) {
            printf("%016" PRIx64 " %016" PRIx64 "\n", even_part((u64)uv), odd_part((u64)uv));
        } else if (sscanf(line, " s %llu", &uv) == 1) {
            printf("%016" PRIx64 "\n", spread_bits((u32)uv));
        } else if (sscanf(line, " %c", &op) == 1) {
            fprintf(stderr, "witness_vec_test: bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
