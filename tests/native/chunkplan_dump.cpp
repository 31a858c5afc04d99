// chunk_plan of csrc/copypool.h as text: one "bytes slot head tail tiny_tail" tuple per input line, one line of chunk sizes per tuple.
// tests/test_hostio_cases.py feeds it the tuples of tests/hostio_cases.py and compares the plans with the Python restatement there.
#include <cstdio>
#include <vector>

#include "../../tiny-ram-halo2_amd/csrc/copypool.h"

int main() {
    unsigned long long bytes, slot, tiny;
    int head, tail;
    std::vector<size_t> plan;
    while (std::scanf("%llu %llu %d %d %llu", &bytes, &slot, &head, &tail, &tiny) == 5) {
        trh::chunk_plan((size_t)bytes, (size_t)slot, head != 0, tail != 0, plan, (size_t)tiny);
        std::printf("plan");
        for (size_t cur : plan) std::printf(" %zu", cur);
        std::printf("\n");
    }
    return 0;
}
