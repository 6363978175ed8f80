// Stand-alone host program over the host part of mdrp_amd/csrc/mdrp_prosac.h (tests/test_prosac_host.py): prints, for each "n max_prosac count" line
// on stdin, the growth table and the subset size of every sample, complete and as the device's truncated table.
//   growth <n entries>
//   subset <min(count, progressive samples) entries>
//   truncated <entries up to the first sample whose subset is n>
#include "../../mdrp_amd/csrc/mdrp_prosac.h"

#include <cstdio>

int main() {
    unsigned long long n, m, count;
    while (scanf("%llu %llu %llu", &n, &m, &count) == 3) {
        const auto g = mdrp::prosac::growth_table(n, m);
        printf("growth");
        for (auto v : g) printf(" %llu", (unsigned long long)v);
        printf("\nsubset");
        for (auto v : mdrp::prosac::subset_schedule(n, m, count, false)) printf(" %u", v);
        printf("\ntruncated");
        for (auto v : mdrp::prosac::subset_schedule(n, m, count, true)) printf(" %u", v);
        printf("\nprogressive %llu\n", (unsigned long long)mdrp::prosac::prosac_samples(m));
    }
    return 0;
}
