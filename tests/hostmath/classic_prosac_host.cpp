// Stand-alone host program over the host part of mdrp_amd/csrc/mdrp_prosac.h with the sample size as a parameter (tests/test_classic_prosac_host.py):
// prints, for each "n sample_size max_prosac count" line on stdin, the growth table and the subset size of every sample, complete and as the
// device's truncated table.
//   growth <max(n, sample_size) entries>
//   subset <min(count, progressive samples) entries>
//   truncated <entries up to the first sample whose subset is n>
#include "../../mdrp_amd/csrc/mdrp_prosac.h"

#include <cstdio>

int main() {
    unsigned long long n, m, count;
    int ssz;
    while (scanf("%llu %d %llu %llu", &n, &ssz, &m, &count) == 4) {
        printf("growth");
        for (auto v : mdrp::prosac::growth_table(n, m, ssz)) printf(" %llu", (unsigned long long)v);
        printf("\nsubset");
        for (auto v : mdrp::prosac::subset_schedule(n, m, count, false, ssz)) printf(" %u", v);
        printf("\ntruncated");
        for (auto v : mdrp::prosac::subset_schedule(n, m, count, true, ssz)) printf(" %u", v);
        printf("\nprogressive %llu\n", (unsigned long long)mdrp::prosac::prosac_samples(m));
    }
    return 0;
}
