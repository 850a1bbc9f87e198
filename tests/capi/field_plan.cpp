// field_plan.cpp -- stand-alone driver of the launch plan of the field kernels (neddf_amd/csrc/field_plan.h: field_plan, each_span) for
// tests/test_field_plan.py: no GPU, no Python, no library.  Built by the test, the host side under AddressSanitizer + UBSan.
//
//   field_plan <case file>      one output line per case on stdout
//
// Case file (text), one case per line:
//   <full> <use3> <N> <env chunk log2, 0: unset> <feat_row> <aux_row> <feat_cap> <aux_cap> <cache_row> <cache_chunk> <probe ok> <free bytes>
// Output line, the walk field_forward makes:
//   <chunk> <ddf_sub> <probed> <cache> <times the probe ran>  then per chunk  C <off> <n>  and per distance launch before it  D <so> <n_sub>
#include "field_plan.h"         // -I neddf_amd/csrc

#include <stdio.h>

using namespace neddf;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: field_plan <case file>\n"); return 2; }
    FILE *fp = fopen(argv[1], "r");
    if (!fp) { perror(argv[1]); return 2; }
    int full, use3, env, probe_ok;
    long long N, cache_chunk;
    unsigned long long feat_row, aux_row, feat_cap, aux_cap, cache_row, free_b;
    while (fscanf(fp, "%d %d %lld %d %llu %llu %llu %llu %llu %lld %d %llu", &full, &use3, &N, &env, &feat_row, &aux_row, &feat_cap, &aux_cap,
                  &cache_row, &cache_chunk, &probe_ok, &free_b) == 12) {
        const FieldPlanIn in{ full != 0, use3 != 0, (int64_t)N, env, (size_t)feat_row, (size_t)aux_row, (size_t)feat_cap, (size_t)aux_cap,
                              (size_t)cache_row, (int64_t)cache_chunk };
        int probes = 0;
        const FieldPlan plan = field_plan(in, [&](size_t &out) { ++probes; out = (size_t)free_b; return probe_ok != 0; });
        printf("%lld %lld %d %d %d", (long long)plan.chunk, (long long)plan.ddf_sub, (int)plan.probed, (int)plan.cache, probes);
        if (plan.chunk < 1 || plan.ddf_sub < 1) { printf("\n"); continue; }     // (the test fails on the missing walk)
        const int rc = each_span(in.N, plan.chunk, [&](int64_t off, int64_t n) -> int {
            const int rc = each_span(n, plan.ddf_sub, [&](int64_t so, int64_t n_sub) -> int {
                printf(" D %lld %lld", (long long)so, (long long)n_sub);
                return 0;
            });
            printf(" C %lld %lld", (long long)off, (long long)n);
            return rc;
        });
        printf("\n");
        if (rc) { fprintf(stderr, "the walk stopped with %d\n", rc); return 1; }
    }
    fclose(fp);
    return 0;
}
