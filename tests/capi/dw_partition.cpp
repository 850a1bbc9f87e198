// dw_partition.cpp -- stand-alone driver of the workgroup partition of the job-parallel weight gradients (neddf_amd/csrc/train_kernels.h
// dw_partition) for tests/test_dw_partition.py: no GPU, no Python, no library.  Built by the test, the host side under
// AddressSanitizer + UBSan.
//
//   dw_partition <case file>      one output line per case on stdout
//
// Case file (text), one case per line:   <cost table: 0 fp32, 1 split fp16> <cus> <n> <K of job 0> ... <K of job n-1>
// Output line:                           <grid> <wg0 of job 0> ... <wg0 of job n-1>
#include "train_kernels.h"      // -I neddf_amd/csrc

#include <stdio.h>

using namespace neddf;

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: dw_partition <case file>\n"); return 2; }
    FILE *fp = fopen(argv[1], "r");
    if (!fp) { perror(argv[1]); return 2; }
    int table, cus, n;
    while (fscanf(fp, "%d %d %d", &table, &cus, &n) == 3) {
        if (n < 1 || n > kMaxDwJobs) { fprintf(stderr, "job count %d out of range\n", n); return 2; }
        DwJobs jobs{};
        jobs.R = 4096;
        for (int i = 0; i < n; ++i) {
            int K;
            if (fscanf(fp, "%d", &K) != 1) { fprintf(stderr, "truncated case\n"); return 2; }
            jobs.add(nullptr, 256, K, K == 256, nullptr, 256, nullptr, 256, 1, 256, nullptr, 4);
            jobs.job[i].wg0 = -1;       // every entry must be written
        }
        const int grid = dw_partition(jobs, table ? dw_cost_split : dw_cost_f32, cus);
        printf("%d", grid);
        for (int i = 0; i < n; ++i) printf(" %d", jobs.job[i].wg0);
        printf("\n");
    }
    fclose(fp);
    return 0;
}
