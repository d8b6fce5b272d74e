// Stand-alone host program (its own main; built with -fsanitize=address,undefined by tests/test_lde_blowup_on_host.py, never loaded into
// python): the row sub-sampling kernel of sandstorm_amd/csrc/deep.hip in its host build (tests/hipemu: workgroups one after the other
// on the CPU) over the shapes of tests/test_gpu_lde_blowup.py's first case - nrows_out in {1, 255, 256, 257, 4096 + 48}, log_stride in
// {0, 1, 2, 3}, 1 / 3 / 16 columns a launch (the seventeenth column is the entry point's second launch: one column).  Every buffer is a
// heap block of exactly the size the entry point documents - inputs ((nrows_out - 1) << log_stride) + 1 cells, outputs nrows_out - so
// a read or a write one cell too far is the sanitizer's report, and the values are checked against the definition.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include "kernels.h"

int main() {
    const uint64_t rows[] = {1, 255, 256, 257, 4096 + 48};
    const uint32_t ncols_of[] = {1, 3, 16};
    uint64_t state = 0x1DE, bad = 0, launches = 0;
    auto next = [&]() { state += 0x9E3779B97F4A7C15ull; uint64_t z = state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    for (uint64_t nrows_out : rows)
        for (uint32_t log_stride = 0; log_stride < 4; ++log_stride)
            for (uint32_t ncols : ncols_of) {
                const uint64_t in_cells = ((nrows_out - 1) << log_stride) + 1;
                std::vector<uint64_t *> in(ncols), out(ncols);
                ss::ColPtrs cols;
                memset(&cols, 0, sizeof cols);
                for (uint32_t c = 0; c < ncols; ++c) {
                    in[c] = new uint64_t[4 * in_cells];
                    out[c] = new uint64_t[4 * nrows_out];
                    for (uint64_t i = 0; i < 4 * in_cells; ++i) in[c][i] = (i / 4) % 97 == 0 ? ~0ull : next();
                    memset(out[c], 0xA5, 32 * nrows_out);
                    cols.src[c] = in[c];
                    cols.dst[c] = out[c];
                }
                if (ss::launch_subsample_rows(nullptr, cols, ncols, nrows_out, log_stride) != hipSuccess) ++bad;
                if (hipDeviceSynchronize() != hipSuccess) ++bad;
                ++launches;
                for (uint32_t c = 0; c < ncols; ++c) {
                    for (uint64_t j = 0; j < nrows_out; ++j)
                        if (memcmp(out[c] + 4 * j, in[c] + 4 * (j << log_stride), 32)) ++bad;
                    delete[] in[c];
                    delete[] out[c];
                }
            }
    // more columns than the kernarg table holds, or nothing to do: no launch
    ss::ColPtrs none;
    memset(&none, 0, sizeof none);
    if (ss::launch_subsample_rows(nullptr, none, ss::MAX_COLS + 1, 4, 1) == hipSuccess) ++bad;
    if (ss::launch_subsample_rows(nullptr, none, 1, 0, 1) != hipSuccess) ++bad;
    printf("%llu launches, %llu mismatches\n", (unsigned long long)launches, (unsigned long long)bad);
    return bad ? 1 : 0;
}
