// Stand-alone host program (its own main; built with -fsanitize=address,undefined by tests/test_gl64_lde_blowup_on_host.py, never loaded
// into python): the 64-bit field's row sub-sampling kernel of sandstorm_amd/csrc/goldilocks.hip in its host build (tests/hipemu:
// workgroups one after the other on the CPU) over the shapes of tests/test_gpu_gl64_lde_blowup.py's first case - nrows_out in
// {1, 2, 3, 255, 256, 257, 1000, 4097}, log_stride 0 .. 4, 1 / 3 / 16 columns a launch (the seventeenth column is the entry point's
// second launch: one column) - and once more per shape into a destination 8 bytes off a 16-byte boundary (the kernel's 8-byte store
// path).  Every buffer is a heap block of exactly the size the entry point documents - inputs ((nrows_out - 1) << log_stride) + 1 words,
// outputs nrows_out - so a read or a write one word too far is the sanitizer's report, and the values are checked against the definition.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include "kernels.h"

int main() {
    const uint64_t rows[] = {1, 2, 3, 255, 256, 257, 1000, 4097};
    const uint32_t ncols_of[] = {1, 3, 16, 1};                  // the last: the unaligned destination
    const uint64_t P = 0xFFFFFFFF00000001ull, SENTINEL = 0xA5A5A5A5A5A5A5A5ull;
    uint64_t state = 0x61DE, bad = 0, launches = 0;
    auto next = [&]() { state += 0x9E3779B97F4A7C15ull; uint64_t z = state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    for (uint64_t nrows_out : rows)
        for (uint32_t log_stride = 0; log_stride <= 4; ++log_stride)
            for (int k = 0; k < 4; ++k) {
                const uint32_t ncols = ncols_of[k];
                const uint64_t shift = k == 3 ? 1 : 0;          // words between the block's start and the destination
                const uint64_t in_words = ((nrows_out - 1) << log_stride) + 1;
                std::vector<uint64_t *> in(ncols), block(ncols), out(ncols);
                for (uint32_t c = 0; c < ncols; ++c) {
                    in[c] = new uint64_t[in_words];
                    block[c] = new uint64_t[nrows_out + shift];
                    out[c] = block[c] + shift;
                    for (uint64_t i = 0; i < in_words; ++i) in[c][i] = i % 97 == 0 ? ~0ull : i % 89 == 0 ? P : i % 83 == 0 ? P - 1 : next();
                    for (uint64_t i = 0; i < nrows_out + shift; ++i) block[c][i] = SENTINEL;
                    if (((uintptr_t)out[c] & 15) != 8 * shift) ++bad;      // (operator new hands out 16-byte aligned blocks)
                }
                if (ss::launch_gl_subsample_rows(nullptr, in.data(), out.data(), ncols, nrows_out, log_stride) != hipSuccess) ++bad;
                if (hipDeviceSynchronize() != hipSuccess) ++bad;
                ++launches;
                for (uint32_t c = 0; c < ncols; ++c) {
                    for (uint64_t j = 0; j < nrows_out; ++j)
                        if (out[c][j] != in[c][j << log_stride]) ++bad;
                    if (shift && block[c][0] != SENTINEL) ++bad;
                    delete[] in[c];
                    delete[] block[c];
                }
            }
    // more columns than the kernarg table holds, or nothing to do: no launch
    uint64_t *none[1] = {nullptr};
    if (ss::launch_gl_subsample_rows(nullptr, none, none, ss::MAX_COLS + 1, 4, 1) == hipSuccess) ++bad;
    if (ss::launch_gl_subsample_rows(nullptr, none, none, 1, 0, 1) != hipSuccess) ++bad;
    printf("%llu launches, %llu mismatches\n", (unsigned long long)launches, (unsigned long long)bad);
    return bad ? 1 : 0;
}
