// TEST INFRASTRUCTURE: host/trace_plain.cpp's parsing, planning and refusals alone, as a program of its own (tests/test_gl64_trace_plan_cpp.py
// builds it with -fsanitize=address,undefined and runs it): no device - the C ABI's entry points the driver would call are stubs that abort.
//   trace_plain_plan_test trace.bin memory.bin public.bin n_steps [status words ...]
// public.bin: (u64 address, u64 value) pairs.  Prints the plan (or "refused: <message>"), then, with 16 status words, the refusal they ask for.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>

#include "../../sandstorm_amd/host/trace_plain.hpp"

#define STUB(name, ...) ss_status name(__VA_ARGS__) { fprintf(stderr, #name " called without a device\n"); abort(); }
extern "C" {
const char *ss_last_error(void) { return "stub"; }
STUB(ss_ctx_sync, ss_ctx *)
STUB(ss_dev_alloc, ss_ctx *, size_t, void **)
STUB(ss_dev_free, ss_ctx *, void *)
STUB(ss_dev_zero, ss_ctx *, void *, size_t)
STUB(ss_upload_async, ss_ctx *, void *, const void *, size_t, uint64_t *)
STUB(ss_wait_upload, ss_ctx *, uint64_t)
STUB(ss_trace_status, ss_ctx *, const uint32_t *, uint32_t *)
STUB(ss_trace_gl64_memory_image, ss_ctx *, const uint64_t *, uint64_t, uint64_t *, uint64_t)
STUB(ss_trace_gl64_cpu_cells, ss_ctx *, const uint64_t *, uint64_t, const uint64_t *, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t *, uint64_t *, uint64_t *, uint64_t *,
     uint32_t *, uint32_t *)
STUB(ss_trace_gl64_rc_pool, ss_ctx *, const ss_trace_rc_plan *, const uint32_t *, const uint16_t *, uint64_t, uint64_t, uint64_t *)
STUB(ss_trace_gl64_ordered_memory, ss_ctx *, uint64_t, uint64_t, uint64_t *, uint64_t *, uint32_t *, const uint32_t *, const uint64_t *, uint32_t, uint64_t, uint32_t *)
}

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 5 && argc != 5 + (int)SS_TRACE_STATUS_WORDS) return 2;
    const std::vector<uint8_t> trace = slurp(argv[1]), memory = slurp(argv[2]), pub = slurp(argv[3]);
    const uint64_t n_steps = strtoull(argv[4], nullptr, 10);
    std::vector<uint64_t> addr, value;
    for (size_t k = 0; k + 16 <= pub.size(); k += 16) {
        uint64_t a, v;
        memcpy(&a, pub.data() + k, 8); memcpy(&v, pub.data() + k + 8, 8);
        addr.push_back(a); value.push_back(v);
    }
    try {
        // exact-size copies: a read past either file is a read past its allocation
        std::vector<uint8_t> t(trace.begin(), trace.end()), m(memory.begin(), memory.end());
        const ssh::PlainTracePlan plan = ssh::plain_trace_plan(t.data(), t.size(), m.data(), m.size(), n_steps, addr.data(), value.data(), addr.size());
        printf("n %llu cells %llu lo %u hi %u pad_value %llu\nfirst", (unsigned long long)plan.n, (unsigned long long)plan.cells, plan.rc_lo, plan.rc_hi,
               (unsigned long long)plan.pad_value);
        for (uint32_t v : plan.first) printf(" %u", v);
        printf("\npadding");
        for (uint16_t v : plan.padding) printf(" %u", v);
        printf("\npublic");
        for (size_t k = 0; k < plan.public_addr.size(); ++k) printf(" %u:%llu", plan.public_addr[k], (unsigned long long)plan.public_value[k]);
        printf("\n");
        if (argc > 5) {
            uint32_t st[SS_TRACE_STATUS_WORDS];
            for (unsigned k = 0; k < SS_TRACE_STATUS_WORDS; ++k) st[k] = (uint32_t)strtoull(argv[5 + k], nullptr, 10);
            std::vector<uint64_t> states(3 * n_steps);
            memcpy(states.data(), t.data(), t.size());
            printf("refusal: %s\n", ssh::plain_trace_refusal(plan, states.data(), st).c_str());
        }
    } catch (const std::exception &e) { printf("refused: %s\n", e.what()); }
    return 0;
}
