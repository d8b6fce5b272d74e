// trace_plain.cpp — see trace_plain.hpp
#include "trace_plain.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace ssh {

namespace {
constexpr uint64_t GL_P = 0xFFFFFFFF00000001ull;
constexpr uint64_t NOT_HELD = ~0ull;
[[noreturn]] void fail(const std::string &m) { throw std::runtime_error("trace: " + m); }
uint64_t word_at(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
uint64_t held(const PlainTracePlan &plan, uint64_t a) { return a < plan.cells ? plan.image[a] : NOT_HELD; }

// device memory and uploads of one generation; everything is freed when it goes
struct Device {
    ss_ctx *ctx;
    std::vector<void *> owned;
    bool synced = false;
    explicit Device(ss_ctx *c) : ctx(c) {}
    ~Device() {
        if (!synced) (void)ss_ctx_sync(ctx);                          // (an exception on the way: nothing may still read what is freed here)
        for (void *p : owned) (void)ss_dev_free(ctx, p);
    }
    void check(ss_status st) const { if (st != SS_OK) fail(std::string("device: ") + ss_last_error()); }
    void *alloc(size_t bytes) {
        void *p = nullptr;
        check(ss_dev_alloc(ctx, bytes ? bytes : 8, &p));
        owned.push_back(p);
        return p;
    }
    // on the context's copy stream, the kernels enqueued after this call behind it; src stays where it is until the generation ends
    void *upload(const void *src, size_t bytes) {
        if (!bytes) return nullptr;
        void *d = alloc(bytes);
        plain_trace_stats().bytes_uploaded += bytes;
        uint64_t ticket = 0;
        check(ss_upload_async(ctx, d, src, bytes, &ticket));
        check(ss_wait_upload(ctx, ticket));
        return d;
    }
};
}  // namespace

PlainTraceStats &plain_trace_stats() { static thread_local PlainTraceStats s; return s; }

PlainTracePlan plain_trace_plan(const uint8_t *trace_bin, uint64_t trace_len, const uint8_t *memory_bin, uint64_t memory_len, uint64_t n_steps,
                                const uint64_t *mem_addresses, const uint64_t *mem_values, uint64_t n_mem) {
    if ((trace_len && !trace_bin) || (memory_len && !memory_bin) || (n_mem && (!mem_addresses || !mem_values))) fail("NULL argument");
    if (!n_steps || (n_steps & (n_steps - 1))) fail("the number of cycles must be a power of two");
    if (n_steps > (1ull << 28)) fail("more than 2^28 cycles");
    if (trace_len != 24 * n_steps) fail("trace file does not hold the run's cycles");
    if (memory_len % 40) fail("memory file is not a sequence of (u64 address, 32-byte word) records");
    PlainTracePlan plan;
    plan.n_steps = n_steps;
    plan.n = 16 * n_steps;
    // continuous memory has an access per address and n / 2 accesses in all: no valid run touches a cell beyond n / 2
    plan.cells = plan.n / 2 + 2;
    plan.image.assign(plan.cells, NOT_HELD);
    for (uint64_t k = 0; k < memory_len / 40; ++k) {                  // the device's rule (ss_trace_gl64_memory_image)
        const uint8_t *r = memory_bin + 40 * k;
        const uint64_t a = word_at(r), w = word_at(r + 8);
        if (a >= plan.cells || (word_at(r + 16) | word_at(r + 24) | word_at(r + 32)) || w >= GL_P) continue;
        plan.image[a] = w;
    }
    // the range-check pool: every cycle's three offsets (a cycle whose instruction the image does not hold is the device's to refuse)
    std::vector<uint32_t> count(1u << 16, 0);
    uint64_t decoded = 0;
    for (uint64_t c = 0; c < n_steps; ++c) {
        const uint64_t w = held(plan, word_at(trace_bin + 24 * c + 16));
        if (w == NOT_HELD) continue;
        ++count[w & 0xffff]; ++count[(w >> 16) & 0xffff]; ++count[(w >> 32) & 0xffff];
        ++decoded;
    }
    uint32_t lo = 0xffff, hi = 0;
    for (uint32_t v = 0; v < (1u << 16); ++v) if (count[v]) { lo = std::min(lo, v); hi = std::max(hi, v); }
    if (!decoded) lo = hi = 0;
    plan.rc_lo = lo; plan.rc_hi = hi;
    plan.first.assign((size_t)(hi - lo) + 2, 0);
    for (uint32_t v = lo; v <= hi; ++v) {
        if (!count[v]) plan.padding.push_back((uint16_t)v);
        plan.first[v - lo + 1] = plan.first[v - lo] + std::max(count[v], 1u);
    }
    if (plan.padding.size() > n_steps || plan.first.back() > plan.n / 4) fail("range-check values do not fit the trace");
    if (n_mem > plan.n / 8) fail("public memory does not fit");
    bool has_one = false;
    for (uint64_t k = 0; k < n_mem; ++k) {
        const uint64_t a = mem_addresses[k], v = mem_values[k] >= GL_P ? mem_values[k] - GL_P : mem_values[k];
        plan.public_addr.push_back(a > 0xffffffffull ? 0xffffffffu : (uint32_t)a);
        plan.public_value.push_back(v);
        if (a == 1 && !has_one) { has_one = true; plan.pad_value = v; }
    }
    if (!has_one) fail("the public memory holds no value at address 1 (the padding pair)");
    return plan;
}

std::string plain_trace_refusal(const PlainTracePlan &plan, const uint64_t *states, const uint32_t st[SS_TRACE_STATUS_WORDS]) {
    const uint32_t err = st[0];
    if (!err) return "";
    auto cycle_of = [&](uint32_t bit) {                                // the cycle that belongs to THIS bit (its own status word)
        uint32_t b = 0;
        while (!((bit >> b) & 1)) ++b;
        const uint64_t c = (uint32_t)~st[SS_TRACE_STATUS_GL_CYCLE + b];
        return c < plan.n_steps ? c : 0;
    };
    const std::string address = std::to_string((uint32_t)~st[1]);
    if (err & SS_TRACE_ERR_MISSING_CELL) {
        const uint64_t c = cycle_of(SS_TRACE_ERR_MISSING_CELL), ap = states[3 * c], fp = states[3 * c + 1], pc = states[3 * c + 2];
        uint64_t missing = pc;
        const uint64_t w = held(plan, pc);
        if (w != NOT_HELD) {                                          // the cycle's accesses in base_trace's order: dst, op0, op1
            auto flag = [&](int f) { return (w >> (48 + f)) & 1; };
            const uint64_t dst_addr = (w & 0xffff) + (flag(0) ? fp : ap) - 0x8000, op0_addr = ((w >> 16) & 0xffff) + (flag(1) ? fp : ap) - 0x8000;
            const uint64_t src = flag(2) + 2 * flag(3) + 4 * flag(4), op0 = held(plan, op0_addr);
            const uint64_t base = src == 0 ? (op0 == NOT_HELD ? 0 : op0) : src == 1 ? pc : src == 2 ? fp : src == 4 ? ap : 0;
            const uint64_t op1_addr = ((w >> 32) & 0xffff) + base - 0x8000;
            missing = held(plan, dst_addr) == NOT_HELD ? dst_addr : op0 == NOT_HELD ? op0_addr : op1_addr;
        }
        return "the run reads address " + std::to_string(missing) + ", which memory.bin does not hold";
    }
    if (err & SS_TRACE_ERR_TOO_MANY_GAPS) return "more memory holes than gap cells";
    if (err & SS_TRACE_ERR_NOT_INSTRUCTION) return "instruction at pc " + std::to_string(states[3 * cycle_of(SS_TRACE_ERR_NOT_INSTRUCTION) + 2]) + " has bit 63 set";
    if (err & SS_TRACE_ERR_BAD_OP1_SOURCE) return "invalid op1 source (cycle " + std::to_string(cycle_of(SS_TRACE_ERR_BAD_OP1_SOURCE)) + ")";
    if (err & SS_TRACE_ERR_BAD_RES_LOGIC) return "invalid res logic (cycle " + std::to_string(cycle_of(SS_TRACE_ERR_BAD_RES_LOGIC)) + ")";
    if (err & SS_TRACE_ERR_NOT_AN_ADDRESS) return "a memory cell is used as an address but is not one (cycle " + std::to_string(cycle_of(SS_TRACE_ERR_NOT_AN_ADDRESS)) + ")";
    if (err & (SS_TRACE_ERR_PUBLIC_ZERO | SS_TRACE_ERR_PUBLIC_CELLS | SS_TRACE_ERR_NO_ONES))
        return "the public-memory cells must be the only accesses of address 0, and memory starts at 1";
    if (err & (SS_TRACE_ERR_ADDRESS_RANGE | SS_TRACE_ERR_NOT_SINGLE_VALUED | SS_TRACE_ERR_NOT_CONTINUOUS)) return "memory is not continuous and single-valued at address " + address;
    return "the ordered memory does not fill its column";
}

void plain_base_trace_device(ss_ctx *ctx, const uint8_t *trace_bin, uint64_t trace_len, const uint8_t *memory_bin, uint64_t memory_len, uint64_t n_steps,
                             const uint64_t *mem_addresses, const uint64_t *mem_values, uint64_t n_mem, uint64_t *const d_cols[5]) {
    if (!ctx || !d_cols) fail("NULL argument");
    for (int c = 0; c < 5; ++c) if (!d_cols[c]) fail("NULL column");
    plain_trace_stats() = PlainTraceStats{};
    const PlainTracePlan plan = plain_trace_plan(trace_bin, trace_len, memory_bin, memory_len, n_steps, mem_addresses, mem_values, n_mem);
    std::vector<uint64_t> states(3 * n_steps);                        // (aligned words for the refusal's lookups; the upload reads the file)
    memcpy(states.data(), trace_bin, trace_len);
    enum { FLAGS = 0, NPC = 1, MEMORY = 2, RANGE_CHECK = 3, AUXILIARY = 4 };       // layouts/src/plain/mod.rs
    Device dev(ctx);
    uint32_t *d_status = (uint32_t *)dev.alloc(SS_TRACE_STATUS_WORDS * 4);
    dev.check(ss_dev_zero(ctx, d_status, SS_TRACE_STATUS_WORDS * 4));
    uint32_t *d_pool_addr = (uint32_t *)dev.alloc(plan.n / 2 * 4);
    const uint64_t *d_states = (const uint64_t *)dev.upload(trace_bin, trace_len);
    const uint64_t *d_records = (const uint64_t *)dev.upload(memory_bin, memory_len);
    uint64_t *d_image = (uint64_t *)dev.alloc(plan.cells * 8);
    const uint32_t *d_first = (const uint32_t *)dev.upload(plan.first.data(), plan.first.size() * 4);
    const uint16_t *d_padding = (const uint16_t *)dev.upload(plan.padding.data(), plan.padding.size() * 2);
    const uint32_t *d_public_addr = (const uint32_t *)dev.upload(plan.public_addr.data(), plan.public_addr.size() * 4);
    const uint64_t *d_public_value = (const uint64_t *)dev.upload(plan.public_value.data(), plan.public_value.size() * 8);
    ss_trace_rc_plan rc{};
    rc.rc_lo = plan.rc_lo; rc.rc_hi = plan.rc_hi; rc.n_padding = plan.padding.size(); rc.pad0 = 0;
    rc.ordered_step = 4; rc.ordered_off = 2; rc.unused_off = 12;
    // the reference's section order: the CPU's cells, the range-check pool, the memory
    dev.check(ss_trace_gl64_memory_image(ctx, d_records, memory_len / 40, d_image, plan.cells));
    dev.check(ss_trace_gl64_cpu_cells(ctx, d_states, n_steps, d_image, plan.cells, plan.pad_value, plan.rc_hi, plan.n, d_cols[FLAGS], d_cols[NPC], d_cols[RANGE_CHECK],
                                      d_cols[AUXILIARY], d_pool_addr, d_status));
    dev.check(ss_trace_gl64_rc_pool(ctx, &rc, d_first, d_padding, n_steps, plan.n, d_cols[RANGE_CHECK]));
    dev.check(ss_trace_gl64_ordered_memory(ctx, plan.n, plan.n, d_cols[NPC], d_cols[MEMORY], d_pool_addr, d_public_addr, d_public_value, (uint32_t)n_mem,
                                           plan.pad_value, d_status));
    uint32_t st[SS_TRACE_STATUS_WORDS];
    dev.check(ss_trace_status(ctx, d_status, st));
    dev.synced = true;
    const std::string refusal = plain_trace_refusal(plan, states.data(), st);
    if (!refusal.empty()) fail(refusal);
}

}  // namespace ssh
