// trace_plain.hpp — the plain layout's base trace over the 64-bit field p = 2^64 - 2^32 + 1, made ON the device from the raw files: the
// plan and the driver above ss_trace_gl64_* (csrc/trace.hip), not a second column generator - the cells' specification stays
// sandstorm_amd/layouts/plain.py base_trace (ExecutionTrace::new, layouts/src/plain/trace.rs:60-262, which cli/src/main.rs:186-202 runs
// inside its "Proof generated in" timer).  The host parses the files, counts the 16-bit range-check histogram from the decoded offsets,
// refuses what base_trace refuses before anything is launched, uploads the files as they are with the plan, launches the four entry
// points in the reference's section order and reads the status block once.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sandstorm_hip.h"

namespace ssh {

// what the last generation on the calling thread uploaded (ssh_gl_trace_last_stats)
struct PlainTraceStats { uint64_t bytes_uploaded = 0; };
PlainTraceStats &plain_trace_stats();

// the plan of a generation: everything the host decides before a kernel runs - no device involved (tests/cpp/trace_plain_plan_test.cpp
// drives it alone).  Throws what base_trace refuses from the files alone.
struct PlainTracePlan {
    uint64_t n_steps = 0, n = 0, cells = 0;      // cycles, trace rows, cells of the memory image (n / 2 + 2)
    std::vector<uint64_t> image;                 // memory.bin as the device's image: image[address], all ones = not held
    uint32_t rc_lo = 0, rc_hi = 0;               // the range-check pool's smallest and largest value
    std::vector<uint32_t> first;                 // d_first of ss_trace_gl64_rc_pool: rc_hi - rc_lo + 2 entries
    std::vector<uint16_t> padding;               // d_padding: the values of [rc_lo, rc_hi] nothing uses
    std::vector<uint32_t> public_addr;           // the public memory: addresses (saturated at 2^32 - 1), values below p
    std::vector<uint64_t> public_value;
    uint64_t pad_value = 0;                      // the value at address 1
};
PlainTracePlan plain_trace_plan(const uint8_t *trace_bin, uint64_t trace_len, const uint8_t *memory_bin, uint64_t memory_len, uint64_t n_steps,
                                const uint64_t *mem_addresses, const uint64_t *mem_values, uint64_t n_mem);
// the refusal a status block asks for, in the order base_trace raises (empty: none).  states: trace.bin's words
std::string plain_trace_refusal(const PlainTracePlan &plan, const uint64_t *states, const uint32_t status[SS_TRACE_STATUS_WORDS]);

// trace.bin / memory.bin (binary/src/lib.rs:33-56, 147-222) and the public memory (one u64 per address and per value) -> the five base
// columns in d_cols (flags, pool, ordered memory, range check, auxiliary: 16 * n_steps u64 each), final when the call returns.  Throws
// std::runtime_error with base_trace's refusals (and "the run reads address %d, which memory.bin does not hold", which Python lacks).
void plain_base_trace_device(ss_ctx *ctx, const uint8_t *trace_bin, uint64_t trace_len, const uint8_t *memory_bin, uint64_t memory_len, uint64_t n_steps,
                             const uint64_t *mem_addresses, const uint64_t *mem_values, uint64_t n_mem, uint64_t *const d_cols[5]);

}  // namespace ssh
