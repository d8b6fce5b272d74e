// gl_check_blob.hpp — what the 64-bit field's check callback hands the C++ host (ssh_gl_check_cb, host_capi.cpp): the check program of
// the layout (one SS_OP_CHECK per constraint over its bare numerator), the per-check domain factor lists and the names, as ONE u64 blob:
//   [n_instr, n_consts, n_slots, n_tables, d_tables, n_checks | code: 2 n_instr words, one per u64 | consts: 3 n_consts |
//    table_desc: 2 n_tables | per check: n_num, (p, e) x n_num, n_den, (p, e) x n_den, name, domain name]
// with a string as its byte length followed by its bytes packed little-endian, eight to a u64.  The blob comes from another language
// through a callback, so the parser trusts nothing: every count is checked against what is left before anything is read, and what is
// refused is refused by name.  Header-only and free of the device runtime: tests/cpp/gl_check_blob_test.cpp drives it on its own.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sandstorm_hip.h"

namespace ssh {
namespace gl {

struct CheckBlob {
    std::vector<uint32_t> code;                             // two words per instruction
    std::vector<uint64_t> consts;                           // three values per constant
    uint32_t n_slots = 0;
    const uint64_t *d_tables = nullptr;
    std::vector<uint32_t> table_desc;
    std::vector<ss_check_domain> domains;                   // one per check
    std::vector<std::string> names, domain_names;
};

inline CheckBlob parse_check_blob(const uint64_t *blob, uint64_t len) {
    static constexpr uint64_t GL_P = 0xFFFFFFFF00000001ull, MAX_COUNT = 1ull << 24, MAX_NAME = 4096;
    auto refuse = [](const std::string &what) -> void { throw std::runtime_error("check callback: " + what); };
    if (!blob) refuse("NULL blob");
    if (len < 6) refuse("blob of " + std::to_string(len) + " words is shorter than its header of 6");
    const uint64_t n_instr = blob[0], n_consts = blob[1], n_slots = blob[2], n_tables = blob[3], n_checks = blob[5];
    if (n_instr == 0 || n_instr > MAX_COUNT) refuse("instruction count " + std::to_string(n_instr) + " out of range");
    if (n_consts > MAX_COUNT) refuse("constant count " + std::to_string(n_consts) + " out of range");
    if (n_slots > MAX_COUNT) refuse("slot count " + std::to_string(n_slots) + " out of range");
    if (n_tables > MAX_COUNT) refuse("table count " + std::to_string(n_tables) + " out of range");
    if (n_checks == 0 || n_checks > MAX_COUNT) refuse("check count " + std::to_string(n_checks) + " out of range");
    if (n_tables && !blob[4]) refuse(std::to_string(n_tables) + " tables and no table address");
    uint64_t at = 6;
    auto need = [&](uint64_t words, const std::string &what) {
        if (words > len - at) refuse("blob truncated in " + what + ": " + std::to_string(words) + " words wanted at word " + std::to_string(at) + " of " + std::to_string(len));
    };
    CheckBlob out;
    out.n_slots = (uint32_t)n_slots;
    out.d_tables = reinterpret_cast<const uint64_t *>((uintptr_t)blob[4]);
    need(2 * n_instr, "the code");
    uint64_t checks_in_code = 0;
    for (uint64_t i = 0; i < 2 * n_instr; ++i) {
        const uint64_t w = blob[at++];
        if (w >> 32) refuse("code word " + std::to_string(i) + " does not fit 32 bits");
        out.code.push_back((uint32_t)w);
        if (!(i & 1) && (w & 0xff) == SS_OP_CHECK) ++checks_in_code;
    }
    if (checks_in_code != n_checks) refuse("the code holds " + std::to_string(checks_in_code) + " CHECK instructions for " + std::to_string(n_checks) + " checks");
    need(3 * n_consts, "the constants");
    for (uint64_t i = 0; i < 3 * n_consts; ++i) {
        if (blob[at] >= GL_P) refuse("constant " + std::to_string(i / 3) + " is not an element of the extension");
        out.consts.push_back(blob[at++]);
    }
    need(2 * n_tables, "the table descriptions");
    for (uint64_t i = 0; i < 2 * n_tables; ++i) {
        if (blob[at] >> 32) refuse("table description word " + std::to_string(i) + " does not fit 32 bits");
        out.table_desc.push_back((uint32_t)blob[at++]);
    }
    auto string_at = [&](const std::string &what) {
        need(1, what);
        const uint64_t bytes = blob[at++];
        if (bytes > MAX_NAME) refuse(what + " of " + std::to_string(bytes) + " bytes");
        const uint64_t words = (bytes + 7) / 8;
        need(words, what);
        std::string s;
        for (uint64_t b = 0; b < bytes; ++b) s.push_back((char)((blob[at + b / 8] >> (8 * (b % 8))) & 0xff));
        at += words;
        return s;
    };
    for (uint64_t k = 0; k < n_checks; ++k) {
        const std::string where = "check " + std::to_string(k);
        ss_check_domain d;
        d.n_num = d.n_den = 0;
        for (auto &f : d.num) f[0] = f[1] = 0;
        for (auto &f : d.den) f[0] = f[1] = 0;
        for (int side = 0; side < 2; ++side) {
            need(1, where + "'s factor count");
            const uint64_t cnt = blob[at++];
            if (cnt > SS_CHECK_MAX_FACTORS)
                refuse(where + ": " + std::to_string(cnt) + (side ? " denominator" : " numerator") + " factors exceed SS_CHECK_MAX_FACTORS = " + std::to_string(SS_CHECK_MAX_FACTORS));
            need(2 * cnt, where + "'s factors");
            for (uint64_t j = 0; j < cnt; ++j) {
                (side ? d.den : d.num)[j][0] = blob[at++];
                (side ? d.den : d.num)[j][1] = blob[at++];
            }
            (side ? d.n_den : d.n_num) = (uint32_t)cnt;
        }
        if (d.n_den == 0) refuse(where + ": a domain without a denominator factor holds no row");
        out.domains.push_back(d);
        out.names.push_back(string_at(where + "'s name"));
        out.domain_names.push_back(string_at(where + "'s domain name"));
    }
    if (at != len) refuse(std::to_string(len - at) + " words left over after check " + std::to_string(n_checks - 1));
    return out;
}

}  // namespace gl
}  // namespace ssh
