// TEST INFRASTRUCTURE: a program of its own around sandstorm_amd/host/gl_check_blob.hpp (the parser of the 64-bit field's check callback
// blob), built with -fsanitize=address,undefined by tests/test_gl64_check_blob_parser.py.  Every blob lives in a heap block of exactly
// its length, so a parser that reads a word past a truncated blob is caught by the sanitizer, not only by the missing refusal.
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "gl_check_blob.hpp"

using ssh::gl::CheckBlob;
using ssh::gl::parse_check_blob;

static std::vector<uint64_t> text(const std::string &s) {
    std::vector<uint64_t> w{(uint64_t)s.size()};
    for (size_t i = 0; i < s.size(); i += 8) {
        uint64_t v = 0;
        for (size_t b = 0; b < 8 && i + b < s.size(); ++b) v |= (uint64_t)(uint8_t)s[i + b] << (8 * b);
        w.push_back(v);
    }
    return w;
}
static void append(std::vector<uint64_t> &a, const std::vector<uint64_t> &b) { a.insert(a.end(), b.begin(), b.end()); }

// two checks: MOV acc0 <- cell; CHECK 0; MOV acc0 <- const 0; CHECK 1
static std::vector<uint64_t> good_blob() {
    std::vector<uint64_t> w{4, 1, 0, 0, 0, 2};
    append(w, {0 | (3u << 12), 0, SS_OP_CHECK, 0, 0 | (2u << 12), 0, SS_OP_CHECK, 1});
    append(w, {5, 6, 7});
    append(w, {0, 1, 16, 0});                               // check 0: no numerator factor, den (16, 0)
    append(w, text("cpu/first"));
    append(w, text("every row"));
    append(w, {1, 1, 15, 1, 16, 0});                        // check 1: num (1, 15), den (16, 0)
    append(w, text("a name of more than eight bytes"));
    append(w, text(""));
    return w;
}

static int failures = 0;
static std::string parse_error(const std::vector<uint64_t> &w) {
    std::unique_ptr<uint64_t[]> heap(new uint64_t[w.size() ? w.size() : 1]);       // exactly the blob: no slack behind it
    if (!w.empty()) memcpy(heap.get(), w.data(), w.size() * 8);
    try {
        parse_check_blob(heap.get(), w.size());
    } catch (const std::exception &e) {
        return e.what();
    }
    return "";
}
static void refused(const char *what, const std::vector<uint64_t> &w, const std::string &needle) {
    const std::string err = parse_error(w);
    const bool ok = err.find("check callback: ") == 0 && err.find(needle) != std::string::npos;
    if (!ok) { ++failures; printf("FAIL %s: wanted a refusal with '%s', got '%s'\n", what, needle.c_str(), err.c_str()); }
}

int main() {
    const std::vector<uint64_t> good = good_blob();
    {
        const std::string err = parse_error(good);
        if (!err.empty()) { ++failures; printf("FAIL the good blob is refused: %s\n", err.c_str()); }
        std::unique_ptr<uint64_t[]> heap(new uint64_t[good.size()]);
        memcpy(heap.get(), good.data(), good.size() * 8);
        const CheckBlob b = parse_check_blob(heap.get(), good.size());
        const bool ok = b.code.size() == 8 && b.consts == std::vector<uint64_t>{5, 6, 7} && b.domains.size() == 2 && b.domains[1].n_num == 1 &&
                        b.domains[1].num[0][1] == 15 && b.domains[0].n_den == 1 && b.domains[0].den[0][0] == 16 && b.names[0] == "cpu/first" &&
                        b.domain_names[0] == "every row" && b.names[1] == "a name of more than eight bytes" && b.domain_names[1].empty();
        if (!ok) { ++failures; printf("FAIL the good blob is parsed into something else\n"); }
    }
    // truncated at EVERY length: each prefix is refused, none is read past its end
    int prefixes = 0;
    for (size_t len = 0; len < good.size(); ++len) {
        const std::string err = parse_error(std::vector<uint64_t>(good.begin(), good.begin() + len));
        ++prefixes;
        if (err.find("check callback: ") != 0 || (err.find("truncated") == std::string::npos && err.find("shorter than its header") == std::string::npos)) {
            ++failures; printf("FAIL prefix of %zu words: '%s'\n", len, err.c_str());
        }
    }
    auto with = [&](size_t at, uint64_t v) { std::vector<uint64_t> w = good; w[at] = v; return w; };
    refused("NULL", {}, "shorter than its header");
    refused("no instruction", with(0, 0), "instruction count 0 out of range");
    refused("huge instruction count", with(0, ~0ull), "instruction count");
    refused("huge constant count", with(1, 1ull << 60), "constant count");
    refused("huge slot count", with(2, 1ull << 40), "slot count");
    refused("tables without an address", with(3, 1), "1 tables and no table address");
    refused("no check", with(5, 0), "check count 0 out of range");
    refused("more checks than CHECK instructions", with(5, 3), "2 CHECK instructions for 3 checks");
    refused("fewer checks than CHECK instructions", with(5, 1), "2 CHECK instructions for 1 checks");
    refused("a code word beyond 32 bits", with(7, 1ull << 32), "code word 1 does not fit 32 bits");
    refused("a constant that is no field element", with(6 + 8 + 1, 0xFFFFFFFF00000001ull), "constant 0 is not an element of the extension");
    refused("17 denominator factors", with(6 + 8 + 3 + 1, 17), "17 denominator factors exceed SS_CHECK_MAX_FACTORS = 16");
    refused("17 numerator factors", with(6 + 8 + 3, 17), "17 numerator factors exceed SS_CHECK_MAX_FACTORS = 16");
    refused("a domain without a denominator", with(6 + 8 + 3 + 1, 0), "check 0");
    refused("a name longer than the blob", with(6 + 8 + 3 + 4, 4000), "truncated in check 0's name");
    refused("a name of absurd length", with(6 + 8 + 3 + 4, 1ull << 50), "check 0's name of");
    {
        std::vector<uint64_t> w = good;
        w.push_back(0);
        refused("words left over", w, "1 words left over after check 1");
    }
    printf("%d prefixes refused, %d failures\n", prefixes, failures);
    return failures ? 1 : 0;
}
