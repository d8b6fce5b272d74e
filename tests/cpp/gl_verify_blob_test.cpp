// gl_verify_blob_test.cpp — the 64-bit field's proof-blob parser and verifier (sandstorm_amd/host/goldilocks_verifier.cpp over
// air_plain.cpp) as a program of its own under the host sanitizers (tests/test_gl64_air_host_cpp.py builds and runs it).
//   argv[1]: a file of little-endian u64 words: n_steps, rc_min, rc_max, program (2), execution (2), n_mem, (address, value) x n_mem,
//            options (6), required_security_bits, seed (4 words = 32 bytes), blob length, the proof blob of a proof that verifies.
// The good blob must verify; every prefix of its first 64 words, 64 seeded longer prefixes, every count word set to 2^63 and 256 seeded
// single-word garblings must each be refused (an exception with a message) or - a garbled word the verifier never reads - accepted
// with the good blob's positions; nothing may read past a blob's end, which is what the sanitizers watch.
// The device runtime is not linked: the few C ABI symbols the host sources name are defined here (Keccak-256 for real).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "goldilocks_verifier.hpp"

// ---- the C ABI symbols coin.cpp and air_plain.cpp name
static void keccak_f(uint64_t s[25]) {
    static const uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
                                    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
                                    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
                                    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    static const int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
    static const int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
    for (int round = 0; round < 24; ++round) {
        uint64_t bc[5];
        for (int i = 0; i < 5; ++i) bc[i] = s[i] ^ s[i + 5] ^ s[i + 10] ^ s[i + 15] ^ s[i + 20];
        for (int i = 0; i < 5; ++i) {
            const uint64_t t = bc[(i + 4) % 5] ^ ((bc[(i + 1) % 5] << 1) | (bc[(i + 1) % 5] >> 63));
            for (int j = 0; j < 25; j += 5) s[j + i] ^= t;
        }
        uint64_t t = s[1];
        for (int i = 0; i < 24; ++i) {
            const int j = PIL[i];
            const uint64_t b = s[j];
            s[j] = (t << ROT[i]) | (t >> (64 - ROT[i]));
            t = b;
        }
        for (int j = 0; j < 25; j += 5) {
            uint64_t row[5];
            for (int i = 0; i < 5; ++i) row[i] = s[j + i];
            for (int i = 0; i < 5; ++i) s[j + i] ^= (~row[(i + 1) % 5]) & row[(i + 2) % 5];
        }
        s[0] ^= RC[round];
    }
}
extern "C" {
ss_status ss_keccak256_host(const uint8_t *msg, size_t len, uint8_t out[32]) {      // Keccak-256 (the 0x01 padding), rate 136
    uint64_t s[25] = {0};
    uint8_t block[136];
    size_t off = 0;
    for (;;) {
        const size_t take = len - off < 136 ? len - off : 136;
        memset(block, 0, sizeof block);
        if (take) memcpy(block, msg + off, take);
        off += take;
        const bool last = take < 136;
        if (last) { block[take] ^= 0x01; block[135] ^= 0x80; }
        for (int i = 0; i < 17; ++i) { uint64_t w; memcpy(&w, block + 8 * i, 8); s[i] ^= w; }
        keccak_f(s);
        if (last) break;
    }
    memcpy(out, s, 32);
    return SS_OK;
}
ss_status ss_pedersen_hash_host(const uint64_t *, const uint64_t *, uint64_t *) { return (ss_status)1; }
const char *ss_last_error(void) { return "the device runtime is not linked into this program"; }
ss_status ss_dev_alloc(ss_ctx *, size_t, void **) { return (ss_status)1; }
ss_status ss_dev_free(ss_ctx *, void *) { return (ss_status)1; }
ss_status ss_upload(ss_ctx *, void *, const void *, size_t) { return (ss_status)1; }
ss_status ss_ctx_sync(ss_ctx *) { return (ss_status)1; }
}

using namespace ssh;

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<uint64_t> w(raw.size() / 8);
    memcpy(w.data(), raw.data(), w.size() * 8);
    size_t at = 0;
    auto next = [&]() { if (at >= w.size()) { fprintf(stderr, "case file too short\n"); exit(2); } return w[at++]; };
    gl::PlainStatement st;
    st.n_steps = next(); st.rc_min = next(); st.rc_max = next();
    st.program[0] = next(); st.program[1] = next(); st.execution[0] = next(); st.execution[1] = next();
    const uint64_t n_mem = next();
    for (uint64_t i = 0; i < n_mem; ++i) { const uint64_t a = next(), v = next(); st.public_memory.push_back({a, v}); }
    gl::Options opt;
    opt.num_queries = (uint32_t)next(); opt.log_blowup = (uint32_t)next(); opt.grinding = (uint32_t)next(); opt.fold = (uint32_t)next(); opt.max_remainder = (uint32_t)next();
    const uint32_t hash_option = (uint32_t)next();
    opt.sha256 = hash_option != 0;
    const uint32_t required = (uint32_t)next();
    Digest seed;
    for (int k = 0; k < 4; ++k) { const uint64_t v = next(); memcpy(seed.data() + 8 * k, &v, 8); }
    const uint64_t blob_len = next();
    if (at + blob_len != w.size()) { fprintf(stderr, "case file: blob length\n"); return 2; }
    const std::vector<uint64_t> good(w.begin() + at, w.end());

    gl::PlainAir air(nullptr, st);
    int failures = 0;
    std::vector<uint64_t> want;
    try {
        want = gl::verify(air, opt, hash_option, seed, gl::parse_proof_blob(good.data(), good.size()), required);
    } catch (const std::exception &e) { printf("FAIL: the good blob is refused: %s\n", e.what()); return 1; }
    // run one blob from an allocation of exactly its size, so that a read past its end is a heap overflow the sanitizer reports
    auto run = [&](const std::vector<uint64_t> &blob, bool must_refuse, const std::string &what) {
        uint64_t *exact = blob.empty() ? nullptr : new uint64_t[blob.size()];
        if (!blob.empty()) memcpy(exact, blob.data(), blob.size() * 8);
        try {
            const std::vector<uint64_t> pos = gl::verify(air, opt, hash_option, seed, gl::parse_proof_blob(exact, blob.size()), required);
            if (must_refuse) { printf("FAIL: %s was accepted\n", what.c_str()); ++failures; }
            else if (pos != want) { printf("FAIL: %s was accepted with other positions\n", what.c_str()); ++failures; }
        } catch (const std::exception &e) {
            if (!*e.what()) { printf("FAIL: %s refused without a message\n", what.c_str()); ++failures; }
        }
        delete[] exact;
    };
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto draw = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    int refused = 0;
    for (size_t len = 0; len < good.size() && len < 64; ++len, ++refused) run(std::vector<uint64_t>(good.begin(), good.begin() + len), true, "the prefix of " + std::to_string(len) + " words");
    for (int k = 0; k < 64; ++k, ++refused) {
        const size_t len = (size_t)(draw() % good.size());
        run(std::vector<uint64_t>(good.begin(), good.begin() + len), true, "the prefix of " + std::to_string(len) + " words");
    }
    {   // every count word set to 2^63: walk the good blob's layout
        std::vector<size_t> counts{3};
        size_t o = 16;
        counts.push_back(o); o += 1 + 3 * good[o] + 18;
        counts.push_back(o); o += 1 + 3 * good[o];
        const uint64_t n_layers = good[3];
        for (uint64_t k = 0; k < n_layers; ++k) { counts.push_back(o + 4); o += 5; }
        const uint64_t n_openings = 2 + good[2] + n_layers;
        for (uint64_t k = 0; k < n_openings; ++k) {
            for (int j = 0; j < 3; ++j) counts.push_back(o + j);
            o += 3 + good[o] * good[o + 1] + good[o] * good[o + 2] * 4;
        }
        if (o != good.size()) { printf("FAIL: the walk of the good blob ends at %zu of %zu\n", o, good.size()); ++failures; }
        for (size_t c : counts) {
            for (uint64_t v : {(uint64_t)1 << 63, ~(uint64_t)0, good[c] + 1, good[c] - 1}) {
                std::vector<uint64_t> b = good;
                b[c] = v;
                run(b, true, "count word " + std::to_string(c) + " set to " + std::to_string(v));
                ++refused;
            }
        }
    }
    for (int k = 0; k < 256; ++k) {                          // one word garbled anywhere: refused, or never read
        std::vector<uint64_t> b = good;
        b[(size_t)(draw() % b.size())] ^= draw() | 1;
        run(b, false, "garbling " + std::to_string(k));
    }
    printf("%d malformed blobs refused, 256 garbled ones judged, %d failures\n", refused, failures);
    return failures ? 1 : 0;
}
