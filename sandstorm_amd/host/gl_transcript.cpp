// gl_transcript.cpp — see gl_transcript.hpp
#include "gl_transcript.hpp"

namespace ssh {
namespace gl {

static const uint64_t P = 0xFFFFFFFF00000001ull;
static uint64_t mulm(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % P); }
static uint64_t addm(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + b) % P); }
Fq3 mul3(const Fq3 &a, const Fq3 &b) {                     // X^3 = 2
    const uint64_t d0 = mulm(a[0], b[0]), d1 = addm(mulm(a[0], b[1]), mulm(a[1], b[0]));
    const uint64_t d2 = addm(addm(mulm(a[0], b[2]), mulm(a[1], b[1])), mulm(a[2], b[0]));
    const uint64_t d3 = addm(mulm(a[1], b[2]), mulm(a[2], b[1])), d4 = mulm(a[2], b[2]);
    return Fq3{addm(d0, addm(d3, d3)), addm(d1, addm(d4, d4)), d2};
}

// ---- SHA-256 (FIPS 180-4) for the coin's host side; the trees' SHA-256 is the device's (csrc/hash.hip)
// ---- SHA-256 (FIPS 180-4) for the coin's host side; the trees' SHA-256 is the device's (csrc/hash.hip)
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
Digest sha256(const uint8_t *msg, size_t len) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
        0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
        0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    std::vector<uint8_t> m(msg, msg + len);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(((uint64_t)len * 8) >> (8 * i)));
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[64];
        for (int t = 0; t < 16; ++t) w[t] = ((uint32_t)m[off + 4 * t] << 24) | ((uint32_t)m[off + 4 * t + 1] << 16) | ((uint32_t)m[off + 4 * t + 2] << 8) | m[off + 4 * t + 3];
        for (int t = 16; t < 64; ++t)
            w[t] = w[t - 16] + (rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 7] + (rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10));
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int t = 0; t < 64; ++t) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    Digest out;
    for (int i = 0; i < 8; ++i) { out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16); out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i]; }
    return out;
}

static void be64(std::vector<uint8_t> &b, uint64_t v) { for (int k = 7; k >= 0; --k) b.push_back((uint8_t)(v >> (8 * k))); }
Digest transcript_seed(const Digest &seed, const Options &opt, uint64_t trace_len, const Digest &statement_digest) {
    std::vector<uint8_t> b(seed.begin(), seed.end());
    for (uint64_t v : {(uint64_t)opt.num_queries, (uint64_t)opt.log_blowup, (uint64_t)opt.grinding, (uint64_t)opt.fold, (uint64_t)opt.max_remainder, trace_len}) be64(b, v);
    b.insert(b.end(), statement_digest.begin(), statement_digest.end());
    if (opt.sha256) { const char *name = "sha256"; b.insert(b.end(), name, name + 6); }
    return keccak256(b.data(), b.size());
}

}  // namespace gl
}  // namespace ssh
