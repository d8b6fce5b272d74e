// Field elements for the host tests of the 252-bit arithmetic: the edge values of [0, p) (p = 2^251 + 17 2^192 + 1) and uniform
// draws from the WHOLE of [0, p) (rejection, not masking: a draw masked below 2^251 never has bit 251 set, and [2^251, p) is where
// the limb form's top limb holds a quotient bit).  The same list as tests/edge_values.py.
#pragma once
#include <cstdint>
#include "../../sandstorm_amd/csrc/fp252.h"

namespace edge_fp {

static const ss::Fp EDGE[] = {
    {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},   // 0
    {{0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},   // 1
    {{0x00000002u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u}},   // 2
    {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000011u, 0x08000000u}},   // p - 1
    {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000010u, 0x08000000u}},   // p - 2
    {{0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000010u, 0x08000000u}},   // p - 3
    {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x07ffffffu}},   // 2^251 - 1
    {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x08000000u}},   // 2^251
    {{0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x08000000u}},   // 2^251 + 1
    {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0x08000000u}},   // 2^251 + 2^192
    {{0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x80000000u, 0x00000008u, 0x04000000u}},   // (p - 1) / 2
    {{0x00000001u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x80000000u, 0x00000008u, 0x04000000u}},   // (p + 1) / 2
    {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000000u}},   // 2^192 - 1
    {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u}},   // 2^224 - 1
    {{0xffffffe1u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffdf0u, 0x07ffffffu}},   // Montgomery 1
    {{0x00000020u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000220u, 0x00000000u}},   // Montgomery -1
    {{0xffffffc1u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xfffffbd0u, 0x07ffffffu}},   // Montgomery 2
    {{0x00000040u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000440u, 0x00000000u}},   // Montgomery -2
    {{0xe0000001u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xe0000010u, 0x07fffffdu}},   // R280 1
    {{0x20000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x20000000u, 0x00000002u}},   // R280 -1
};
static constexpr int N_EDGE = (int)(sizeof(EDGE) / sizeof(EDGE[0]));

// a < p (word-wise compare from the top; p's words: 1, 0 x 5, SS_P6, SS_P7)
inline bool below_p(const ss::Fp &a) {
    const uint32_t pw[8] = {SS_P0, 0, 0, 0, 0, 0, SS_P6, SS_P7};
    for (int i = 7; i >= 0; --i)
        if (a.v[i] != pw[i]) return a.v[i] < pw[i];
    return false;
}

// uniform on [0, p): 252-bit draws, the ones >= p drawn again.  next(): any source of 64 random bits
template <class Next>
ss::Fp uniform(Next &&next) {
    for (;;) {
        ss::Fp a;
        for (int i = 0; i < 8; i += 2) { const uint64_t r = next(); a.v[i] = (uint32_t)r; a.v[i + 1] = (uint32_t)(r >> 32); }
        a.v[7] &= 0x0fffffffu;
        if (below_p(a)) return a;
    }
}

// in [2^251, p)
template <class Next>
ss::Fp top(Next &&next) {
    ss::Fp a = uniform(next);
    a.v[7] = SS_P7;
    a.v[6] = (uint32_t)(next() % SS_P6);
    return a;
}

// draw i of a test: the edge list first, then an edge value, a value of [2^251, p) or a uniform one
template <class Next>
ss::Fp draw(Next &&next, long i) {
    if (i < N_EDGE) return EDGE[i];
    const uint64_t k = next() % 8;
    if (k < 2) return EDGE[next() % N_EDGE];
    if (k < 3) return top(next);
    return uniform(next);
}

}  // namespace edge_fp
