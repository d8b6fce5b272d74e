// quotient_derive.h — derived columns of the generated constraint kernels (tools/gen_quotient.py derived_column_of).
//
// A value the constraint program makes from cells of ONE trace column by additions and subtractions only is a fixed integer
// combination of that column's rows:  F[i] = sum_t coef_t * column[i + (off_t << log_blowup)].  The 16 decoded flags of the
// Cairo CPU constraints are the case in point: f_j(i) = c_j(i) - 2 c_(j+1)(i) = F[i + (j << log_blowup)] with
// F = column 0 - 2 x (column 0, one row on).  The kernels read such a value as one cell of F instead of recomputing it at every
// use; the launch builds F once (csrc/quotient.hip qg_derive_column_kernel).  This header holds what the device kernel, the
// CPU build of the device code and the host tests share: the description of a derived column and the arithmetic of one row - and,
// below, the same for the alpha copies of the periodic multiplier tables.  It needs fp252.h only.
#pragma once
#include "fp252.h"

namespace ss {

static constexpr int QG_MAX_DERIVED = 2;         // derived columns per compiled program (each costs a column of scratch)
static constexpr int QG_MAX_DERIVED_TERMS = 4;   // terms per derived column (the generator's longest recipe)
struct QGenDerived {
    uint32_t col;                                // the trace column it derives from
    uint32_t n_terms;
    uint32_t off[QG_MAX_DERIVED_TERMS];          // row offsets, the smallest is 0
    int32_t coef[QG_MAX_DERIVED_TERMS];          // small non-zero integers
};

// the farthest row a derived column's terms reach
SS_HD uint32_t qg_derived_reach(const QGenDerived &d) {
    uint32_t m = 0;
    for (uint32_t t = 0; t < d.n_terms; ++t) m = d.off[t] > m ? d.off[t] : m;
    return m;
}

// k * a for a small k >= 1, by doubling and adding; canonical in, canonical out
SS_HD Fp qg_small_multiple(const Fp &a, uint32_t k) {
    Fp r = a;
    int top = 31;
    while (top > 0 && !((k >> top) & 1u)) --top;
    for (int b = top - 1; b >= 0; --b) {
        r = fp_dbl(r);
        if ((k >> b) & 1u) r = fp_add(r, a);
    }
    return r;
}

// Row k of a derived column: the fully reduced interchange image, like any trace cell.  `load(index)` reads the source column;
// the index rule is QG_TRACE_RAW's - (k + (off << log_blowup)) & trace_mask, the mask N - 1 on whole columns and all ones on a row
// block that carries the rows behind it.
template <class Load>
SS_HD Fp qg_derived_row(const QGenDerived &d, uint32_t k, uint32_t log_blowup, uint32_t trace_mask, Load load) {
    Fp r = fp_zero();
    for (uint32_t t = 0; t < d.n_terms; ++t) {
        const Fp c = load((k + (d.off[t] << log_blowup)) & trace_mask);
        const int32_t m = d.coef[t];
        r = m > 0 ? fp_add(r, qg_small_multiple(c, (uint32_t)m)) : fp_sub(r, qg_small_multiple(c, (uint32_t)(-m)));
    }
    return r;
}

// ---- ALPHA COPIES (tools/gen_quotient.py fold_alpha_tables).  A zerofier group is (sum_k alpha^k C_k) x T; where T is a multiplier-only
// periodic table the launch makes one copy of it per constraint, T'_k = alpha^k T, so that the group is sum_k C_k T'_k - terms of the
// part's running wide sum - and its reduction and its product by T are not paid at every point.  The factor is the program's
// constant in one of the limb forms the kernels' constants have (quotient_gen.h QG_CONST_R280 / _UP / _UPN).
enum { QG_ALPHA_R280 = 0, QG_ALPHA_R280_UP = 1, QG_ALPHA_R280_UPN = 2 };       // c 2^24, c 2^48, -c 2^48
struct QGenAlpha {
    uint32_t table, constant, form;
};
// what a copy's entries are multiplied by, from the constant's interchange image: an interchange image as well
SS_HD Fp qg_alpha_factor(const Fp &c, uint32_t form) {
    Fp two24 = fp_zero(); two24.v[0] = 1u << 24;
    const Fp f24 = fp_to_mont(two24);
    Fp f = fp_mul(c, f24);
    if (form != (uint32_t)QG_ALPHA_R280) f = fp_mul(f, f24);
    return form == (uint32_t)QG_ALPHA_R280_UPN ? fp_neg(f) : f;
}
// One copy: out[dst + k] = tables[src + k] x factor for k < len.  The copies of a launch lie one after the other (dst ascending,
// dst[j + 1] = dst[j] + len[j], dst[0] = 0).
struct alignas(32) QgCopy {
    uint32_t src, dst, len, pad[5];
    Fp factor;
};
// entry i of the concatenated copies (what one lane of qg_copy_tables_kernel computes): canonical, like every table entry.
// -> false if i lies in none of them
template <class Load>
SS_HD bool qg_copy_entry(const QgCopy *copies, uint32_t n, uint64_t i, Load load, Fp *out) {
    uint32_t lo = 0, hi = n;                                   // the last copy with dst <= i
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (copies[mid].dst <= i) lo = mid; else hi = mid;
    }
    if (n == 0 || i < copies[lo].dst || i - copies[lo].dst >= copies[lo].len) return false;
    *out = fp_mul(load(copies[lo].src + (uint32_t)(i - copies[lo].dst)), copies[lo].factor);
    return true;
}

}  // namespace ss
