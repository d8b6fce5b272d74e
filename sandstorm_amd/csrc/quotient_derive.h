// quotient_derive.h — derived columns of the generated constraint kernels (tools/gen_quotient.py derived_column_of).
//
// A value the constraint program makes from cells of ONE trace column by additions and subtractions only is a fixed integer
// combination of that column's rows:  F[i] = sum_t coef_t * column[i + (off_t << log_blowup)].  The 16 decoded flags of the
// Cairo CPU constraints are the case in point: f_j(i) = c_j(i) - 2 c_(j+1)(i) = F[i + (j << log_blowup)] with
// F = column 0 - 2 x (column 0, one row on).  The kernels read such a value as one cell of F instead of recomputing it at every
// use; the launch builds F once (csrc/quotient.hip qg_derive_column_kernel).  This header holds what the device kernel, the
// CPU build of the device code and the host tests share: the description of a derived column and the arithmetic of one row.
// It needs fp252.h only.
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

}  // namespace ss
