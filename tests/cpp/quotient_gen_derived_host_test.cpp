// The generated constraint kernels on the CPU with their DERIVED COLUMNS as the device has them (test infrastructure).
// tests/cpp/quotient_gen_host_test.cpp leaves QG_DERIVED_RAW to the fallback the generated bodies carry (a cell computed from the
// real column at every read); here the macro is a read of an array that the library's own row function
// (sandstorm_amd/csrc/quotient_derive.h qg_derived_row, what csrc/quotient.hip qg_derive_column_kernel runs per lane) fills once,
// sized as csrc/capi.hip eval_quotient_compiled sizes it: N rows on the whole domain, the block's rows less the terms' reach on a
// row block.  The reads are bounds-checked, so a row the body reads and the launch would not have built ends the run.
// tests/test_quotient_gen_derived.py holds the two harnesses' outputs against each other.
//
// usage: as quotient_gen_host_test; QG_DERIVED_H (written by the test) lists the derived columns: QG_N_DERIVED, QG_DERIVED[]
#include <vector>

#include "../../sandstorm_amd/csrc/fp252.h"
#include "../../sandstorm_amd/csrc/quotient_derive.h"

static std::vector<std::vector<ss::Fp>> qg_derived_cols;
#define QG_DERIVED_RAW(d, off, idx) qg_derived_cols.at(d).at(((idx) + ((off) << lb)) & maskN)

#define main quotient_gen_host_test_main           // its operand macros, HostArgs and PARTS; main below builds the derived columns first
#include "quotient_gen_host_test.cpp"
#undef main
#include QG_DERIVED_H

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hdr[10];          // ncols, rows per column, ntables_felts, ntables, nconsts, npoints, row0, trace_mask, log_blowup, lanes
    rd(f, hdr, 10);
    HostArgs a;
    a.cols.resize(hdr[0]);
    for (auto &c : a.cols) { c.resize(hdr[1]); rd(f, c.data(), c.size()); }
    a.tables.resize(hdr[2]); rd(f, a.tables.data(), a.tables.size());
    a.tdesc.resize(2 * hdr[3]); rd(f, a.tdesc.data(), a.tdesc.size());
    std::vector<Fp> consts(hdr[4]); rd(f, consts.data(), consts.size());
    rd(f, &a.offset, 1); rd(f, &a.w, 1);
    fclose(f);
    Fp two24 = fp_zero(); two24.v[0] = 1u << 24;
    const Fp f24 = fp_to_mont(two24);
    for (auto &c : consts) {
        const Fp up = fp_mul(c, f24);
        a.consts.push_back(fl_from_fp(c)); a.consts_r280.push_back(fl_to_r280(c));
        a.consts_up.push_back(fl_to_r280(up)); a.consts_upn.push_back(fl_to_r280(fp_neg(up)));
    }
    for (uint32_t j = 0; j < QG_N_SCALED; ++j) {
        const uint32_t t = QG_SCALED_TABLES[j], first = a.tdesc[2 * t], len = a.tdesc[2 * t + 1] + 1u;
        a.tdesc.push_back((uint32_t)a.tables_scaled.size());
        a.tdesc.push_back(len - 1u);
        for (uint32_t i = 0; i < len; ++i) a.tables_scaled.push_back(fp_mul(a.tables[first + i], f24));
    }
    a.npoints = hdr[5]; a.row0 = (uint32_t)hdr[6]; a.trace_mask = (uint32_t)hdr[7]; a.log_blowup = (uint32_t)hdr[8];
    // what csrc/capi.hip eval_quotient_compiled queues in front of the first part
    const bool block = a.trace_mask == 0xffffffffu;
    for (uint32_t j = 0; j < QG_N_DERIVED; ++j) {
        const QGenDerived &d = QG_DERIVED[j];
        const uint64_t reach = (uint64_t)qg_derived_reach(d) << a.log_blowup;
        if (block && hdr[1] <= reach) { fprintf(stderr, "block shorter than the derived column's reach\n"); return 2; }
        const uint64_t rows = block ? hdr[1] - reach : hdr[1];
        const std::vector<Fp> &col = a.cols.at(d.col);
        std::vector<Fp> out(rows);
        for (uint64_t k = 0; k < rows; ++k)
            out[k] = qg_derived_row(d, (uint32_t)k, a.log_blowup, a.trace_mask, [&col](uint32_t index) { return col.at(index); });
        qg_derived_cols.push_back(out);
    }
    a.out.assign(a.npoints, fp_zero());
    a.offset = fp_mul(a.offset, fp_pow_u64(a.w, a.row0));
    const uint64_t lanes = hdr[9];
    for (part_fn part : PARTS) {
#pragma omp parallel for schedule(dynamic, 16)
        for (uint64_t lane = 0; lane < lanes; ++lane) part(a, lane, lanes);
    }
    f = fopen(argv[2], "wb");
    fwrite(a.out.data(), sizeof(Fp), a.out.size(), f);
    fclose(f);
    return 0;
}
