// The generated constraint kernels on the CPU with their ALPHA COPIES as the device has them (test infrastructure).
// tests/cpp/quotient_gen_host_test.cpp leaves QG_TABLE_ALPHA_RAW to the fallback the generated bodies carry (the scaled table's entry
// times the constant's limb form, at every read); here the macro is a read of the array that the launch builds: the scaled tables and,
// behind them, one copy per (table, constant, form) of the kernel table's list, every entry made by the library's own function
// (sandstorm_amd/csrc/quotient_derive.h qg_copy_entry, what csrc/quotient.hip qg_copy_tables_kernel runs per lane) from descriptors
// laid out as csrc/capi.hip eval_quotient_compiled lays them out.  The reads are bounds-checked.
// tests/test_quotient_gen_alpha_tables_host.py holds the two harnesses' outputs against each other.
//
// usage: as quotient_gen_host_test; QG_SCALED_H (csrc/quotient_gen_<layout>_scaled.inc) also lists the copies: QG_N_ALPHA, QG_ALPHA_COPIES[]
#include <vector>

#include "../../sandstorm_amd/csrc/fp252.h"
#include "../../sandstorm_amd/csrc/quotient_derive.h"

static std::vector<uint32_t> qg_adesc;             // per alpha copy: first element in tables_scaled, index mask
#define QG_TABLE_ALPHA_RAW(j, idx) a.tables_scaled.at(qg_adesc.at(2 * (j)) + (((idx) + row0) & qg_adesc.at(2 * (j) + 1)))
#define QG_PIN_WIDE(w)

#define main quotient_gen_host_test_main           // its operand macros, HostArgs and PARTS; main below builds the copies first
#include "quotient_gen_host_test.cpp"
#undef main

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
    // what csrc/capi.hip eval_quotient_compiled stages and queues in front of the first part: one descriptor per scaled table and per
    // alpha copy, the copies one after the other in one array
    std::vector<QgCopy> copies;
    uint64_t total = 0;
    for (uint32_t j = 0; j < QG_N_SCALED + QG_N_ALPHA; ++j) {
        const bool is_alpha = j >= QG_N_SCALED;
        const uint32_t t = is_alpha ? QG_ALPHA_COPIES[j - QG_N_SCALED][0] : QG_SCALED_TABLES[j];
        const uint32_t len = a.tdesc.at(2 * t + 1) + 1u;
        QgCopy c = {};
        c.src = a.tdesc.at(2 * t); c.dst = (uint32_t)total; c.len = len;
        c.factor = is_alpha ? qg_alpha_factor(consts.at(QG_ALPHA_COPIES[j - QG_N_SCALED][1]), QG_ALPHA_COPIES[j - QG_N_SCALED][2]) : f24;
        copies.push_back(c);
        std::vector<uint32_t> &desc = is_alpha ? qg_adesc : a.tdesc;
        desc.push_back((uint32_t)total);
        desc.push_back(len - 1u);
        total += len;
    }
    a.tables_scaled.resize(total);
    const std::vector<Fp> &tables = a.tables;
    for (uint64_t i = 0; i < total; ++i)
        if (!qg_copy_entry(copies.data(), (uint32_t)copies.size(), i, [&tables](uint32_t index) { return tables.at(index); }, &a.tables_scaled[i])) {
            fprintf(stderr, "entry %llu lies in no copy\n", (unsigned long long)i);
            return 2;
        }
    a.npoints = hdr[5]; a.row0 = (uint32_t)hdr[6]; a.trace_mask = (uint32_t)hdr[7]; a.log_blowup = (uint32_t)hdr[8];
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
