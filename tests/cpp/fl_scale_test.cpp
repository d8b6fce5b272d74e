// Host run of fl_scale<C> (sandstorm_amd/csrc/fl252.h: the small integer multiples the generated constraint kernels take instead of
// a product by a structural constant) and of its negative, for every (C, input bound) pair tools/gen_quotient.py can emit: C = 2 .. 8
// on a lazy value of bound b (value < 2 b p, limbs < b 2^28) with C b <= 8, negated the way the generator negates - fl_sub_c<8, 2> of a
// scaled bound 2, <16, 4> of 3 or 4, a weak reduction and <2, 1> above (<2, 1> also of a bound 1).
//
// usage: fl_scale_test <input file> <output file>.  Input: u32 count, then per value 9 limbs and its bound b (u32 each).  Output, per
// value and per C = 2 .. 8 with C b <= 8: C, 9 limbs of C x, 9 limbs of -(C x), then the canonical 8 x 32-bit images of both
// (fl_to_fp).  tests/test_fl_scale_host.py holds them to Python's integers: the limb vectors EXACTLY (C x and C' p - C x as
// integers, so no limb wrapped), the documented bounds, and the images modulo p.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sandstorm_amd/csrc/fl252.h"

using namespace ss;

template <u32 C>
static void one(const Fl &x, u32 b, std::vector<u32> &out) {
    if (C * b > 8u) return;
    const Fl s = fl_scale<C>(x);
    const u32 sb = C * b;
    Fl n;
    if (sb == 1u) n = fl_sub_c<2, 1>(fl_zero(), s);
    else if (sb == 2u) n = fl_sub_c<8, 2>(fl_zero(), s);
    else if (sb <= 4u) n = fl_sub_c<16, 4>(fl_zero(), s);
    else n = fl_sub_c<2, 1>(fl_zero(), fl_weak_reduce(s));
    out.push_back(C);
    for (int i = 0; i < 9; ++i) out.push_back(s.l[i]);
    for (int i = 0; i < 9; ++i) out.push_back(n.l[i]);
    const Fp sf = fl_to_fp(s), nf = fl_to_fp(n);
    for (int i = 0; i < 8; ++i) out.push_back(sf.v[i]);
    for (int i = 0; i < 8; ++i) out.push_back(nf.v[i]);
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    u32 count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    std::vector<u32> in((size_t)count * 10), out;
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose(f);
    for (u32 k = 0; k < count; ++k) {
        Fl x;
        for (int i = 0; i < 9; ++i) x.l[i] = in[(size_t)k * 10 + i];
        const u32 b = in[(size_t)k * 10 + 9];
        one<2>(x, b, out); one<3>(x, b, out); one<4>(x, b, out); one<5>(x, b, out);
        one<6>(x, b, out); one<7>(x, b, out); one<8>(x, b, out);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    printf("FL_SCALE_DONE %u\n", count);
    return 0;
}
