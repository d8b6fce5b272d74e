// The generated constraint kernels on the CPU with their small structural multiples taken the way the DEVICE takes them
// (sandstorm_amd/csrc/quotient_gen.h): QG_SCALE / QG_RESCALE / QG_NEGSCALED as fl_scale shifts and adds and a borrow-free negation.
// quotient_gen_host_test.cpp leaves these macros undefined, and a body then falls back to the product by the table's constant (a
// harness may fill the constant table with values of its own); this one runs the shifts and adds, so the caller has to give the baked
// constants the values the kernel table lists - what csrc/capi.hip checks before it launches.  Everything else is that harness.
#include "../../sandstorm_amd/csrc/fp252.h"
#include "../../sandstorm_amd/csrc/fl252.h"

#define QG_SCALE(k, f, x) ss::fl_scale<f>(x)
#define QG_RESCALE(f, x) ss::fl_scale<f>(x)
#define QG_NEGSCALED(C, F, x) ss::fl_sub_c<C, F>(ss::fl_zero(), x)

#include "quotient_gen_host_test.cpp"
