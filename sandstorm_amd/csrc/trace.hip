// trace.hip — the BASE trace made on the device ("next" row X1).
//
// ExecutionTrace::new (layouts/src/starknet/trace.rs:99-987, layouts/src/recursive/trace.rs:89-688,
// layouts/src/utils.rs:112-152) turns ~25 MB of `cairo-run` output (trace.bin: (ap, fp, pc) per cycle; memory.bin:
// (address, word) records) into 7 / 9 columns of 16 rows per cycle - 3.6 / 4.8 GB at 2^20 steps.  The reference makes them
// with rayon loops and sequential sorts on the host; this repo's host generator (host/trace_*.cpp) does the same, and a
// files -> proof call was then bound by the PCIe uploads of cells that are functions of the 25 MB.  Here the cells are made
// where they are used:
//   trace_cpu_kernel      one lane per Cairo cycle decodes the instruction, reads its three operands from the memory image,
//                         computes res / tmp0 / tmp1 / op0*op1 (trace.rs:177-244) into LDS; the workgroup then writes the
//                         cycle's 16 rows of the flags, memory-pool, range-check and auxiliary columns row by row
//                         (consecutive lanes = consecutive rows: whole 2 KiB runs per wave) and the pool's addresses as
//                         integers for the sort-free ordered memory below
//   trace_tile_kernel     a builtin's instances: ONE template of cells per distinct instance (the dummy instance: one for
//                         the whole run), written into every block that holds it; address cells are affine in the block
//   trace_pedersen_*      the GIVEN Pedersen instances from their two inputs (72 bytes each instead of a 66 KB template): the
//                         partial sums as one chain of Jacobian additions with one inversion per instance, then one lane per row
//   trace_bitwise_kernel  the GIVEN bitwise instances from x, y (72 bytes each): one lane per written cell - 64 diluted parts, four shifted
//                         top segments, five memory-pool pairs
//   trace_poseidon_kernel the GIVEN Poseidon instances from their three inputs (104 bytes each): one lane per instance walks the 91
//                         rounds and stores every S-box input with its square (the S-box's own intermediate)
//   trace_ec_op_kernel    the GIVEN EC-op instances from P, Q, m (168 bytes each): one wave per instance - the doubling chain and the
//                         multiply-add chain in Jacobian coordinates on one lane, then four steps a lane with one inversion each
//   trace_ecdsa_kernel    the GIVEN ECDSA instances from the key, the message, r and w (168 bytes each): one wave per instance - three
//                         multiply-add chains and two doubling chains of the EC-op kernel's, run for the key's other root when the first fails
//   trace_rc_*            the range-check builtin's parts and the pool's ordered values / padding (utils.rs:357-380):
//                         runs located by binary search in a prefix array of the 65536-bin histogram
//   trace_runs_kernel     the diluted pool's ordered column the same way
//   trace_patch_kernel    the few cells that are neither (the diluted pool's padding values)
//   mem_*                 get_ordered_memory_accesses (utils.rs:112-152) without a sort: count per address through an LDS
//                         table per workgroup (an idling run reads the same handful of cells a million times), gaps by a
//                         flag scan, a prefix sum over the counts, rows by binary search in it; the reference's checks
//                         (continuous, single-valued, public memory = the address-0 cells) as error bits in a status word
//   trace_gl64_* / mem_*_gl64   the plain layout over the 64-bit field (layouts/src/plain/trace.rs:60-262): the same pipeline over one-word
//                         cells, canonical (not Montgomery), with that layout's placement; the counting half of the ordered memory -
//                         u32 addresses, no field - is the kernels above, launched as they are
// HBM-write bound: ~5 GB written once.  No floating point, no MFMA: integer decode and a handful of modular products per cell.
#include <hip/hip_runtime.h>
#include "inv252.h"
#include "gl64.h"
#include "kernels.h"

namespace ss {

namespace {

__device__ __forceinline__ Fp load_fp(const Fp *p) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    const uint4 a = q[0], b = q[1];
    Fp r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
__device__ __forceinline__ void store_fp(Fp *p, const Fp &x) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    q[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}
__device__ __forceinline__ Fp fp_of_words(const u64 w[4]) {          // a 256-bit integer, not yet in Montgomery form
    Fp r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { r.v[2 * i] = (u32)w[i]; r.v[2 * i + 1] = (u32)(w[i] >> 32); }
    return r;
}
__device__ __forceinline__ u32 sat32(u64 a) { return a > 0xffffffffull ? 0xffffffffu : (u32)a; }
__device__ __forceinline__ void status_error(u32 *status, u32 bits, u64 where) {
    atomicOr(&status[TRACE_ST_ERRORS], bits);
    atomicMax(&status[TRACE_ST_WHERE], ~sat32(where));              // the SMALLEST cycle / address that failed, as its complement
}

// ------------------------------------------------------------------------------------------------ memory image
// memory.bin: records of (u64 address, 32-byte little-endian word) -> image[address] (4 x u64); a cell no record names keeps
// the fill (all ones: not a field element, binary/src/lib.rs reads values < p)
__global__ __launch_bounds__(256) void trace_memory_image_kernel(const u64 *__restrict__ records, u64 n_records, u64 *__restrict__ image, u64 cells) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_records) return;
    const u64 a = records[5 * k];
    if (a >= cells) return;                                          // beyond every address a continuous memory of this trace can hold
#pragma unroll
    for (int i = 0; i < 4; ++i) image[4 * a + i] = records[5 * k + 1 + i];
}

// ------------------------------------------------------------------------------------------------ the CPU's cells
constexpr int CPU_CYC = 128;                 // cycles (and lanes) per workgroup
struct CpuRec {
    u64 word, ap, fp;
    u32 addr[4];                             // pc, op0, dst, op1 (saturated at 2^32 - 1: such an address fails the memory checks)
    u32 jnz, pad;
    Fp val[4];                               // the instruction word, op0, dst, op1 as Montgomery felts
    Fp res, tmp1, mul;
};
enum { REC_PC = 0, REC_OP0 = 1, REC_DST = 2, REC_OP1 = 3 };

__device__ __forceinline__ bool image_cell(const u64 *image, u64 cells, u64 a, u64 w[4]) {
    if (a >= cells) { w[0] = w[1] = w[2] = w[3] = 0; return false; }
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = image[4 * a + i];
    if (w[3] == ~0ull) { w[0] = w[1] = w[2] = w[3] = 0; return false; }
    return true;
}

__global__ __launch_bounds__(CPU_CYC) void trace_cpu_kernel(TraceLayout L, const u64 *__restrict__ states, u64 num_cycles, const u64 *__restrict__ image,
                                                            u64 cells, Fp pad_value, Fp rc_fill, Fp *__restrict__ flags, Fp *__restrict__ npc,
                                                            Fp *__restrict__ rc, Fp *__restrict__ aux, u32 *__restrict__ pool_addr, u32 *status) {
    __shared__ CpuRec rec[CPU_CYC];
    __shared__ uint8_t tab[48];              // the layout's placement tables (indexed per lane: LDS, not the kernel arguments)
    const u32 t = threadIdx.x;
    if (t < 8) tab[t] = L.npc_pair[t];
    if (t < 16) { tab[16 + t] = L.rc_cell[t]; tab[32 + t] = L.aux_cell[t]; }
    const u64 cyc0 = (u64)blockIdx.x * CPU_CYC, cyc = cyc0 + t;
    if (cyc < num_cycles) {
        CpuRec &r = rec[t];
        const u64 ap = states[3 * cyc], fp = states[3 * cyc + 1], pc = states[3 * cyc + 2];
        u32 err = 0;
        u64 iw[4], w0[4], wd[4], w1[4];
        if (!image_cell(image, cells, pc, iw)) err |= TRACE_ERR_MISSING_CELL;
        const u64 w = iw[0];
        if ((iw[1] | iw[2] | iw[3]) || (w >> 63)) err |= TRACE_ERR_NOT_INSTRUCTION;
        auto flag = [&](int f) { return (u32)((w >> (48 + f)) & 1); };
        const u64 dst_addr = (w & 0xffff) + (flag(0) ? fp : ap) - 0x8000, op0_addr = ((w >> 16) & 0xffff) + (flag(1) ? fp : ap) - 0x8000;
        if (!image_cell(image, cells, op0_addr, w0)) err |= TRACE_ERR_MISSING_CELL;
        if (!image_cell(image, cells, dst_addr, wd)) err |= TRACE_ERR_MISSING_CELL;
        const u32 src = flag(2) + 2 * flag(3) + 4 * flag(4);
        u64 base = 0;
        if (src == 0) { if (w0[1] | w0[2] | w0[3]) err |= TRACE_ERR_NOT_AN_ADDRESS; base = w0[0]; }
        else if (src == 1) base = pc;
        else if (src == 2) base = fp;
        else if (src == 4) base = ap;
        else err |= TRACE_ERR_BAD_OP1_SOURCE;
        const u64 op1_addr = ((w >> 32) & 0xffff) + base - 0x8000;
        if (!image_cell(image, cells, op1_addr, w1)) err |= TRACE_ERR_MISSING_CELL;
        const Fp inst = fp_to_mont(fp_of_words(iw)), op0 = fp_to_mont(fp_of_words(w0)), dst = fp_to_mont(fp_of_words(wd)), op1 = fp_to_mont(fp_of_words(w1));
        const u32 pc_update = flag(7) + 2 * flag(8) + 4 * flag(9), res_logic = flag(5) + 2 * flag(6);
        Fp res = fp_zero();
        if (pc_update == 4) { if (!fp_is_zero(dst)) res = fp_inv_safegcd(dst); }        // get_res of a conditional jump: dst^-1
        else if (res_logic == 0) res = op1;
        else if (res_logic == 1) res = fp_add(op0, op1);
        else if (res_logic == 2) res = fp_mul(op0, op1);
        else err |= TRACE_ERR_BAD_RES_LOGIC;
        r.word = w; r.ap = ap; r.fp = fp;
        r.addr[REC_PC] = sat32(pc); r.addr[REC_OP0] = sat32(op0_addr); r.addr[REC_DST] = sat32(dst_addr); r.addr[REC_OP1] = sat32(op1_addr);
        r.jnz = flag(9);
        r.val[REC_PC] = inst; r.val[REC_OP0] = op0; r.val[REC_DST] = dst; r.val[REC_OP1] = op1;
        r.res = res; r.tmp1 = r.jnz ? fp_mul(dst, res) : fp_zero(); r.mul = fp_mul(op0, op1);
        if (err) status_error(status, err, cyc);
    }
    __syncthreads();
    const u64 live = num_cycles - cyc0 < CPU_CYC ? num_cycles - cyc0 : CPU_CYC;       // cycles of this workgroup
    const u64 row0 = cyc0 * 16;
    for (u32 it = 0; it < 16; ++it) {
        const u32 lr = it * CPU_CYC + t, c = lr >> 4, o = lr & 15;
        if (c >= live) break;
        const CpuRec &r = rec[c];
        // flags: the instruction word's bits from bit o upwards (Flag::*.curr(): binary/src/lib.rs:740-772; bit 15 is zero)
        store_fp(&flags[row0 + lr], fp_from_u64(o == 15 ? 0 : (r.word >> (48 + o)) & ((1ull << (15 - o)) - 1)));
        // range-check column: the fill, the instruction's three offsets, zeros where the layout has other cells (the pool's cells
        // come with trace_rc_pool_kernel)
        {
            const u32 kind = tab[16 + o];
            Fp v = rc_fill;
            if (kind == TRACE_RC_ZERO) v = fp_zero();
            else if (kind != TRACE_RC_FILL) v = fp_from_u64((r.word >> (kind == TRACE_RC_OFF_DST ? 0 : kind == TRACE_RC_OFF_OP0 ? 16 : 32)) & 0xffff);
            store_fp(&rc[row0 + lr], v);
        }
        // auxiliary column
        {
            const u32 kind = tab[32 + o];
            Fp v = fp_zero();
            if (kind == TRACE_AUX_AP || kind == TRACE_AUX_FP) v = fp_from_u64(kind == TRACE_AUX_AP ? r.ap : r.fp);
            else if (kind == TRACE_AUX_TMP0) { if (r.jnz) v = r.val[REC_DST]; }
            else if (kind == TRACE_AUX_TMP1) v = r.tmp1;
            else if (kind == TRACE_AUX_MUL) v = r.mul;
            else if (kind == TRACE_AUX_RES) v = r.res;
            store_fp(&aux[row0 + lr], v);
        }
        // memory pool: (address, value) pairs - the CPU's four accesses, the public memory's (0, 0) slots, the padding pair elsewhere
        {
            const u32 kind = tab[o >> 1];
            Fp v;
            if (kind == TRACE_NPC_PAD) v = (o & 1) ? pad_value : fp_one();
            else if (kind == TRACE_NPC_PUBLIC) v = fp_zero();
            else v = (o & 1) ? r.val[kind - TRACE_NPC_PC] : fp_from_u64(r.addr[kind - TRACE_NPC_PC]);
            store_fp(&npc[row0 + lr], v);
        }
    }
    for (u32 it = 0; it < 8; ++it) {
        const u32 lp = it * CPU_CYC + t, c = lp >> 3, j = lp & 7;
        if (c >= live) break;
        const u32 kind = tab[j];
        pool_addr[cyc0 * 8 + lp] = kind == TRACE_NPC_PAD ? 1u : kind == TRACE_NPC_PUBLIC ? 0u : rec[c].addr[kind - TRACE_NPC_PC];
    }
}

// ------------------------------------------------------------------------------------------------ builtin instances
// entry e of a builtin's template: column, row offset inside the instance's block, kind (a value of the template, or the felt of
// the address addr_begin + addr_mult * block + arg); thread g writes entry g % n_e of block g / n_e
__global__ __launch_bounds__(256) void trace_tile_kernel(ColPtrs cols, u32 ncols, const TraceTileEntry *__restrict__ entries, u32 n_e, const Fp *__restrict__ values,
                                                         u32 n_templates, const u32 *__restrict__ tmpl_of_block, u64 nblocks, u64 step, u64 addr_begin,
                                                         u64 addr_mult, u32 *__restrict__ pool_addr) {
    __shared__ Fp *col_ptr[MAX_COLS];
    if (threadIdx.x < MAX_COLS) col_ptr[threadIdx.x] = (Fp *)cols.dst[threadIdx.x];
    __syncthreads();
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= nblocks * n_e) return;
    u64 i; u32 e;
    if (nblocks * n_e <= 0xffffffffull) { i = (u32)g / n_e; e = (u32)g - (u32)i * n_e; } else { i = g / n_e; e = (u32)(g - i * n_e); }
    const TraceTileEntry en = entries[e];
    if (en.col >= ncols || en.off >= step) return;                   // (the table is the caller's device memory: never write outside a column)
    const u64 row = i * step + en.off;
    Fp v;
    if (en.kind == TRACE_TILE_ADDRESS) {
        const u64 a = addr_begin + addr_mult * i + en.arg;
        v = fp_from_u64(a);
        pool_addr[row >> 1] = sat32(a);
    } else {
        const u32 tm = tmpl_of_block ? tmpl_of_block[i] : 0;
        if (tm >= n_templates) return;
        v = load_fp(&values[(u64)tm * n_e + e]);
    }
    store_fp(&col_ptr[en.col][row], v);
}

// ------------------------------------------------------------------------------------------------ Pedersen instances from their inputs
// A GIVEN Pedersen instance (index, a, b: 9 u64) -> the cells the host generator's Pedersen section writes for it
// (host/trace_common.hpp element_steps): the 512 partial sums P0 + sum of the constant points of the set bits, the suffixes
// input >> j, the slopes of the additions, the flag cells and the three memory-pool pairs.  Two kernels:
//   trace_pedersen_sums_kernel   one lane per instance walks the set bits of a, then b, as ONE chain of Jacobian mixed additions
//                                and parks (X3, Y3, H, R) of every addition in the four cells of ITS OWN row (x, y, suffix, slope of
//                                step j: the instance's cells are the scratch).  Z3 = Z1 H, so the Z's are the prefix products of
//                                the H's: ONE inversion of the last Z and a walk back (1 / Z_{k-1} = H_k / Z_k) turn every row into
//                                the affine sum AFTER step j and the slope R / Z3 of step j.
//   trace_pedersen_rows_kernel   one workgroup per instance, one lane per step: reads the sum BEFORE its step (the row of the last set
//                                bit below it, or P0) and its own slope, barrier, writes its row - x, y, suffix, slope - then the flag
//                                cells and the pool pairs (the last writes of the section, as on the host).
// The exceptional case - a partial sum that meets its constant point (H = 0) - sets TRACE_ERR_PEDERSEN_INFINITY and leaves the
// generation refused: the rows kernel does not touch that instance (its step-511 suffix cell keeps the all-ones mark, no field element); an instance whose index is beyond the blocks or whose input has a bit from 252 up (not a field element) is
// skipped with TRACE_ERR_PEDERSEN_INSTANCE: nothing is written outside the columns.
constexpr u32 PED_STEPS = 512, PED_INPUT_BITS = 252;
struct PedCells { Fp *x, *y, *suffix, *slope; u64 stride; };
__device__ __forceinline__ PedCells ped_cells(const ColPtrs &cols, const TracePedersenLayout &L, u64 base) {
    PedCells c;
    c.x = (Fp *)cols.dst[L.col_x] + base + L.off_x; c.y = (Fp *)cols.dst[L.col_y] + base + L.off_y;
    c.suffix = (Fp *)cols.dst[L.col_suffix] + base + L.off_suffix; c.slope = (Fp *)cols.dst[L.col_slope] + base + L.off_slope;
    c.stride = L.row_stride;
    return c;
}
__device__ __forceinline__ bool ped_instance_ok(const u64 *rec, u64 n_blocks) { return rec[0] < n_blocks && !(rec[4] >> 60) && !(rec[8] >> 60); }

__global__ __launch_bounds__(64) void trace_pedersen_sums_kernel(ColPtrs cols, TracePedersenLayout L, const u64 *__restrict__ inst, u64 n_given, u64 n_blocks,
                                                                 u64 block_rows, const Fp *__restrict__ points, u32 *status) {
    const u64 g = (u64)blockIdx.x * 64 + threadIdx.x;
    if (g >= n_given) return;
    const u64 *rec = inst + 9 * g;                                   // (the words are read where they are used: no indexed private array)
    if (!ped_instance_ok(rec, n_blocks)) { status_error(status, TRACE_ERR_PEDERSEN_INSTANCE, g); return; }
    const u64 index = rec[0];
    const PedCells c = ped_cells(cols, L, index * block_rows);
    // the suffix cell of step 511 (bit 255 of b: never set, so never scratch) says whether the chain came through: all ones - no field
    // element - from here until the walk back is done; the rows kernel leaves an instance alone whose mark is still there
    Fp *const mark = &c.suffix[(u64)(PED_STEPS - 1) * c.stride];
    Fp unfinished;
#pragma unroll
    for (int k = 0; k < 8; ++k) unfinished.v[k] = 0xffffffffu;
    store_fp(mark, unfinished);
    Fp X = load_fp(&points[0]), Y = load_fp(&points[1]), Z = fp_one();
    bool any = false;
    for (u32 wi = 0; wi < 8; ++wi) {                                 // the words of a, then of b, bits ascending
        u64 bits = rec[1 + wi];
        const u32 e = wi >> 2, bit0 = (wi & 3) * 64;
        while (bits) {
            const u64 low = bits & (~bits + 1);
            bits ^= low;
            const u32 i = bit0 + 63 - (u32)__clzll((long long)low);
            const Fp *q = &points[2 * (1 + PED_INPUT_BITS * e + i)];
            const Fp zz = fp_sqr(Z);
            const Fp h = fp_sub(fp_mul(load_fp(q), zz), X), r = fp_sub(fp_mul(load_fp(q + 1), fp_mul(Z, zz)), Y);
            if (fp_is_zero(h)) { status_error(status, TRACE_ERR_PEDERSEN_INFINITY, index); return; }
            const Fp hh = fp_sqr(h), hhh = fp_mul(h, hh), v = fp_mul(X, hh);
            const Fp x3 = fp_sub(fp_sub(fp_sqr(r), hhh), fp_dbl(v));
            Y = fp_sub(fp_mul(r, fp_sub(v, x3)), fp_mul(Y, hhh));
            X = x3;
            Z = fp_mul(Z, h);
            const u64 row = (u64)(256 * e + i) * c.stride;
            store_fp(&c.x[row], X); store_fp(&c.y[row], Y); store_fp(&c.suffix[row], h); store_fp(&c.slope[row], r);
            any = true;
        }
    }
    if (!any) { store_fp(mark, fp_zero()); return; }
    Fp zinv = fp_inv_safegcd(Z);                                     // no H was zero: Z is not
    for (u32 wk = 8; wk-- > 0;) {                                    // the same bits, descending
        u64 bits = rec[1 + wk];
        const u32 e = wk >> 2, bit0 = (wk & 3) * 64;
        while (bits) {
            const u32 b = 63 - (u32)__clzll((long long)bits);
            bits ^= 1ull << b;
            const u64 row = (u64)(256 * e + bit0 + b) * c.stride;
            const Fp zi2 = fp_sqr(zinv);
            store_fp(&c.x[row], fp_mul(load_fp(&c.x[row]), zi2));
            store_fp(&c.y[row], fp_mul(load_fp(&c.y[row]), fp_mul(zi2, zinv)));
            store_fp(&c.slope[row], fp_mul(load_fp(&c.slope[row]), zinv));
            zinv = fp_mul(zinv, load_fp(&c.suffix[row]));
        }
    }
    store_fp(mark, fp_zero());
}

// the highest set bit below position `limit` (<= 512) of the chain a (bits 0 .. 255), b (256 .. 511); -1: none
__device__ __forceinline__ int ped_last_set_below(const u64 *words /* 8 */, u32 limit) {
    for (u32 wk = 8; wk-- > 0;) {
        if (64 * wk >= limit) continue;
        u64 m = words[wk];
        if (limit - 64 * wk < 64) m &= (1ull << (limit - 64 * wk)) - 1;
        if (m) return (int)(64 * wk + 63 - (u32)__clzll((long long)m));
    }
    return -1;
}
__device__ __forceinline__ void ped_pool_pair(Fp *pool, u32 *pool_addr, u64 row, u64 addr, const Fp &value) {
    store_fp(&pool[row], fp_from_u64(addr));
    store_fp(&pool[row + 1], value);
    pool_addr[row >> 1] = sat32(addr);
}
__global__ __launch_bounds__(PED_STEPS) void trace_pedersen_rows_kernel(ColPtrs cols, TracePedersenLayout L, const u64 *__restrict__ inst, u64 n_blocks, u64 block_rows,
                                                                        u64 addr_begin, const Fp *__restrict__ points, u32 *__restrict__ pool_addr) {
    __shared__ u64 rec[9];
    const u32 t = threadIdx.x;
    if (t < 9) rec[t] = inst[9 * (u64)blockIdx.x + t];
    __syncthreads();
    if (!ped_instance_ok(rec, n_blocks)) return;                     // (flagged by the sums kernel; the whole workgroup leaves)
    const u64 base = rec[0] * block_rows;
    const PedCells c = ped_cells(cols, L, base);
    const u64 *words = rec + 1;
    {                                                                // the sums kernel's mark (every lane reads the same cell: the whole workgroup leaves)
        const Fp m = load_fp(&c.suffix[(u64)(PED_STEPS - 1) * c.stride]);
        if ((m.v[0] & m.v[7]) == 0xffffffffu) return;                // the chain met its constant point: the cells stay unfinished, the mark with them
    }
    const u32 e = t >> 8, i = t & 255;
    const int before = ped_last_set_below(words, t);
    const Fp x = before < 0 ? load_fp(&points[0]) : load_fp(&c.x[(u64)before * c.stride]);
    const Fp y = before < 0 ? load_fp(&points[1]) : load_fp(&c.y[(u64)before * c.stride]);
    const bool set = (words[4 * e + (i >> 6)] >> (i & 63)) & 1;
    const Fp slope = set ? load_fp(&c.slope[(u64)t * c.stride]) : fp_zero();
    Fp out = fp_zero();                                              // the sum after the last step: the hash (lane 511 keeps it)
    if (t == PED_STEPS - 1) { const int last = ped_last_set_below(words, PED_STEPS); out = last < 0 ? load_fp(&points[0]) : load_fp(&c.x[(u64)last * c.stride]); }
    u64 sfx[4];                                                      // input e >> i
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 w = k + (i >> 6), sh = i & 63;
        u64 v = w < 4 ? words[4 * e + w] >> sh : 0;
        if (sh && w + 1 < 4) v |= words[4 * e + w + 1] << (64 - sh);
        sfx[k] = v;
    }
    const Fp suffix = fp_to_mont(fp_of_words(sfx));
    __syncthreads();
    const u64 row = (u64)t * c.stride;
    store_fp(&c.x[row], x); store_fp(&c.y[row], y); store_fp(&c.suffix[row], suffix); store_fp(&c.slope[row], slope);
    __syncthreads();
    // the flag cells (they overwrite what the steps wrote there) and the pool's pairs
    if (t < 2) {
        const u64 top = words[4 * t + 3];                            // bits 192 ..: bit 251 = 59, 196 = 4, 192 = 0
        const bool f2 = ((top >> 59) & 1) && ((top >> 4) & 1), f3 = f2 && (top & 1);
        const u64 second = (u64)t * 256 * c.stride;
        store_fp((Fp *)cols.dst[L.col_flag2] + base + L.off_flag2 + second, fp_from_u64(f2));
        store_fp((Fp *)cols.dst[L.col_flag3] + base + L.off_flag3 + second, fp_from_u64(f3));
    }
    Fp *pool = (Fp *)cols.dst[L.col_pool];
    const u64 addr0 = addr_begin + 3 * rec[0];
    if (t == 2 || t == 3) ped_pool_pair(pool, pool_addr, base + (t == 2 ? L.off_input0 : L.off_input1), addr0 + (t - 2), fp_to_mont(fp_of_words(words + 4 * (t - 2))));
    if (t == PED_STEPS - 1) ped_pool_pair(pool, pool_addr, base + L.off_output, addr0 + 2, out);
}

// ------------------------------------------------------------------------------------------------ bitwise instances from their inputs
// A GIVEN bitwise instance (index, x, y: 9 u64) -> the cells the host generator's bitwise section writes for it (host/device_trace.hpp
// bitwise_instance_trace; builtins/src/bitwise/mod.rs:23-133): for each of x, y, x & y, x ^ y the 4 x 4 parts (word c, bits 4 b + sg
// moved to 4 b: already diluted), the four top segments of x & y + x ^ y shifted by 4, 4, 4, 8, and the pool pairs of x, y, x & y,
// x ^ y, x | y.  BW_LANES lanes per instance, one per written cell or pair: an instance's stores go out side by side.  An instance whose
// index is beyond the blocks or whose input has a bit from 252 up is skipped with TRACE_ERR_BITWISE_INSTANCE.  (Bit 251 of x | y does
// not fit the last shifted cell: the host generator refuses such an instance and host/device_trace.hpp refuses it before the upload;
// here the cell would get the bits that fit.)
constexpr u32 BW_LANES = 80;                 // 64 parts, 4 shifted cells, 5 pairs, 7 idle
constexpr u64 BW_DILUTED = 0x1111111111111111ull;
__global__ __launch_bounds__(256) void trace_bitwise_kernel(ColPtrs cols, TraceBitwiseLayout L, const u64 *__restrict__ inst, u64 n_given, u64 n_blocks, u64 block_rows,
                                                            u64 addr_begin, u32 what, u32 *__restrict__ pool_addr, u32 *status) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 i = g / BW_LANES;
    const u32 t = (u32)(g - i * BW_LANES);
    if (i >= n_given) return;
    const u64 *rec = inst + 9 * i;
    const u64 index = rec[0];
    if (index >= n_blocks || (rec[4] >> 60) || (rec[8] >> 60)) { if (t == 0) status_error(status, TRACE_ERR_BITWISE_INSTANCE, i); return; }
    const u64 base = index * block_rows;
    auto word = [&](u32 p, u32 c) {          // word c of x, y, x & y, x ^ y, x | y
        const u64 x = rec[1 + c], y = rec[5 + c];
        return p == 0 ? x : p == 1 ? y : p == 2 ? (x & y) : p == 3 ? (x ^ y) : (x | y);
    };
    if (t < 64) {
        if (!(what & TRACE_BITWISE_CELLS)) return;
        const u32 p = t >> 4, c = (t >> 2) & 3, sg = t & 3;
        store_fp((Fp *)cols.dst[L.col_diluted] + base + L.off_part + L.stride_p * p + L.stride_c * c + L.stride_s * sg, fp_from_u64((word(p, c) >> sg) & BW_DILUTED));
    } else if (t < 68) {
        if (!(what & TRACE_BITWISE_CELLS)) return;
        const u32 k = t - 64;
        const u64 v = ((word(2, 3) >> k) & BW_DILUTED) + ((word(3, 3) >> k) & BW_DILUTED);
        const u32 off = k == 0 ? L.off_shifted[0] : k == 1 ? L.off_shifted[1] : k == 2 ? L.off_shifted[2] : L.off_shifted[3];      // (selects: no lane-indexed kernel argument)
        store_fp((Fp *)cols.dst[L.col_diluted] + base + off, fp_from_u64(v << (k == 3 ? 8 : 4)));
    } else if (t < 73) {
        if (!(what & TRACE_BITWISE_PAIRS)) return;
        const u32 k = t - 68;
        u64 w[4];
#pragma unroll
        for (u32 c = 0; c < 4; ++c) w[c] = word(k, c);
        const u32 off = k == 0 ? L.off_pair[0] : k == 1 ? L.off_pair[1] : k == 2 ? L.off_pair[2] : k == 3 ? L.off_pair[3] : L.off_pair[4];
        ped_pool_pair((Fp *)cols.dst[L.col_pool], pool_addr, base + off, addr_begin + 5 * index + k, fp_to_mont(fp_of_words(w)));
    }
}

// ------------------------------------------------------------------------------------------------ Poseidon instances from their inputs
// A GIVEN Poseidon instance (index, three inputs: 13 u64) -> the cells the host generator's Poseidon section writes for it
// (host/trace_starknet.cpp poseidon_trace; builtins/src/poseidon/mod.rs:45-152): the state of each of the 8 full rounds after the key
// addition with its squares, the third element of each of the 83 partial rounds with its square, the three outputs; the pool pairs
// of inputs and outputs.  One lane per instance: a dependent chain of 107 S-boxes, v^3 = v^2 v with v^2 the stored cell - 214
// products an instance, nothing computed twice.  Skipped with TRACE_ERR_POSEIDON_INSTANCE: an index beyond the blocks, an input with a
// bit from 252 up.
struct PoseidonState { Fp a, b, c; };
__device__ __forceinline__ PoseidonState poseidon_mix(const PoseidonState &s) {      // (3 a + b + c, a - b + c, a + b - 2 c)
    PoseidonState r;
    r.a = fp_add(fp_add(fp_add(fp_add(s.a, s.a), s.a), s.b), s.c);
    r.b = fp_add(fp_sub(s.a, s.b), s.c);
    r.c = fp_sub(fp_add(s.a, s.b), fp_add(s.c, s.c));
    return r;
}
__global__ __launch_bounds__(64) void trace_poseidon_kernel(ColPtrs cols, TracePoseidonLayout L, const Fp *__restrict__ keys, const u64 *__restrict__ inst, u64 n_given,
                                                            u64 n_blocks, u64 block_rows, u64 addr_begin, u32 *__restrict__ pool_addr, u32 *status) {
    const u64 g = (u64)blockIdx.x * 64 + threadIdx.x;
    if (g >= n_given) return;
    const u64 *rec = inst + 13 * g;
    const u64 index = rec[0];
    if (index >= n_blocks || (rec[4] >> 60) || (rec[8] >> 60) || (rec[12] >> 60)) { status_error(status, TRACE_ERR_POSEIDON_INSTANCE, g); return; }
    const u64 base = index * block_rows, addr0 = addr_begin + 6 * index;
    Fp *const full = (Fp *)cols.dst[L.col_full] + base, *const partial = (Fp *)cols.dst[L.col_partial] + base, *const tail = (Fp *)cols.dst[L.col_tail] + base;
    Fp *const pool = (Fp *)cols.dst[L.col_pool];
    PoseidonState s;
    s.a = fp_to_mont(fp_of_words(rec + 1)); s.b = fp_to_mont(fp_of_words(rec + 5)); s.c = fp_to_mont(fp_of_words(rec + 9));
    ped_pool_pair(pool, pool_addr, base + L.off_pair[0], addr0, s.a);
    ped_pool_pair(pool, pool_addr, base + L.off_pair[1], addr0 + 1, s.b);
    ped_pool_pair(pool, pool_addr, base + L.off_pair[2], addr0 + 2, s.c);
    u32 r = 0;
    auto full_round = [&](u32 rnd) {
        s.a = fp_add(s.a, load_fp(&keys[3 * r])); s.b = fp_add(s.b, load_fp(&keys[3 * r + 1])); s.c = fp_add(s.c, load_fp(&keys[3 * r + 2]));
        ++r;
        Fp *const row = full + (u64)L.full_stride * rnd;
        const Fp qa = fp_sqr(s.a), qb = fp_sqr(s.b), qc = fp_sqr(s.c);
        store_fp(row + L.off_full[0], s.a); store_fp(row + L.off_full_sq[0], qa);
        store_fp(row + L.off_full[1], s.b); store_fp(row + L.off_full_sq[1], qb);
        store_fp(row + L.off_full[2], s.c); store_fp(row + L.off_full_sq[2], qc);
        s.a = fp_mul(qa, s.a); s.b = fp_mul(qb, s.b); s.c = fp_mul(qc, s.c);
        s = poseidon_mix(s);
    };
    for (u32 rnd = 0; rnd < 4; ++rnd) full_round(rnd);
    for (u32 k = 0; k < TRACE_POSEIDON_PARTIAL_ROUNDS; ++k, ++r) {
        s.a = fp_add(s.a, load_fp(&keys[3 * r])); s.b = fp_add(s.b, load_fp(&keys[3 * r + 1])); s.c = fp_add(s.c, load_fp(&keys[3 * r + 2]));
        const Fp q = fp_sqr(s.c);
        if (k < L.n_partial) { Fp *const row = partial + (u64)L.partial_stride * k; store_fp(row + L.off_partial, s.c); store_fp(row + L.off_partial_sq, q); }
        if (k >= L.tail_first) { Fp *const row = tail + (u64)L.tail_stride * (k - L.tail_first); store_fp(row + L.off_tail, s.c); store_fp(row + L.off_tail_sq, q); }
        s.c = fp_mul(q, s.c);
        s = poseidon_mix(s);
    }
    for (u32 rnd = 4; rnd < 8; ++rnd) full_round(rnd);
    ped_pool_pair(pool, pool_addr, base + L.off_pair[3], addr0 + 3, s.a);
    ped_pool_pair(pool, pool_addr, base + L.off_pair[4], addr0 + 4, s.b);
    ped_pool_pair(pool, pool_addr, base + L.off_pair[5], addr0 + 5, s.c);
}

// ------------------------------------------------------------------------------------------------ EC-op instances from their inputs
// A GIVEN EC-op instance (index, P, Q, m: 21 u64) -> the cells the host generator's EC-op section writes for it (host/trace_starknet.cpp
// doubling_steps / ec_mad_steps; builtins/src/ec_op/mod.rs:40-130): per step j < 256 the doubling point 2^j Q with its tangent's slope,
// the partial sum P + the 2^i Q of the set bits i < j of m, the suffix m >> j and - for j != 255, the ECDSA section owns those two
// cells of the last step - the chord's slope and 1 / (partial.x - point.x); the two flag cells; the seven memory-pool pairs.
// One workgroup of ONE wave per instance: the two chains are sequential - a wave per instance keeps every instance of a 2^20-step
// statement (1024) resident at once, a wave to a SIMD - and run on lane 0 in Jacobian coordinates into LDS; what surrounds them is
// 256-wide, four steps a lane, each step with ONE inversion of its own (safegcd: no batching, no scan, no scratch outside LDS):
//   wg_doubling_steps   lane 0: the 256 Jacobian doublings; per step: 1 / (2 Y Z) gives both 1 / Z (the affine point) and
//                       1 / (2 y) = Z^4 / (2 Y Z) (the slope) - straight into the cells
//   wg_ec_mad_steps     lane 0: one mixed addition per set bit i (the affine point read back from its cell), the sum AFTER bit i in LDS
//                       slot i; per step j: the sum BEFORE it is the one after the last set bit below j, h = x_j Z^2 - X =
//                       -(partial.x - point.x) Z^2, and 1 / (h Z) gives 1 / Z and 1 / (partial.x - point.x)
// These have the parameters of the host's doubling_steps(p) and ec_mad_steps(x, point, start, max_doublings): an ECDSA instance is
// three of the second and two of the first.  A doubling whose y is zero sets TRACE_ERR_EC_OP_DIVISOR, a partial sum that shares its
// x with its step's point - set bit or clear - TRACE_ERR_EC_OP_MEETS; the workgroup leaves the instance unfinished then (only cells of
// its own steps were touched) and the generation is refused.  An index beyond the blocks or an input with a bit from 252 up: skipped
// with TRACE_ERR_EC_OP_INSTANCE, nothing written.
constexpr u32 EC_STEPS = 256, EC_LANES = 64;
struct EcShared { Fp a[EC_STEPS], b[EC_STEPS], c[EC_STEPS]; u64 rec[21]; u32 divisor, meets, late; };
struct EcJac { Fp X, Y, Z; };
__device__ __forceinline__ EcJac ec_jac_double(const EcJac &p) {     // a = 1: M = 3 X^2 + Z^4, S = 4 X Y^2 (host/trace_common.hpp jac_double)
    const Fp xx = fp_sqr(p.X), yy = fp_sqr(p.Y), zz = fp_sqr(p.Z);
    const Fp s4 = fp_dbl(fp_dbl(fp_mul(p.X, yy)));
    const Fp m = fp_add(fp_add(fp_dbl(xx), xx), fp_sqr(zz));
    EcJac r;
    r.X = fp_sub(fp_sqr(m), fp_dbl(s4));
    r.Y = fp_sub(fp_mul(m, fp_sub(s4, r.X)), fp_dbl(fp_dbl(fp_dbl(fp_sqr(yy)))));
    r.Z = fp_dbl(fp_mul(p.Y, p.Z));
    return r;
}
// p, 2 p, 4 p, ... with the tangents' slopes: x, y, slope of step j to cx / cy / cslope[stride * j].  -> false (for every lane) when a
// doubling divides by zero; sh.a / b / c are scratch
__device__ __forceinline__ bool wg_doubling_steps(EcShared &sh, const Fp &px, const Fp &py, Fp *cx, Fp *cy, Fp *cslope, u64 stride) {
    const u32 t = threadIdx.x;
    if (t == 0) {
        EcJac d;
        d.X = px; d.Y = py; d.Z = fp_one();
#pragma unroll 1
        for (u32 j = 0; j < EC_STEPS; ++j) {
            sh.a[j] = d.X; sh.b[j] = d.Y; sh.c[j] = d.Z;
            if (j + 1 < EC_STEPS) d = ec_jac_double(d);
        }
    }
    __syncthreads();
    for (u32 j = t; j < EC_STEPS; j += EC_LANES)
        if (fp_is_zero(sh.b[j]) || fp_is_zero(sh.c[j])) sh.divisor = 1;              // (Z_{j+1} = 2 Y_j Z_j: a zero y shows in every later Z too)
    __syncthreads();
    if (sh.divisor) return false;
#pragma unroll 1
    for (u32 j = t; j < EC_STEPS; j += EC_LANES) {
        const Fp X = sh.a[j], Y = sh.b[j], Z = sh.c[j];
        const Fp y2 = fp_dbl(Y), zz = fp_sqr(Z);
        const Fp inv = fp_inv_safegcd(fp_mul(y2, Z));
        const Fp zi = fp_mul(y2, inv), zi2 = fp_sqr(zi);
        const Fp x = fp_mul(X, zi2), y = fp_mul(Y, fp_mul(zi2, zi));
        const Fp xx = fp_sqr(x);
        store_fp(&cx[stride * j], x); store_fp(&cy[stride * j], y);
        store_fp(&cslope[stride * j], fp_mul(fp_add(fp_add(fp_dbl(xx), xx), fp_one()), fp_mul(fp_sqr(zz), inv)));
    }
    __syncthreads();
    return true;
}
// the highest set bit below position `limit` (<= 256) of x; -1: none
__device__ __forceinline__ int ec_last_set_below(const u64 *x /* 4 */, u32 limit) {
    for (u32 wk = 4; wk-- > 0;) {
        if (64 * wk >= limit) continue;
        u64 m = x[wk];
        if (limit - 64 * wk < 64) m &= (1ull << (limit - 64 * wk)) - 1;
        if (m) return (int)(64 * wk + 63 - (u32)__clzll((long long)m));
    }
    return -1;
}
// step j of a multiply-add chain: the partial sum before the step, x >> j, the chord's slope (zero where bit j is clear),
// 1 / (partial.x - point.x)
struct EcMadStep { Fp x, y, suffix, slope, x_diff_inv; };
// partial_j = start + the point_i of the set bits i < j of x, point_i = 2^min(i, max_doublings) point = (qx, qy)[qstride * min(i,
// max_doublings)]: the cells wg_doubling_steps has written.  emit(j, step) takes each of the 256 steps, on the lane that made it.
// -> false (for every lane) when a partial sum meets its step's point, before anything is emitted: sh.meets when a step up to the
// scalar's highest set bit does (the steps the reference's mimic_ec_mad_air walks), sh.late when a later one does; sh.a / b / c are
// scratch
template <class Emit>
__device__ __forceinline__ bool wg_ec_mad_steps(EcShared &sh, const u64 *x /* 4 */, const Fp *qx, const Fp *qy, u64 qstride, const Fp &start_x, const Fp &start_y,
                                                u32 max_doublings, const Emit &emit) {
    const u32 t = threadIdx.x;
    if (t == 0) {
        EcJac s;
        s.X = start_x; s.Y = start_y; s.Z = fp_one();
        for (u32 wi = 0; wi < 4; ++wi) {
            u64 bits = x[wi];
#pragma unroll 1
            while (bits) {
                const u64 low = bits & (~bits + 1);
                bits ^= low;
                const u32 i = 64 * wi + 63 - (u32)__clzll((long long)low), pi = i < max_doublings ? i : max_doublings;
                const Fp zz = fp_sqr(s.Z);
                const Fp h = fp_sub(fp_mul(load_fp(&qx[qstride * pi]), zz), s.X), r = fp_sub(fp_mul(load_fp(&qy[qstride * pi]), fp_mul(s.Z, zz)), s.Y);
                if (fp_is_zero(h)) { sh.meets = 1; bits = 0; wi = 4; continue; }        // the chain ends here: what comes after has no sum to start from
                const Fp hh = fp_sqr(h), hhh = fp_mul(h, hh), v = fp_mul(s.X, hh);
                const Fp x3 = fp_sub(fp_sub(fp_sqr(r), hhh), fp_dbl(v));
                s.Y = fp_sub(fp_mul(r, fp_sub(v, x3)), fp_mul(s.Y, hhh));
                s.X = x3;
                s.Z = fp_mul(s.Z, h);
                sh.a[i] = s.X; sh.b[i] = s.Y; sh.c[i] = s.Z;
            }
        }
    }
    __syncthreads();
    if (sh.meets) return false;
    const int top = ec_last_set_below(x, EC_STEPS);
    for (u32 pass = 0; pass < 2; ++pass) {                           // every step's difference is looked at before any step is emitted
#pragma unroll 1
        for (u32 j = t; j < EC_STEPS; j += EC_LANES) {
            const int before = ec_last_set_below(x, j);
            const Fp X = before < 0 ? start_x : sh.a[before], Z = before < 0 ? fp_one() : sh.c[before];
            const u32 pi = j < max_doublings ? j : max_doublings;
            const Fp zz = fp_sqr(Z);
            const Fp h = fp_sub(fp_mul(load_fp(&qx[qstride * pi]), zz), X);            // = (point.x - partial.x) Z^2
            if (pass == 0) { if (fp_is_zero(h)) { if ((int)j <= top) sh.meets = 1; else sh.late = 1; } continue; }
            const Fp Y = before < 0 ? start_y : sh.b[before];
            const Fp inv = fp_inv_safegcd(fp_mul(h, Z));
            const Fp zi = fp_mul(h, inv), zi2 = fp_sqr(zi);
            EcMadStep st;
            st.x = fp_mul(X, zi2); st.y = fp_mul(Y, fp_mul(zi2, zi));
            st.x_diff_inv = fp_neg(fp_mul(fp_mul(zz, Z), inv));
            const bool set = (x[j >> 6] >> (j & 63)) & 1;
            st.slope = set ? fp_mul(fp_sub(st.y, load_fp(&qy[qstride * pi])), st.x_diff_inv) : fp_zero();
            u64 sfx[4];                                              // x >> j
#pragma unroll
            for (u32 k = 0; k < 4; ++k) {
                const u32 w = k + (j >> 6), sft = j & 63;
                u64 v = w < 4 ? x[w] >> sft : 0;
                if (sft && w + 1 < 4) v |= x[w + 1] << (64 - sft);
                sfx[k] = v;
            }
            st.suffix = fp_to_mont(fp_of_words(sfx));
            emit(j, st);
        }
        __syncthreads();
        if (sh.meets | sh.late) return false;
    }
    return true;
}
__global__ __launch_bounds__(EC_LANES) void trace_ec_op_kernel(ColPtrs cols, TraceEcOpLayout L, const u64 *__restrict__ inst, u64 n_blocks, u64 block_rows,
                                                               u64 addr_begin, u32 *__restrict__ pool_addr, u32 *status) {
    __shared__ EcShared sh;
    const u32 t = threadIdx.x;
    if (t < 21) sh.rec[t] = inst[21 * (u64)blockIdx.x + t];
    if (t == 0) sh.divisor = sh.meets = sh.late = 0;
    __syncthreads();
    const u64 *rec = sh.rec;
    const u64 index = rec[0];
    if (index >= n_blocks || ((rec[4] | rec[8] | rec[12] | rec[16] | rec[20]) >> 60)) {          // (the whole workgroup leaves)
        if (t == 0) status_error(status, TRACE_ERR_EC_OP_INSTANCE, blockIdx.x);
        return;
    }
    const u64 base = index * block_rows, stride = L.row_stride;
    Fp *const col = (Fp *)cols.dst[L.col] + base;
    const u64 *m = rec + 17;
    if (!wg_doubling_steps(sh, fp_to_mont(fp_of_words(rec + 9)), fp_to_mont(fp_of_words(rec + 13)), col + L.off_dbl_x, col + L.off_dbl_y, col + L.off_dbl_slope, stride)) {
        if (t == 0) status_error(status, TRACE_ERR_EC_OP_DIVISOR, index);
        return;
    }
    Fp *const pool = (Fp *)cols.dst[L.col_pool];
    const u64 addr0 = addr_begin + 7 * index;
    const bool done = wg_ec_mad_steps(sh, m, col + L.off_dbl_x, col + L.off_dbl_y, stride, fp_to_mont(fp_of_words(rec + 1)), fp_to_mont(fp_of_words(rec + 5)), EC_STEPS - 1,
                                      [&](u32 j, const EcMadStep &st) {
        const u64 row = stride * j;
        store_fp(&col[L.off_sum_x + row], st.x); store_fp(&col[L.off_sum_y + row], st.y); store_fp(&col[L.off_suffix + row], st.suffix);
        if (j != EC_STEPS - 1) { store_fp(&col[L.off_slope + row], st.slope); store_fp(&col[L.off_x_diff_inv + row], st.x_diff_inv); }
        else {                                                       // R: the sum before step 255 (bit 255 of m is never set)
            ped_pool_pair(pool, pool_addr, base + L.off_pair[5], addr0 + 5, st.x);
            ped_pool_pair(pool, pool_addr, base + L.off_pair[6], addr0 + 6, st.y);
        }
    });
    if (!done) {
        if (t == 0) status_error(status, TRACE_ERR_EC_OP_MEETS, index);
        return;
    }
    // the flag cells (none of them a step's cell) and the pool's other pairs
    if (t == 0) {
        const u64 top = m[3];                                        // bits 192 ..: bit 251 = 59, 196 = 4, 192 = 0
        const bool f2 = ((top >> 59) & 1) && ((top >> 4) & 1), f3 = f2 && (top & 1);
        store_fp(&col[L.off_flag2], fp_from_u64(f2));
        store_fp(&col[L.off_flag3], fp_from_u64(f3));
    }
    if (t >= 1 && t <= 5) {
        const u32 k = t - 1;
        const u32 off = k == 0 ? L.off_pair[0] : k == 1 ? L.off_pair[1] : k == 2 ? L.off_pair[2] : k == 3 ? L.off_pair[3] : L.off_pair[4];      // (selects: no lane-indexed kernel argument)
        ped_pool_pair(pool, pool_addr, base + off, addr0 + k, fp_to_mont(fp_of_words(rec + 1 + 4 * k)));
    }
}

// ------------------------------------------------------------------------------------------------ ECDSA builtin
// A given signature from the public key (x and either root y of x^3 + x + beta), the message z, r and w (builtins/src/ecdsa/mod.rs:85-147
// InstanceTrace::new; starknet trace.rs:428-523; host/trace_starknet.cpp ecdsa_trace and the section's `place` lambda): one wave per
// instance, three of wg_ec_mad_steps and two of wg_doubling_steps.  z G from -P0 over the constant points 2^i G (its cells do not depend
// on the root); then, for the canonically larger of y, p - y first (verify, ecdsa/mod.rs:275-304): Q's doubling chain and r Q from P0,
// B = z G + r Q, B's doubling chain and w B from P0, and the check x(w B - P0) = r.  A candidate that fails the check, or whose partial sum
// meets its step's point at a step mimic_ec_mad_air walks, is rejected and the other root runs the same way over the same cells (a full
// second pass: every cell the first wrote is written again); both rejected: TRACE_ERR_ECDSA_INVALID, as a scalar that is zero or has bit
// 251 set.  A doubling whose y is zero, or a zero z G.x - r Q.x or w B.x - P0.x: TRACE_ERR_ECDSA_DIVISOR; a meeting at a step above the
// scalar's highest set bit (mimic_ec_mad_air does not see it, gen_ec_mad_steps divides by it): TRACE_ERR_ECDSA_MEETS - both end the
// instance at the candidate that finds them (with a key on the curve neither is reachable: the start points are fixed and the group's
// order is prime).  The eight cells an instance has one of are written last: four of them are step-255 cells of the chains.
struct EcdsaShared { Fp zg[2], end[2], b_slope, b_x_diff_inv, r_slope, r_x_diff_inv; };
__device__ __forceinline__ bool ecdsa_scalar_ok(const u64 *s /* 4 */) { return (s[0] | s[1] | s[2] | s[3]) && !(s[3] >> 59); }       // 1 <= bit length < 252
__global__ __launch_bounds__(EC_LANES) void trace_ecdsa_kernel(ColPtrs cols, TraceEcdsaLayout L, const Fp *__restrict__ points, const u64 *__restrict__ inst,
                                                               u64 n_blocks, u64 block_rows, u64 addr_begin, u32 *__restrict__ pool_addr, u32 *status) {
    __shared__ EcShared sh;
    __shared__ EcdsaShared es;
    const u32 t = threadIdx.x;
    if (t < 21) sh.rec[t] = inst[21 * (u64)blockIdx.x + t];
    if (t == 0) sh.divisor = sh.meets = sh.late = 0;
    __syncthreads();
    const u64 *rec = sh.rec;
    const u64 index = rec[0];
    if (index >= n_blocks || ((rec[4] | rec[8] | rec[12] | rec[16] | rec[20]) >> 60)) {          // (the whole workgroup leaves, here and below)
        if (t == 0) status_error(status, TRACE_ERR_ECDSA_INSTANCE, blockIdx.x);
        return;
    }
    const u64 *key_y = rec + 5, *message = rec + 9, *r = rec + 13, *w = rec + 17;
    if (!ecdsa_scalar_ok(message) || !ecdsa_scalar_ok(r) || !ecdsa_scalar_ok(w)) {
        if (t == 0) status_error(status, TRACE_ERR_ECDSA_INVALID, index);
        return;
    }
    const u64 base = index * block_rows, stride = L.row_stride;
    Fp *const col = (Fp *)cols.dst[L.col] + base;
    const Fp *const shift = points + 2 * TRACE_ECDSA_SHIFT;
    // z G: the sum before step 255 is the whole sum (bit 251 and up are clear)
    if (!wg_ec_mad_steps(sh, message, points, points + 1, 2, load_fp(shift), fp_neg(load_fp(shift + 1)), TRACE_ECDSA_SHIFT - 1, [&](u32 j, const EcMadStep &st) {
            const u64 row = (u64)L.gen_stride * j;
            store_fp(&col[L.off_gen_x + row], st.x); store_fp(&col[L.off_gen_y + row], st.y); store_fp(&col[L.off_gen_slope + row], st.slope);
            store_fp(&col[L.off_gen_x_diff_inv + row], st.x_diff_inv); store_fp(&col[L.off_gen_suffix + row], st.suffix);
            if (j == EC_STEPS - 1) { es.zg[0] = st.x; es.zg[1] = st.y; }
        })) {
        if (t == 0) status_error(status, sh.meets ? TRACE_ERR_ECDSA_INVALID : TRACE_ERR_ECDSA_MEETS, index);
        return;
    }
    // y >= (p + 1) / 2 = 2^250 + 17 * 2^191 + 1: y is the larger of y, p - y
    const u64 half_p[4] = {1, 0, 0x8000000000000000ull, 0x0400000000000008ull};
    bool y_first = true;
    for (u32 k = 4; k-- > 0;) if (key_y[k] != half_p[k]) { y_first = key_y[k] > half_p[k]; break; }
    bool accepted = false;
#pragma unroll 1
    for (u32 cand = 0; cand < 2 && !accepted; ++cand) {
        bool rejected = false;
#pragma unroll 1
        for (u32 half = 0; half < 2 && !rejected; ++half) {           // 0: Q's doublings and r Q; 1: B's and w B
            Fp px, py;
            if (half == 0) {
                px = fp_to_mont(fp_of_words(rec + 1)); py = fp_to_mont(fp_of_words(key_y));
                if (y_first != (cand == 0)) py = fp_neg(py);
            } else {                                                 // B = z G + r Q along the chord (every lane: the values are the wave's)
                const Fp dx = fp_sub(es.zg[0], es.end[0]);
                if (fp_is_zero(dx)) {
                    if (t == 0) status_error(status, TRACE_ERR_ECDSA_DIVISOR, index);
                    return;
                }
                const Fp inv = fp_inv_safegcd(dx), slope = fp_mul(fp_sub(es.zg[1], es.end[1]), inv);
                px = fp_sub(fp_sub(fp_sqr(slope), es.zg[0]), es.end[0]);
                py = fp_sub(fp_mul(slope, fp_sub(es.zg[0], px)), es.zg[1]);
                if (t == 0) { es.b_slope = slope; es.b_x_diff_inv = inv; }
            }
            Fp *const c = col + stride * EC_STEPS * half;
            if (!wg_doubling_steps(sh, px, py, c + L.off_dbl_x, c + L.off_dbl_y, c + L.off_dbl_slope, stride)) {
                if (t == 0) status_error(status, TRACE_ERR_ECDSA_DIVISOR, index);
                return;
            }
            if (!wg_ec_mad_steps(sh, half ? w : r, c + L.off_dbl_x, c + L.off_dbl_y, stride, load_fp(shift), load_fp(shift + 1), EC_STEPS - 1,
                                 [&](u32 j, const EcMadStep &st) {
                    const u64 row = stride * j;
                    store_fp(&c[L.off_sum_x + row], st.x); store_fp(&c[L.off_sum_y + row], st.y); store_fp(&c[L.off_slope + row], st.slope);
                    store_fp(&c[L.off_x_diff_inv + row], st.x_diff_inv); store_fp(&c[L.off_suffix + row], st.suffix);
                    if (j == EC_STEPS - 1) { es.end[0] = st.x; es.end[1] = st.y; }
                })) {
                if (!sh.meets) {
                    if (t == 0) status_error(status, TRACE_ERR_ECDSA_MEETS, index);
                    return;
                }
                __syncthreads();                                     // (every lane has read the flags)
                if (t == 0) sh.meets = sh.late = 0;
                __syncthreads();
                rejected = true;
            }
        }
        if (rejected) continue;
        // R = w B - P0 along the chord; its x is r
        const Fp dx = fp_sub(es.end[0], load_fp(shift));
        if (fp_is_zero(dx)) {
            if (t == 0) status_error(status, TRACE_ERR_ECDSA_DIVISOR, index);
            return;
        }
        const Fp inv = fp_inv_safegcd(dx), slope = fp_mul(fp_add(es.end[1], load_fp(shift + 1)), inv);
        accepted = fp_eq(fp_sub(fp_sub(fp_sqr(slope), es.end[0]), load_fp(shift)), fp_to_mont(fp_of_words(r)));
        if (accepted && t == 0) { es.r_slope = slope; es.r_x_diff_inv = inv; }
        __syncthreads();                                             // (es.end is read; the other root's chains write it again)
    }
    if (!accepted) {
        if (t == 0) status_error(status, TRACE_ERR_ECDSA_INVALID, index);
        return;
    }
    // the cells an instance has one of, after the steps': four of them lie on step 255 of a chain
    if (t < 8) {
        const u32 off = t == 0 ? L.off_w_inv : t == 1 ? L.off_r_inv : t == 2 ? L.off_message_inv : t == 3 ? L.off_r_point_slope : t == 4 ? L.off_r_point_x_diff_inv
                      : t == 5 ? L.off_pubkey_x_squared : t == 6 ? L.off_b_slope : L.off_b_x_diff_inv;       // (selects: no lane-indexed kernel argument)
        Fp v;
        if (t < 3) v = fp_inv_safegcd(fp_to_mont(fp_of_words(t == 0 ? w : t == 1 ? r : message)));
        else if (t == 5) v = fp_sqr(fp_to_mont(fp_of_words(rec + 1)));
        else v = t == 3 ? es.r_slope : t == 4 ? es.r_x_diff_inv : t == 6 ? es.b_slope : es.b_x_diff_inv;
        store_fp(&col[off], v);
    } else if (t < 10) {
        const u32 k = t - 8;
        ped_pool_pair((Fp *)cols.dst[L.col_pool], pool_addr, base + (k ? L.off_pair[1] : L.off_pair[0]), addr_begin + 2 * index + k,
                      fp_to_mont(fp_of_words(k ? message : rec + 1)));
    }
}

// ------------------------------------------------------------------------------------------------ range-check builtin and pool
// the pool's padding values in order (utils.rs:357-380 RangeCheckPool::get_ordered_values_with_padding's second half), then rc_hi
__device__ __forceinline__ u32 rc_padding(const TraceRcPlan &p, const uint16_t *padding, u64 j) { return j < p.n_padding ? padding[j] : p.rc_hi; }

// slot s of the range-check builtin (trace.rs:388-426 / recursive 236-284): a given instance, or a dummy whose 8 parts are the
// next padding values; the 16-bit parts go to the range-check column, (address, value) to the memory pool
__global__ __launch_bounds__(256) void trace_rc_builtin_kernel(TraceRcPlan p, const u64 *__restrict__ given /* index, lo, hi */, const uint16_t *__restrict__ padding,
                                                               Fp *__restrict__ rc, Fp *__restrict__ npc, u32 *__restrict__ pool_addr) {
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n_slots) return;
    u64 lo, hi, index = s;
    if (s < p.n_given) { index = given[3 * s]; lo = given[3 * s + 1]; hi = given[3 * s + 2]; }
    else {
        lo = hi = 0;
        for (u32 k = 0; k < 8; ++k) { hi = (hi << 16) | (lo >> 48); lo = (lo << 16) | rc_padding(p, padding, 8 * (s - p.n_given) + k); }
    }
    const u64 base = s * p.slot_rows;
    for (u32 k = 0; k < 8; ++k) {
        const u32 sh = 16 * (7 - k);
        store_fp(&rc[base + (u64)p.part_stride * k + p.part_off], fp_from_u64((sh >= 64 ? hi >> (sh - 64) : lo >> sh) & 0xffff));
    }
    const u64 a = p.addr_begin + index;
    Fp v = fp_zero();
    v.v[0] = (u32)lo; v.v[1] = (u32)(lo >> 32); v.v[2] = (u32)hi; v.v[3] = (u32)(hi >> 32);
    store_fp(&npc[base + p.pair_off], fp_from_u64(a));
    store_fp(&npc[base + p.pair_off + 1], fp_to_mont(v));
    pool_addr[(base + p.pair_off) >> 1] = sat32(a);
}

// the value of slot k of an ordered pool: every value of [lo, hi] max(count, 1) times, ascending; first[j] = slots before value
// lo + j (j <= hi - lo + 1).  -> the value, or `beyond` from the pool's end on
__device__ __forceinline__ u32 run_value(const u32 *__restrict__ first, u32 n_values, u32 lo, u64 k, u32 beyond) {
    if (k >= first[n_values]) return beyond;
    u32 a = 0, b = n_values;                  // first[a] <= k < first[b]
    while (b - a > 1) { const u32 m = (a + b) >> 1; if (first[m] <= k) a = m; else b = m; }
    return lo + a;
}
// per cycle: its ordered values (every RANGE_CHECK_STEP rows) and, on odd cycles, the next unused padding value (trace.rs:263-292)
__global__ __launch_bounds__(256) void trace_rc_pool_kernel(TraceRcPlan p, const u32 *__restrict__ first, const uint16_t *__restrict__ padding, u64 num_cycles,
                                                            Fp *__restrict__ rc) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 per = 16 / p.ordered_step;
    if (g < num_cycles * per) {
        const u64 cyc = g / per, j = g - cyc * per;
        store_fp(&rc[cyc * 16 + j * p.ordered_step + p.ordered_off], fp_from_u64(run_value(first, p.rc_hi - p.rc_lo + 1, p.rc_lo, g, p.rc_hi)));
    } else if (g < num_cycles * per + num_cycles / 2) {
        const u64 h = g - num_cycles * per;   // odd cycle 2 h + 1
        store_fp(&rc[(2 * h + 1) * 16 + p.unused_off], fp_from_u64(rc_padding(p, padding, p.pad0 + h)));
    }
}

__device__ __forceinline__ u64 dilute16(u32 v) {                     // bit i -> bit 4 i (builtins/src/bitwise/mod.rs dilute)
    u64 x = v & 0xffffu;
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}
// slot k of an ordered pool into col[k * stride + off]: zero before the pool's first slot (first[0]), then the runs
__global__ __launch_bounds__(256) void trace_runs_kernel(Fp *__restrict__ col, u64 stride, u64 off, u64 slots, const u32 *__restrict__ first, u32 n_values,
                                                         u32 lo, u32 diluted) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= slots) return;
    Fp v = fp_zero();
    if (k >= first[0]) {
        const u32 x = run_value(first, n_values, lo, k, lo + n_values - 1);
        v = fp_from_u64(diluted ? dilute16(x) : x);
    }
    store_fp(&col[k * stride + off], v);
}
__global__ __launch_bounds__(256) void trace_patch_kernel(Fp *__restrict__ col, u64 col_rows, const u64 *__restrict__ rows, const u64 *__restrict__ values, u64 count) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k < count && rows[k] < col_rows) store_fp(&col[rows[k]], fp_from_u64(values[k]));
}

// ------------------------------------------------------------------------------------------------ exclusive prefix sums (u32)
constexpr u32 SCAN_LANES = 256, SCAN_PER = 16, SCAN_CHUNK = SCAN_LANES * SCAN_PER;
// exclusive scan of the 256 lane sums of a workgroup -> the lane's offset; *total = their sum
__device__ __forceinline__ u32 wg_exclusive(u32 mine, u32 *lds, u32 *total) {
    const u32 t = threadIdx.x;
    lds[t] = mine;
    __syncthreads();
    for (u32 d = 1; d < SCAN_LANES; d <<= 1) {
        const u32 add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const u32 incl = lds[t];
    *total = lds[SCAN_LANES - 1];
    __syncthreads();
    return incl - mine;
}
__global__ __launch_bounds__(SCAN_LANES) void scan_chunks_kernel(u32 *__restrict__ data, u64 n, u32 *__restrict__ sums) {
    __shared__ u32 lds[SCAN_LANES];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_PER;
    u32 v[SCAN_PER], s = 0;
#pragma unroll
    for (u32 k = 0; k < SCAN_PER; ++k) { v[k] = base + k < n ? data[base + k] : 0; s += v[k]; }
    u32 total;
    u32 run = wg_exclusive(s, lds, &total);
#pragma unroll
    for (u32 k = 0; k < SCAN_PER; ++k) { if (base + k < n) data[base + k] = run; run += v[k]; }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: the chunk sums in place (exclusive), the grand total to *total_out
__global__ __launch_bounds__(SCAN_LANES) void scan_sums_kernel(u32 *__restrict__ sums, u32 n_sums, u32 *total_out) {
    __shared__ u32 lds[SCAN_LANES];
    u32 carry = 0;
    for (u32 c0 = 0; c0 < n_sums; c0 += SCAN_CHUNK) {
        const u32 base = c0 + threadIdx.x * SCAN_PER;
        u32 v[SCAN_PER], s = 0;
#pragma unroll
        for (u32 k = 0; k < SCAN_PER; ++k) { v[k] = base + k < n_sums ? sums[base + k] : 0; s += v[k]; }
        u32 total;
        u32 run = carry + wg_exclusive(s, lds, &total);
#pragma unroll
        for (u32 k = 0; k < SCAN_PER; ++k) { if (base + k < n_sums) sums[base + k] = run; run += v[k]; }
        carry += total;
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}
__global__ __launch_bounds__(SCAN_LANES) void scan_apply_kernel_u32(u32 *__restrict__ data, u64 n, const u32 *__restrict__ sums) {
    const u32 add = sums[blockIdx.x];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + threadIdx.x;
#pragma unroll
    for (u32 k = 0; k < SCAN_PER; ++k) { const u64 i = base + (u64)k * SCAN_LANES; if (i < n) data[i] += add; }
}
hipError_t exclusive_scan_u32(hipStream_t st, u32 *data, u64 n, u32 *sums, u32 *total_out) {
    const u32 chunks = (u32)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);
    hipLaunchKernelGGL(scan_chunks_kernel, dim3(chunks), dim3(SCAN_LANES), 0, st, data, n, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_LANES), 0, st, sums, chunks, total_out);
    hipLaunchKernelGGL(scan_apply_kernel_u32, dim3(chunks), dim3(SCAN_LANES), 0, st, data, n, (const u32 *)sums);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ ordered memory
constexpr u32 MEM_LANES = 256, MEM_PER = 16, MEM_SLOTS = 1024;
// accesses per address: count[a] (a >= 2) and rep[a] = the first access of a (its index in the pool); address 0 / 1 accesses are
// counted in the status words (most of a run: the public-memory slots and the padding pairs).  Hot addresses - an idling run reads
// its `jmp rel 0` a million times - are counted in an LDS table per workgroup and reach the global arrays once per workgroup.
__global__ __launch_bounds__(MEM_LANES) void mem_count_kernel(const u32 *__restrict__ pool_addr, u64 half, u32 cap, u32 *__restrict__ count, u32 *__restrict__ rep,
                                                              u32 *status) {
    __shared__ u32 key[MEM_SLOTS], cnt[MEM_SLOTS], first[MEM_SLOTS];
    __shared__ u32 agg[4];                    // zeros, ones, max address, ~min address
    const u32 t = threadIdx.x;
    for (u32 s = t; s < MEM_SLOTS; s += MEM_LANES) { key[s] = 0; cnt[s] = 0; first[s] = 0xffffffffu; }
    if (t < 4) agg[t] = 0;
    __syncthreads();
    u32 zeros = 0, ones = 0, top = 0, nlow = 0;
    for (u32 it = 0; it < MEM_PER; ++it) {
        const u64 j = (u64)blockIdx.x * (MEM_LANES * MEM_PER) + (u64)it * MEM_LANES + t;
        if (j >= half) break;
        const u32 a = pool_addr[j];
        top = a > top ? a : top;
        nlow = ~a > nlow ? ~a : nlow;
        if (a == 0) { ++zeros; continue; }
        if (a == 1) { ++ones; continue; }
        if (a > cap) { status_error(status, TRACE_ERR_ADDRESS_RANGE, a); continue; }
        const u32 s = a & (MEM_SLOTS - 1);
        const u32 old = atomicCAS(&key[s], 0u, a);
        if (old == 0 || old == a) { atomicAdd(&cnt[s], 1u); atomicMin(&first[s], (u32)j); }
        else { atomicAdd(&count[a], 1u); atomicMin(&rep[a], (u32)j); }
    }
    if (zeros) atomicAdd(&agg[0], zeros);
    if (ones) atomicAdd(&agg[1], ones);
    atomicMax(&agg[2], top);
    atomicMax(&agg[3], nlow);
    __syncthreads();
    for (u32 s = t; s < MEM_SLOTS; s += MEM_LANES)
        if (key[s]) { atomicAdd(&count[key[s]], cnt[s]); atomicMin(&rep[key[s]], first[s]); }
    if (t == 0) {
        if (agg[0]) atomicAdd(&status[TRACE_ST_ZEROS], agg[0]);
        if (agg[1]) atomicAdd(&status[TRACE_ST_ONES], agg[1]);
        atomicMax(&status[TRACE_ST_TOP], agg[2]);
        atomicMax(&status[TRACE_ST_NLOW], agg[3]);
    }
}
// the public memory's entries are accesses too (utils.rs:116-131): entry k is access half + k
__global__ __launch_bounds__(256) void mem_public_kernel(const u32 *__restrict__ pub_addr, u32 n_pub, u64 half, u32 cap, u32 *__restrict__ count,
                                                         u32 *__restrict__ rep, u32 *status) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_pub) return;
    const u32 a = pub_addr[k];
    atomicMax(&status[TRACE_ST_TOP], a);
    atomicMax(&status[TRACE_ST_NLOW], ~a);
    if (a == 0) { status_error(status, TRACE_ERR_PUBLIC_ZERO, 0); return; }
    if (a == 1) { atomicAdd(&status[TRACE_ST_ONES], 1u); return; }
    if (a > cap) { status_error(status, TRACE_ERR_ADDRESS_RANGE, a); return; }
    atomicAdd(&count[a], 1u);
    atomicMin(&rep[a], (u32)(half + k));
}
// gap fillers (trace.rs:594-625 / 890-925): the addresses strictly between the lowest and the highest accessed one that nothing
// accesses, ascending; gap number g takes the unused pool pair of cycle g as (address, 0)
__global__ __launch_bounds__(256) void mem_gap_flags_kernel(const u32 *__restrict__ count, u32 cap, const u32 *status, u32 *__restrict__ flag) {
    const u32 a = blockIdx.x * 256 + threadIdx.x;
    if (a > cap) return;
    const u32 top = status[TRACE_ST_TOP], low = ~status[TRACE_ST_NLOW];
    flag[a] = (a > low && a < top && a >= 2 && count[a] == 0) ? 1u : 0u;             // (address 1 always has the padding pairs; 0 is never a gap: low <= 0)
}
__global__ __launch_bounds__(256) void mem_gap_fill_kernel(const u32 *__restrict__ gap_index, u32 cap, u64 num_cycles, u32 unused_off, u32 *__restrict__ count,
                                                           u32 *__restrict__ rep, Fp *__restrict__ npc, u32 *__restrict__ pool_addr, u32 *status) {
    const u32 a = blockIdx.x * 256 + threadIdx.x;
    if (a > cap) return;
    const u32 top = status[TRACE_ST_TOP], low = ~status[TRACE_ST_NLOW];
    if (!(a > low && a < top && a >= 2 && count[a] == 0)) return;
    const u32 g = gap_index[a];
    if (g >= num_cycles) { status_error(status, TRACE_ERR_TOO_MANY_GAPS, a); return; }
    const u64 row = (u64)g * 16 + unused_off;
    store_fp(&npc[row], fp_from_u64(a));
    store_fp(&npc[row + 1], fp_zero());
    pool_addr[row >> 1] = a;
    count[a] = 1;
    rep[a] = (u32)(row >> 1);
}
__device__ __forceinline__ Fp mem_value_of(u32 idx, u64 half, const Fp *npc, const Fp *pub_value) {
    return idx < half ? load_fp(&npc[2 * (u64)idx + 1]) : load_fp(&pub_value[idx - half]);
}
// the reference's checks (utils.rs:132-150): one value per address, the pool's address-0 cells are exactly the public-memory
// cells, memory starts at address 1 and has no holes; then the counts become the prefix array's input: start[a] = count of a
// (address 1: the padding pairs that are left + the public memory's own entries at 1)
__global__ __launch_bounds__(256) void mem_check_kernel(const u32 *__restrict__ pool_addr, u64 half, const u32 *__restrict__ pub_addr, u32 n_pub,
                                                        const Fp *__restrict__ pub_value, Fp pad_value, const u32 *__restrict__ rep, const Fp *__restrict__ npc,
                                                        u32 cap, u32 *status) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= half + n_pub) return;
    const u32 a = j < half ? pool_addr[j] : pub_addr[j - half];
    if (a == 0 || a > cap) return;
    const Fp mine = mem_value_of((u32)j, half, npc, pub_value);
    const Fp want = a == 1 ? pad_value : mem_value_of(rep[a], half, npc, pub_value);
    if (!fp_eq(mine, want)) status_error(status, TRACE_ERR_NOT_SINGLE_VALUED, a);
}
__global__ __launch_bounds__(256) void mem_starts_kernel(const u32 *__restrict__ count, u32 cap, u64 public_cells, u32 n_pub, u32 *status, u32 *__restrict__ start) {
    const u32 a = blockIdx.x * 256 + threadIdx.x;
    if (a > cap + 1) return;
    const u32 top = status[TRACE_ST_TOP];
    // the padding pairs the gaps took are gone; the public memory's padding entries (1, pad) come on top (utils.rs:120-124)
    const u32 ones = status[TRACE_ST_ONES] - status[TRACE_ST_GAPS] + (u32)(public_cells - n_pub);
    u32 c = 0;
    if (a == 1) c = ones;
    else if (a >= 2 && a <= top && a <= cap) c = count[a];
    if (a >= 1 && a <= top && a <= cap && c == 0) status_error(status, TRACE_ERR_NOT_CONTINUOUS, a);
    if (a == 0) {
        if (status[TRACE_ST_ZEROS] != public_cells) status_error(status, TRACE_ERR_PUBLIC_CELLS, 0);
        if (top > cap) status_error(status, TRACE_ERR_ADDRESS_RANGE, top);
    }
    start[a] = c;
}
// row pair j of the ordered column: (a, value of a) for the address whose run holds j (utils.rs:138-152)
__global__ __launch_bounds__(256) void mem_fill_kernel(const u32 *__restrict__ start, u64 half, u32 cap, const u32 *__restrict__ rep, const Fp *__restrict__ npc,
                                                       const Fp *__restrict__ pub_value, Fp pad_value, Fp *__restrict__ mem_col, u32 *status) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    u32 top = status[TRACE_ST_TOP];
    if (top > cap) top = cap;
    Fp av = fp_zero(), vv = fp_zero();
    if (j >= start[top + 1]) {                                       // the runs do not fill the column
        status_error(status, TRACE_ERR_FILL, top);
    } else {
        u32 a = 0, b = top + 1;                                      // start[a] <= j < start[b]
        while (b - a > 1) { const u32 m = (a + b) >> 1; if (start[m] <= j) a = m; else b = m; }
        av = fp_from_u64(a);
        vv = a <= 1 ? pad_value : mem_value_of(rep[a], half, npc, pub_value);
    }
    store_fp(&mem_col[2 * j], av);
    store_fp(&mem_col[2 * j + 1], vv);
}
__global__ void mem_fill_total_kernel(const u32 *__restrict__ start, u64 half, u32 cap, u32 *status) {
    if (threadIdx.x || blockIdx.x) return;
    u32 top = status[TRACE_ST_TOP];
    if (top > cap) top = cap;
    if (start[top + 1] != half) status_error(status, TRACE_ERR_FILL, top);
    if (start[2] == 0) status_error(status, TRACE_ERR_NO_ONES, 1);     // start[2] = accesses of address 1 (start[0] = start[1] = 0)
}

// ------------------------------------------------------------------------------------------------ the plain layout over the 64-bit field
// ExecutionTrace::new of layouts/src/plain/trace.rs:60-262 (restated cell for cell by sandstorm_amd/layouts/plain.py base_trace): five
// columns of canonical u64 values below p = 2^64 - 2^32 + 1 (gl64.h), not Montgomery - what every *_gl64* entry point takes.  The field has
// this one layout, so the placement is written out here instead of coming in as tables:
//   flags        the 16 prefix values
//   pool (Npc)   pairs 0 / 2 / 4 / 6 = (pc, instruction), (op0), (dst), (op1); pairs 1 and 5 the public-memory slots (0, 0); pairs 3 and 7
//                the padding pair (1, value at 1) - pair 7 is the gap cell mem_gap_fill_gl64_kernel takes
//   range check  offsets 0 / 4 / 8 = off_dst / off_op1 / off_op0; 3 / 7 / 11 / 15 = ap / op0 * op1 / fp / res; 2 + 4 j the ordered values
//                and 12 the unused value (trace_gl64_rc_pool_kernel); the filler elsewhere
//   auxiliary    tmp0 at 0, tmp1 at 8, zero elsewhere
// The memory image holds one u64 per cell; all ones (>= p: no field element) marks a cell no record names, or whose word is no field element.
// A CPU error names its cycle in a status word of ITS OWN BIT (TRACE_ST_GL_CYCLE + bit number): the ordered memory's errors name
// addresses in TRACE_ST_WHERE, and a cycle of one error is never reported for another.
__global__ __launch_bounds__(256) void trace_gl64_memory_image_kernel(const u64 *__restrict__ records, u64 n_records, u64 *__restrict__ image, u64 cells) {
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_records) return;
    const u64 a = records[5 * k];
    if (a >= cells) return;
    const u64 w = records[5 * k + 1];
    if ((records[5 * k + 2] | records[5 * k + 3] | records[5 * k + 4]) || w >= GL_P) return;      // no field element: the cell keeps the mark
    image[a] = w;
}

struct GlCpuRec {
    u64 word, ap, fp;
    u64 val[4];                              // the instruction word, op0, dst, op1 (REC_*)
    u64 res, tmp1, mul;
    u32 addr[4];                             // pc, op0, dst, op1, saturated as in CpuRec
    u32 jnz, pad;
};
__device__ __forceinline__ bool gl_image_cell(const u64 *image, u64 cells, u64 a, u64 &w) {
    w = 0;
    if (a >= cells) return false;
    const u64 v = image[a];
    if (v >= GL_P) return false;
    w = v;
    return true;
}
__device__ __forceinline__ void gl_cpu_error(u32 *status, u32 bits, u64 cyc) {
    atomicOr(&status[TRACE_ST_ERRORS], bits);
#pragma unroll
    for (u32 b = 0; b < TRACE_GL_CPU_ERROR_BITS; ++b)
        if ((bits >> b) & 1) atomicMax(&status[TRACE_ST_GL_CYCLE + b], ~sat32(cyc));
}

__global__ __launch_bounds__(CPU_CYC) void trace_gl64_cpu_kernel(const u64 *__restrict__ states, u64 num_cycles, const u64 *__restrict__ image, u64 cells, u64 pad_value,
                                                                 u64 rc_fill, u64 *__restrict__ flags, u64 *__restrict__ npc, u64 *__restrict__ rc, u64 *__restrict__ aux,
                                                                 u32 *__restrict__ pool_addr, u32 *status) {
    __shared__ GlCpuRec rec[CPU_CYC];
    const u32 t = threadIdx.x;
    const u64 cyc0 = (u64)blockIdx.x * CPU_CYC, cyc = cyc0 + t;
    if (cyc < num_cycles) {
        GlCpuRec &r = rec[t];
        const u64 ap = states[3 * cyc], fp = states[3 * cyc + 1], pc = states[3 * cyc + 2];
        u32 err = 0;
        u64 w, op0, dst, op1;
        if (!gl_image_cell(image, cells, pc, w)) err |= TRACE_ERR_MISSING_CELL;
        if (w >> 63) err |= TRACE_ERR_NOT_INSTRUCTION;
        auto flag = [&](int f) { return (u32)((w >> (48 + f)) & 1); };
        const u64 dst_addr = (w & 0xffff) + (flag(0) ? fp : ap) - 0x8000, op0_addr = ((w >> 16) & 0xffff) + (flag(1) ? fp : ap) - 0x8000;
        if (!gl_image_cell(image, cells, op0_addr, op0)) err |= TRACE_ERR_MISSING_CELL;
        if (!gl_image_cell(image, cells, dst_addr, dst)) err |= TRACE_ERR_MISSING_CELL;
        const u32 src = flag(2) + 2 * flag(3) + 4 * flag(4);
        u64 base = 0;
        if (src == 0) { if (op0 >> 32) err |= TRACE_ERR_NOT_AN_ADDRESS; base = op0; }      // (no address of a trace has more than 32 bits)
        else if (src == 1) base = pc;
        else if (src == 2) base = fp;
        else if (src == 4) base = ap;
        else err |= TRACE_ERR_BAD_OP1_SOURCE;
        const u64 op1_addr = ((w >> 32) & 0xffff) + base - 0x8000;
        if (!gl_image_cell(image, cells, op1_addr, op1)) err |= TRACE_ERR_MISSING_CELL;
        const u32 pc_update = flag(7) + 2 * flag(8) + 4 * flag(9), res_logic = flag(5) + 2 * flag(6);
        u64 res = 0;
        if (pc_update == 4) { if (dst) res = gl_pow(dst, GL_P - 2); }                      // get_res of a conditional jump: dst^-1
        else if (res_logic == 0) res = op1;
        else if (res_logic == 1) res = gl_add(op0, op1);
        else if (res_logic == 2) res = gl_mul(op0, op1);
        else err |= TRACE_ERR_BAD_RES_LOGIC;
        r.word = w; r.ap = gl_canon(ap); r.fp = gl_canon(fp);
        r.addr[REC_PC] = sat32(pc); r.addr[REC_OP0] = sat32(op0_addr); r.addr[REC_DST] = sat32(dst_addr); r.addr[REC_OP1] = sat32(op1_addr);
        r.jnz = flag(9);
        r.val[REC_PC] = w; r.val[REC_OP0] = op0; r.val[REC_DST] = dst; r.val[REC_OP1] = op1;
        r.res = res; r.tmp1 = r.jnz ? gl_mul(dst, res) : 0; r.mul = gl_mul(op0, op1);
        if (err) gl_cpu_error(status, err, cyc);
    }
    __syncthreads();
    const u64 live = num_cycles - cyc0 < CPU_CYC ? num_cycles - cyc0 : CPU_CYC;       // cycles of this workgroup
    const u64 row0 = cyc0 * 16;
    for (u32 it = 0; it < 16; ++it) {
        const u32 lr = it * CPU_CYC + t, c = lr >> 4, o = lr & 15;
        if (c >= live) break;
        const GlCpuRec &r = rec[c];
        flags[row0 + lr] = o == 15 ? 0 : (r.word >> (48 + o)) & ((1ull << (15 - o)) - 1);
        {
            u64 v = rc_fill;
            if ((o & 3) == 0 && o != 12) v = (r.word >> (o == 0 ? 0 : o == 4 ? 32 : 16)) & 0xffff;       // off_dst, off_op1, off_op0 at 0, 4, 8
            else if ((o & 3) == 3) v = o == 3 ? r.ap : o == 7 ? r.mul : o == 11 ? r.fp : r.res;
            rc[row0 + lr] = v;
        }
        aux[row0 + lr] = o == 0 ? (r.jnz ? r.val[REC_DST] : 0) : o == 8 ? r.tmp1 : 0;
        {
            const u32 j = o >> 1, odd = o & 1;
            u64 v;
            if (j & 1) v = (j == 1 || j == 5) ? 0 : odd ? pad_value : 1;
            else { const u32 k = j == 0 ? REC_PC : j == 2 ? REC_OP0 : j == 4 ? REC_DST : REC_OP1; v = odd ? r.val[k] : r.addr[k]; }
            npc[row0 + lr] = v;
        }
    }
    for (u32 it = 0; it < 8; ++it) {
        const u32 lp = it * CPU_CYC + t, c = lp >> 3, j = lp & 7;
        if (c >= live) break;
        u32 a;
        if (j & 1) a = (j == 1 || j == 5) ? 0u : 1u;
        else a = rec[c].addr[j == 0 ? REC_PC : j == 2 ? REC_OP0 : j == 4 ? REC_DST : REC_OP1];
        pool_addr[cyc0 * 8 + lp] = a;
    }
}

// per cycle: its four ordered values at rows 4 j + 2 and ONE padding value at row 12 - every cycle, where the 252-bit layouts take one
// on odd cycles (plain/trace.rs: RangeCheck::Unused has step CYCLE_HEIGHT); then rc_hi forever
__global__ __launch_bounds__(256) void trace_gl64_rc_pool_kernel(TraceRcPlan p, const u32 *__restrict__ first, const uint16_t *__restrict__ padding, u64 num_cycles,
                                                                 u64 *__restrict__ rc) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g < num_cycles * 4) rc[(g >> 2) * 16 + (g & 3) * 4 + 2] = run_value(first, p.rc_hi - p.rc_lo + 1, p.rc_lo, g, p.rc_hi);
    else if (g < num_cycles * 5) { const u64 c = g - num_cycles * 4; rc[c * 16 + 12] = rc_padding(p, padding, p.pad0 + c); }
}

// the three kernels of the ordered memory that read or write cell values, over one-word cells (the others know addresses only)
constexpr u32 GL_GAP_OFF = 14;               // Npc::GapAddr / GapVal: rows 14, 15 of a cycle
__global__ __launch_bounds__(256) void mem_gap_fill_gl64_kernel(const u32 *__restrict__ gap_index, u32 cap, u64 num_cycles, u32 *__restrict__ count, u32 *__restrict__ rep,
                                                                u64 *__restrict__ npc, u32 *__restrict__ pool_addr, u32 *status) {
    const u32 a = blockIdx.x * 256 + threadIdx.x;
    if (a > cap) return;
    const u32 top = status[TRACE_ST_TOP], low = ~status[TRACE_ST_NLOW];
    if (!(a > low && a < top && a >= 2 && count[a] == 0)) return;
    const u32 g = gap_index[a];
    if (g >= num_cycles) { status_error(status, TRACE_ERR_TOO_MANY_GAPS, a); return; }
    const u64 row = (u64)g * 16 + GL_GAP_OFF;
    npc[row] = a;
    npc[row + 1] = 0;
    pool_addr[row >> 1] = a;
    count[a] = 1;
    rep[a] = (u32)(row >> 1);
}
__device__ __forceinline__ u64 mem_value_of_gl64(u32 idx, u64 half, const u64 *npc, const u64 *pub_value) {
    return idx < half ? npc[2 * (u64)idx + 1] : pub_value[idx - half];
}
__global__ __launch_bounds__(256) void mem_check_gl64_kernel(const u32 *__restrict__ pool_addr, u64 half, const u32 *__restrict__ pub_addr, u32 n_pub,
                                                             const u64 *__restrict__ pub_value, u64 pad_value, const u32 *__restrict__ rep, const u64 *__restrict__ npc,
                                                             u32 cap, u32 *status) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= half + n_pub) return;
    const u32 a = j < half ? pool_addr[j] : pub_addr[j - half];
    if (a == 0 || a > cap) return;
    const u64 mine = mem_value_of_gl64((u32)j, half, npc, pub_value);
    const u64 want = a == 1 ? pad_value : mem_value_of_gl64(rep[a], half, npc, pub_value);
    if (mine != want) status_error(status, TRACE_ERR_NOT_SINGLE_VALUED, a);
}
__global__ __launch_bounds__(256) void mem_fill_gl64_kernel(const u32 *__restrict__ start, u64 half, u32 cap, const u32 *__restrict__ rep, const u64 *__restrict__ npc,
                                                            const u64 *__restrict__ pub_value, u64 pad_value, u64 *__restrict__ mem_col, u32 *status) {
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    u32 top = status[TRACE_ST_TOP];
    if (top > cap) top = cap;
    u64 av = 0, vv = 0;
    if (j >= start[top + 1]) {                                       // the runs do not fill the column
        status_error(status, TRACE_ERR_FILL, top);
    } else {
        u32 a = 0, b = top + 1;                                      // start[a] <= j < start[b]
        while (b - a > 1) { const u32 m = (a + b) >> 1; if (start[m] <= j) a = m; else b = m; }
        av = a;
        vv = a <= 1 ? pad_value : mem_value_of_gl64(rep[a], half, npc, pub_value);
    }
    mem_col[2 * j] = av;
    mem_col[2 * j + 1] = vv;
}

inline dim3 grid_for(u64 lanes, u32 block) { return dim3((u32)((lanes + block - 1) / block)); }

}  // namespace

hipError_t launch_trace_memory_image(hipStream_t st, const u64 *d_records, u64 n_records, u64 *d_image, u64 cells) {
    hipError_t e = hipMemsetAsync(d_image, 0xff, cells * 32, st);
    if (e != hipSuccess || !n_records) return e;
    hipLaunchKernelGGL(trace_memory_image_kernel, grid_for(n_records, 256), dim3(256), 0, st, d_records, n_records, d_image, cells);
    return hipGetLastError();
}
hipError_t launch_trace_cpu(hipStream_t st, const TraceLayout &L, const u64 *d_states, u64 num_cycles, const u64 *d_image, u64 cells, const Fp &pad_value,
                            u64 rc_fill, Fp *flags, Fp *npc, Fp *rc, Fp *aux, u32 *d_pool_addr, u32 *d_status) {
    hipLaunchKernelGGL(trace_cpu_kernel, grid_for(num_cycles, CPU_CYC), dim3(CPU_CYC), 0, st, L, d_states, num_cycles, d_image, cells, pad_value,
                       fp_from_u64(rc_fill), flags, npc, rc, aux, d_pool_addr, d_status);
    return hipGetLastError();
}
hipError_t launch_trace_tile(hipStream_t st, const ColPtrs &cols, u32 ncols, const TraceTileEntry *d_entries, u32 n_entries, const Fp *d_values, u32 n_templates,
                             const u32 *d_tmpl_of_block, u64 nblocks, u64 step, u64 addr_begin, u64 addr_mult, u32 *d_pool_addr) {
    if (!nblocks || !n_entries) return hipSuccess;
    hipLaunchKernelGGL(trace_tile_kernel, grid_for(nblocks * n_entries, 256), dim3(256), 0, st, cols, ncols, d_entries, n_entries, d_values, n_templates,
                       d_tmpl_of_block, nblocks, step, addr_begin, addr_mult, d_pool_addr);
    return hipGetLastError();
}
hipError_t launch_trace_pedersen(hipStream_t st, const ColPtrs &cols, const TracePedersenLayout &L, const u64 *d_instances, u64 n_given, u64 n_blocks, u64 block_rows,
                                 u64 addr_begin, const Fp *d_points, u32 *d_pool_addr, u32 *d_status) {
    if (!n_given) return hipSuccess;
    hipLaunchKernelGGL(trace_pedersen_sums_kernel, grid_for(n_given, 64), dim3(64), 0, st, cols, L, d_instances, n_given, n_blocks, block_rows, d_points, d_status);
    hipLaunchKernelGGL(trace_pedersen_rows_kernel, dim3((u32)n_given), dim3(PED_STEPS), 0, st, cols, L, d_instances, n_blocks, block_rows, addr_begin, d_points, d_pool_addr);
    return hipGetLastError();
}
hipError_t launch_trace_bitwise(hipStream_t st, const ColPtrs &cols, const TraceBitwiseLayout &L, const u64 *d_instances, u64 n_given, u64 n_blocks, u64 block_rows,
                                u64 addr_begin, u32 what, u32 *d_pool_addr, u32 *d_status) {
    if (!n_given) return hipSuccess;
    hipLaunchKernelGGL(trace_bitwise_kernel, grid_for(n_given * BW_LANES, 256), dim3(256), 0, st, cols, L, d_instances, n_given, n_blocks, block_rows, addr_begin, what,
                       d_pool_addr, d_status);
    return hipGetLastError();
}
hipError_t launch_trace_poseidon(hipStream_t st, const ColPtrs &cols, const TracePoseidonLayout &L, const Fp *d_round_keys, const u64 *d_instances, u64 n_given,
                                 u64 n_blocks, u64 block_rows, u64 addr_begin, u32 *d_pool_addr, u32 *d_status) {
    if (!n_given) return hipSuccess;
    hipLaunchKernelGGL(trace_poseidon_kernel, grid_for(n_given, 64), dim3(64), 0, st, cols, L, d_round_keys, d_instances, n_given, n_blocks, block_rows, addr_begin,
                       d_pool_addr, d_status);
    return hipGetLastError();
}
hipError_t launch_trace_ec_op(hipStream_t st, const ColPtrs &cols, const TraceEcOpLayout &L, const u64 *d_instances, u64 n_given, u64 n_blocks, u64 block_rows,
                              u64 addr_begin, u32 *d_pool_addr, u32 *d_status) {
    if (!n_given) return hipSuccess;
    hipLaunchKernelGGL(trace_ec_op_kernel, dim3((u32)n_given), dim3(EC_LANES), 0, st, cols, L, d_instances, n_blocks, block_rows, addr_begin, d_pool_addr, d_status);
    return hipGetLastError();
}
hipError_t launch_trace_ecdsa(hipStream_t st, const ColPtrs &cols, const TraceEcdsaLayout &L, const Fp *d_points, const u64 *d_instances, u64 n_given, u64 n_blocks,
                              u64 block_rows, u64 addr_begin, u32 *d_pool_addr, u32 *d_status) {
    if (!n_given) return hipSuccess;
    hipLaunchKernelGGL(trace_ecdsa_kernel, dim3((u32)n_given), dim3(EC_LANES), 0, st, cols, L, d_points, d_instances, n_blocks, block_rows, addr_begin, d_pool_addr, d_status);
    return hipGetLastError();
}
hipError_t launch_trace_rc_builtin(hipStream_t st, const TraceRcPlan &p, const u64 *d_given, const uint16_t *d_padding, Fp *rc, Fp *npc, u32 *d_pool_addr) {
    if (!p.n_slots) return hipSuccess;
    hipLaunchKernelGGL(trace_rc_builtin_kernel, grid_for(p.n_slots, 256), dim3(256), 0, st, p, d_given, d_padding, rc, npc, d_pool_addr);
    return hipGetLastError();
}
hipError_t launch_trace_rc_pool(hipStream_t st, const TraceRcPlan &p, const u32 *d_first, const uint16_t *d_padding, u64 num_cycles, Fp *rc) {
    hipLaunchKernelGGL(trace_rc_pool_kernel, grid_for(num_cycles * (16 / p.ordered_step) + num_cycles / 2, 256), dim3(256), 0, st, p, d_first, d_padding, num_cycles, rc);
    return hipGetLastError();
}
hipError_t launch_trace_runs(hipStream_t st, Fp *col, u64 stride, u64 off, u64 slots, const u32 *d_first, u32 n_values, u32 lo, bool diluted) {
    if (!slots) return hipSuccess;
    hipLaunchKernelGGL(trace_runs_kernel, grid_for(slots, 256), dim3(256), 0, st, col, stride, off, slots, d_first, n_values, lo, diluted ? 1u : 0u);
    return hipGetLastError();
}
hipError_t launch_trace_patch(hipStream_t st, Fp *col, u64 col_rows, const u64 *d_rows, const u64 *d_values, u64 count) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(trace_patch_kernel, grid_for(count, 256), dim3(256), 0, st, col, col_rows, d_rows, d_values, count);
    return hipGetLastError();
}

// scratch (u32 words): count, rep, start (cap + 2 each), the scans' chunk sums
uint64_t trace_memory_scratch_words(u64 half) {
    const u64 cap = half;
    return 3 * (cap + 2) + 2 * ((cap + 2 + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) + 16;
}
hipError_t launch_trace_ordered_memory(hipStream_t st, const TraceMemoryArgs &m, u32 *scratch) {
    const u64 half = m.n / 2;
    const u32 cap = (u32)half;                // continuous memory has an access per address 1 .. top and n / 2 accesses in all
    u32 *count = scratch, *rep = count + (cap + 2), *start = rep + (cap + 2), *sums = start + (cap + 2);
    hipError_t e;
    if ((e = hipMemsetAsync(count, 0, (size_t)(cap + 2) * 4, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(rep, 0xff, (size_t)(cap + 2) * 4, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(mem_count_kernel, grid_for(half, MEM_LANES * MEM_PER), dim3(MEM_LANES), 0, st, (const u32 *)m.d_pool_addr, half, cap, count, rep, m.d_status);
    if (m.n_public) hipLaunchKernelGGL(mem_public_kernel, grid_for(m.n_public, 256), dim3(256), 0, st, m.d_public_addr, m.n_public, half, cap, count, rep, m.d_status);
    // gaps: flags -> their rank among the gaps (start[] as the temporary) -> the pool pairs
    hipLaunchKernelGGL(mem_gap_flags_kernel, grid_for((u64)cap + 1, 256), dim3(256), 0, st, (const u32 *)count, cap, (const u32 *)m.d_status, start);
    if ((e = exclusive_scan_u32(st, start, (u64)cap + 1, sums, m.d_status + TRACE_ST_GAPS)) != hipSuccess) return e;
    hipLaunchKernelGGL(mem_gap_fill_kernel, grid_for((u64)cap + 1, 256), dim3(256), 0, st, (const u32 *)start, cap, m.n / 16, m.unused_off, count, rep, m.npc,
                       m.d_pool_addr, m.d_status);
    hipLaunchKernelGGL(mem_check_kernel, grid_for(half + m.n_public, 256), dim3(256), 0, st, (const u32 *)m.d_pool_addr, half, m.d_public_addr, m.n_public,
                       m.d_public_value, m.pad_value, (const u32 *)rep, (const Fp *)m.npc, cap, m.d_status);
    hipLaunchKernelGGL(mem_starts_kernel, grid_for((u64)cap + 2, 256), dim3(256), 0, st, (const u32 *)count, cap, m.public_cells, m.n_public, m.d_status, start);
    if ((e = exclusive_scan_u32(st, start, (u64)cap + 2, sums, nullptr)) != hipSuccess) return e;
    hipLaunchKernelGGL(mem_fill_total_kernel, dim3(1), dim3(64), 0, st, (const u32 *)start, half, cap, m.d_status);
    hipLaunchKernelGGL(mem_fill_kernel, grid_for(half, 256), dim3(256), 0, st, (const u32 *)start, half, cap, (const u32 *)rep, (const Fp *)m.npc, m.d_public_value,
                       m.pad_value, m.memory, m.d_status);
    return hipGetLastError();
}

// ---- the plain layout over the 64-bit field
hipError_t launch_trace_gl64_memory_image(hipStream_t st, const u64 *d_records, u64 n_records, u64 *d_image, u64 cells) {
    hipError_t e = hipMemsetAsync(d_image, 0xff, cells * 8, st);
    if (e != hipSuccess || !n_records) return e;
    hipLaunchKernelGGL(trace_gl64_memory_image_kernel, grid_for(n_records, 256), dim3(256), 0, st, d_records, n_records, d_image, cells);
    return hipGetLastError();
}
hipError_t launch_trace_gl64_cpu(hipStream_t st, const u64 *d_states, u64 num_cycles, const u64 *d_image, u64 cells, u64 pad_value, u64 rc_fill, u64 *flags, u64 *npc,
                                 u64 *rc, u64 *aux, u32 *d_pool_addr, u32 *d_status) {
    hipLaunchKernelGGL(trace_gl64_cpu_kernel, grid_for(num_cycles, CPU_CYC), dim3(CPU_CYC), 0, st, d_states, num_cycles, d_image, cells, pad_value, rc_fill, flags, npc,
                       rc, aux, d_pool_addr, d_status);
    return hipGetLastError();
}
hipError_t launch_trace_gl64_rc_pool(hipStream_t st, const TraceRcPlan &p, const u32 *d_first, const uint16_t *d_padding, u64 num_cycles, u64 *rc) {
    hipLaunchKernelGGL(trace_gl64_rc_pool_kernel, grid_for(num_cycles * 5, 256), dim3(256), 0, st, p, d_first, d_padding, num_cycles, rc);
    return hipGetLastError();
}
// the pipeline of launch_trace_ordered_memory, kernel for kernel; scratch as there (trace_memory_scratch_words)
hipError_t launch_trace_gl64_ordered_memory(hipStream_t st, const TraceGl64MemoryArgs &m, u32 *scratch) {
    const u64 half = m.n / 2;
    const u32 cap = (u32)half;
    u32 *count = scratch, *rep = count + (cap + 2), *start = rep + (cap + 2), *sums = start + (cap + 2);
    hipError_t e;
    if ((e = hipMemsetAsync(count, 0, (size_t)(cap + 2) * 4, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(rep, 0xff, (size_t)(cap + 2) * 4, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(mem_count_kernel, grid_for(half, MEM_LANES * MEM_PER), dim3(MEM_LANES), 0, st, (const u32 *)m.d_pool_addr, half, cap, count, rep, m.d_status);
    if (m.n_public) hipLaunchKernelGGL(mem_public_kernel, grid_for(m.n_public, 256), dim3(256), 0, st, m.d_public_addr, m.n_public, half, cap, count, rep, m.d_status);
    hipLaunchKernelGGL(mem_gap_flags_kernel, grid_for((u64)cap + 1, 256), dim3(256), 0, st, (const u32 *)count, cap, (const u32 *)m.d_status, start);
    if ((e = exclusive_scan_u32(st, start, (u64)cap + 1, sums, m.d_status + TRACE_ST_GAPS)) != hipSuccess) return e;
    hipLaunchKernelGGL(mem_gap_fill_gl64_kernel, grid_for((u64)cap + 1, 256), dim3(256), 0, st, (const u32 *)start, cap, m.n / 16, count, rep, m.npc, m.d_pool_addr,
                       m.d_status);
    hipLaunchKernelGGL(mem_check_gl64_kernel, grid_for(half + m.n_public, 256), dim3(256), 0, st, (const u32 *)m.d_pool_addr, half, m.d_public_addr, m.n_public,
                       m.d_public_value, m.pad_value, (const u32 *)rep, (const u64 *)m.npc, cap, m.d_status);
    hipLaunchKernelGGL(mem_starts_kernel, grid_for((u64)cap + 2, 256), dim3(256), 0, st, (const u32 *)count, cap, m.n / 8, m.n_public, m.d_status, start);
    if ((e = exclusive_scan_u32(st, start, (u64)cap + 2, sums, nullptr)) != hipSuccess) return e;
    hipLaunchKernelGGL(mem_fill_total_kernel, dim3(1), dim3(64), 0, st, (const u32 *)start, half, cap, m.d_status);
    hipLaunchKernelGGL(mem_fill_gl64_kernel, grid_for(half, 256), dim3(256), 0, st, (const u32 *)start, half, cap, (const u32 *)rep, (const u64 *)m.npc, m.d_public_value,
                       m.pad_value, m.memory, m.d_status);
    return hipGetLastError();
}

}  // namespace ss
