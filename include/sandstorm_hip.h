/* sandstorm_hip.h — C ABI of libsandstorm_hip.so
 *
 * The MI355X (gfx950) proving backend that slots behind Sandstorm's
 * `sandstorm-cli prove` / ministark prover API.  The reference has no FFI for
 * this path: its seams are Rust traits.  Each entry point below
 * is what a `hip` cargo feature of ministark would bind in place of its Metal
 * `gpu` feature, and cites the reference interface it replaces.  See
 * INTEGRATION.md for the Rust-side `extern "C"` block.
 *
 * Conventions
 *  - Field element: 4 x u64 little-endian limbs, Montgomery form, R = 2^256,
 *    p = 2^251 + 17*2^192 + 1 — the in-memory image of the reference's `Fp`
 *    (crypto/src/utils.rs:8-22).  "felt" below always means this 32-byte image.
 *  - A matrix is column-major: one contiguous device array per column
 *    (ministark `Matrix<F>` = Vec<GpuVec<F>>; layouts/src/recursive/trace.rs:652-660).
 *    `cols` arguments are HOST arrays of DEVICE pointers.
 *  - Digest: 32 raw bytes.  MixedMerkleDigest (crypto/src/merkle/mixed.rs:34-71)
 *    additionally carries a tag byte: 0 = HighLevel (Pedersen felt as 32-byte
 *    big-endian canonical, hash/pedersen.rs:23-28), 1 = LowLevel (Blake2s).
 *  - Every pointer named d_* is device memory (from ss_dev_alloc, hipMalloc or a
 *    torch tensor's data_ptr); every other pointer is host memory owned by the
 *    caller for the duration of the call.
 *  - Work is enqueued on the context's HIP stream; calls that return host data
 *    synchronise that stream, the others do not (use ss_ctx_sync).
 *  - Errors: integer status, never an exception/abort across the ABI; the text
 *    is in ss_last_error() (thread-local).  The reference panics on any error
 *    (cli/src/main.rs:201 `unwrap`), so a Rust shim `expect()`s on non-zero.
 *  - One ctx per host thread and per GPU; no global mutable state.
 */
#ifndef SANDSTORM_HIP_H
#define SANDSTORM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every entry point validates what it is handed before anything is launched - sizes, directions / orders / hash, tree, leaf and coin
 * kinds, NULL tables and NULL entries of column tables, mask cells and program operands against the column / constant / slot /
 * table counts of the same call, query indices against the tree - and answers SS_ERR_INVALID / SS_ERR_UNSUPPORTED with a message in
 * ss_last_error(); a call it cannot serve never reaches a kernel (tests/hipemu/extra_bad_arguments.py sweeps all of them).  What
 * it cannot check is the SIZE of device memory behind a pointer: buffers must hold what the call's sizes say. */
typedef int ss_status;
enum {
    SS_OK = 0,
    SS_ERR_INVALID = 1,     /* bad argument */
    SS_ERR_HIP = 2,         /* HIP runtime error, see ss_last_error */
    SS_ERR_NO_DEVICE = 3,   /* no gfx950 device / HIP extension unusable */
    SS_ERR_UNSUPPORTED = 4
};

typedef struct ss_ctx ss_ctx;

/* NTT direction / element order */
enum { SS_NTT_FORWARD = 0, SS_NTT_INVERSE = 1 };
enum { SS_ORDER_NATURAL = 0, SS_ORDER_BITREV = 1 };

/* HashFn implementations of crypto/src/hash/{keccak,blake2s}.rs */
enum {
    SS_HASH_KECCAK = 0,       /* Keccak256HashFn           keccak.rs:13-59  */
    SS_HASH_KECCAK_M20 = 1,   /* MaskedKeccak256HashFn<20> keccak.rs:61-98  */
    SS_HASH_BLAKE2S = 2,      /* Blake2sHashFn             blake2s.rs:10-62 */
    SS_HASH_BLAKE2S_M20 = 3,  /* MaskedBlake2sHashFn<20>   blake2s.rs:64-100 */
    SS_HASH_SHA256 = 4        /* ministark's Sha256HashFn (cli/src/main.rs:105,119: the 64-bit field's claim); FIPS 180-4; ss_hash_rows_gl64 only */
};
/* Merkle tree types chosen by src/claims.rs:12-33 */
enum {
    SS_TREE_KECCAK = 0,       /* LeafVariantMerkleTree<Keccak256HashFn>           */
    SS_TREE_KECCAK_M20 = 1,   /* LeafVariantMerkleTree<MaskedKeccak256HashFn<20>> */
    SS_TREE_FRIENDLY = 2,     /* FriendlyMerkleTree<N, PedersenHashFn>            */
    SS_TREE_BLAKE2S = 3,      /* MatrixMerkleTree over Blake2sHashFn (blake2s.rs:10-62): the 64-bit field's trees here */
    SS_TREE_SHA256 = 4        /* MatrixMerkleTreeImpl<Sha256HashFn> (cli/src/main.rs:119): node = SHA-256(left || right), digests as leaves */
};
enum { SS_LEAF_DIGEST = 0, SS_LEAF_FELT = 1 };
enum { SS_COIN_SOLIDITY = 0, SS_COIN_CAIRO = 1 };

const char *ss_last_error(void);
/* ABI version of this header; bump on any signature change.  ss_abi_version() of the loaded
 * library must equal SS_ABI_VERSION of the header the caller was built against. */
#define SS_ABI_VERSION 12u
uint32_t ss_abi_version(void);

/* ---- context & memory (replaces ministark-gpu's Metal planner/GpuAllocator;
 *      call sites src/lib.rs:27-28, layouts/src/recursive/trace.rs:115-120) */
ss_status ss_ctx_create(int device, ss_ctx **out);
void ss_ctx_destroy(ss_ctx *ctx);
ss_status ss_ctx_set_stream(ss_ctx *ctx, void *hip_stream); /* NULL = ctx-owned stream */
ss_status ss_ctx_sync(ss_ctx *ctx);       /* waits for the ctx stream and for the copy stream of ss_upload_async */
/* ss_dev_alloc/ss_dev_free are pooled (the role of GpuAllocator / PageAlignedAllocator,
 * src/lib.rs:27-28): a freed block is kept for reuse by later allocations of a similar size
 * on the same context, so steady-state proving makes no hipMalloc/hipFree calls.
 * ss_ctx_trim returns the cached blocks to the driver, and with them the Pedersen window tables that no context of the process
 * uses any more.  (Memory a process holds besides its buffers: twiddle plans, 36 B per point and (size, direction, offset);
 * for FriendlyMerkleTree claims ONE fixed-base window table per device and process - 23.6 GB at the default 24-bit windows,
 * narrower windows (6.4 / 1.75 / 0.47 / 0.13 GB) when the device's free memory does not leave 4 GiB beside it or SS_PED_WINDOW
 * says so; built at the first friendly tree in ~0.1 s.) */
ss_status ss_dev_alloc(ss_ctx *ctx, size_t bytes, void **d_out);
ss_status ss_dev_free(ss_ctx *ctx, void *d_ptr);
ss_status ss_ctx_trim(ss_ctx *ctx);
ss_status ss_upload(ss_ctx *ctx, void *d_dst, const void *src, size_t bytes);
ss_status ss_download(ss_ctx *ctx, void *dst, const void *d_src, size_t bytes);
/* Upload without the wait: the copy is enqueued on a copy stream of the context's own and returns at once (src: pinned host memory
 * that stays untouched until the copy is done - the `GpuAllocator` seam, layouts/src/recursive/trace.rs:115-120); *ticket names it.
 * ss_wait_upload(ctx, ticket) orders everything enqueued on the context's stream AFTERWARDS behind that copy (a stream wait: the
 * host does not block); a ticket is waited for once.  ss_upload_async may be called from another host thread than the one that
 * drives the context - the trace generator's, which uploads a column the moment no section will write it again, while the prover
 * already extends the columns that have arrived (`Stark::prove` starts from the witness: src/lib.rs:94-100). */
ss_status ss_upload_async(ss_ctx *ctx, void *d_dst, const void *src, size_t bytes, uint64_t *ticket);
ss_status ss_wait_upload(ss_ctx *ctx, uint64_t ticket);
/* zero-fill on the ctx stream (`Vec::resize(trace_len, Fp::ZERO)`, layouts/src/recursive/trace.rs:741-748) */
ss_status ss_dev_zero(ss_ctx *ctx, void *d_ptr, size_t bytes);

/* ---- data movement of the sharded driver (ABI 7; DESIGN.md section 6: nothing in the reference to replace - its
 * parallelism is rayon loops in one address space, crypto/src/merkle/utils.rs:30-32).  All on the ctx stream, no host sync. */
/* device -> device */
ss_status ss_dev_copy(ss_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* `rows` runs of `width` bytes: row r from d_src + r * src_pitch to d_dst + r * dst_pitch (the stride-R comb of a leaf block) */
ss_status ss_dev_copy_2d(ss_ctx *ctx, void *d_dst, size_t dst_pitch, const void *d_src, size_t src_pitch, size_t width, size_t rows);
/* 32-byte elements: d_dst[bitrev(i)] = d_src[i], i < 2^log_n (a single column's leaves in the commitment order); not in place */
ss_status ss_bitrev_permute32(ss_ctx *ctx, const void *d_src, uint32_t log_n, void *d_dst);

/* One communicator per rank over RCCL (loaded with dlopen at the first call: a process that never shards does not need the
 * library).  Rank 0 makes the 128-byte id (ss_comm_unique_id) and hands it to the other ranks by whatever launched them; every
 * rank then calls ss_comm_create on its own context.  The exchanges run on the context's stream. */
typedef struct ss_comm ss_comm;
ss_status ss_comm_unique_id(uint8_t id_out[128]);
ss_status ss_comm_create(ss_ctx *ctx, const uint8_t id[128], uint32_t rank, uint32_t world, ss_comm **out);
void ss_comm_destroy(ss_comm *comm);
/* One exchange step that EVERY rank enters: message i of this rank goes from d_send[i] (send_bytes[i] bytes) to rank
 * send_peer[i]; message j arrives from rank recv_peer[j] in d_recv[j].  The messages of one ordered pair of ranks are matched
 * in list order (messages to the own rank are device copies); either list may be empty.  ONE grouped ncclSend / ncclRecv
 * batch - on xGMI each pair of GPUs has its own link, so the R (R - 1) transfers of a re-shard run concurrently, no ring. */
ss_status ss_comm_exchange(ss_comm *comm, uint32_t nsend, const uint32_t *send_peer, const void *const *d_send, const uint64_t *send_bytes,
                           uint32_t nrecv, const uint32_t *recv_peer, void *const *d_recv, const uint64_t *recv_bytes);
/* `bytes` bytes of every rank, in rank order, into d_recv (world * bytes) */
ss_status ss_comm_all_gather(ss_comm *comm, const void *d_send, uint64_t bytes, void *d_recv);

/* ---- N1/N2: ministark Matrix::interpolate / Matrix::evaluate (un-vendored;
 *      call sites src/lib.rs:17-26; convention pinned by
 *      builtins/src/pedersen/periodic.rs:1183-1209).
 * In-place NTT of `ncols` columns of 2^log_n felts over offset*<w>, w =
 * 3^((p-1)/2^log_n).  FORWARD: coefficients -> evaluations; INVERSE:
 * evaluations -> coefficients (includes 1/n and offset^-i).  `offset` is a
 * Montgomery felt (NULL = 1).  in_order/out_order select natural or
 * bit-reversed indexing of the array on entry/exit. */
ss_status ss_ntt_fp252(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint32_t log_n,
                       int direction, const uint64_t offset[4], int in_order, int out_order);

/* Low-degree extension of `ncols` columns (pipeline steps 3+4 / 8 / 10 of
 * SURVEY §3.1): interpolate over <w_n>, evaluate over offset*<w_{n*2^log_blowup}>.
 * d_evals[c]: 2^(log_n+log_blowup) felts, natural order.
 * d_coeffs (may be NULL) / d_coeffs[c]: 2^log_n felts, the interpolant's
 * coefficients in BIT-REVERSED index order (kept for OOD/DEEP). d_in may alias
 * d_coeffs column-wise, never d_evals. */
ss_status ss_lde_fp252(ss_ctx *ctx, const uint64_t *const *d_in, uint32_t ncols, uint32_t log_n,
                       uint32_t log_blowup, const uint64_t offset[4], uint64_t *const *d_evals,
                       uint64_t *const *d_coeffs);

/* Evaluate-only half of the LDE (pipeline step 10: the composition columns, whose
 * coefficients come from one inverse NTT): d_coeffs[c] holds 2^log_n coefficients
 * in BIT-REVERSED order; d_evals[c] receives the 2^(log_n+log_blowup) evaluations
 * over offset*<w>, natural order.  d_coeffs is not modified. */
ss_status ss_evaluate_fp252(ss_ctx *ctx, const uint64_t *const *d_coeffs, uint32_t ncols, uint32_t log_n,
                            uint32_t log_blowup, const uint64_t offset[4], uint64_t *const *d_evals);

/* Every 2^log_stride-th row of `ncols` columns as contiguous columns: d_out[c][j] = d_in[c][j << log_stride], j < nrows_out, 32-byte
 * cells.  With an LDE blowup above 2 (`--lde-blowup-factor`, cli/src/main.rs:53-54) the composition constraint, of degree
 * ce_blowup_factor = 2 (src/lib.rs:110), is still evaluated on the 2n-point coset offset*<w_2n> only: rows j << (log_blowup - 1) of the
 * LDE, which this call hands to ss_eval_quotient / ss_eval_quotient_rows as columns of log_blowup = 1.  nrows_out is arbitrary (a row
 * block plus its halo); d_in[c] holds at least ((nrows_out - 1) << log_stride) + 1 cells, d_out[c] nrows_out, and nothing beyond them is
 * written; the two do not overlap.  log_stride <= 4; any ncols (16 columns a launch).  On the ctx stream, no host sync. */
ss_status ss_subsample_rows(ss_ctx *ctx, const uint64_t *const *d_in, uint32_t ncols, uint64_t nrows_out, uint32_t log_stride,
                            uint64_t *const *d_out);

/* ---- (e) ONE transform spread over R = 2^log_ranks GPUs (nothing in the reference to match: its
 * Matrix::interpolate / evaluate run in one address space, src/lib.rs:17-26).  A rank holds the contiguous block
 * [rank n/R, (rank+1) n/R) of the array.  The network's log2(n/R) stages that pair elements less than n/R apart never leave
 * a block (part LOCAL: on the rank's block, a buffer of n/R felts); its log_ranks stages that pair element x of block b with
 * element x of another block run after ONE equal-split all-to-all (ss_comm_exchange: chunk m of every block to rank m) has
 * given rank m the x-range [m n/R^2, (m+1) n/R^2) of EVERY block, block after block in a buffer of n/R felts (part CROSS).
 *   INVERSE (natural in, bit-reversed out, 1/n and offset^-j included):  CROSS on the exchanged layout, exchange back, LOCAL
 *   FORWARD (bit-reversed in, natural out):  LOCAL on the block, exchange, CROSS; the caller exchanges back if it wants blocks.
 * log_n = log2 of the WHOLE transform, n >= R^2.  log_expand (FORWARD LOCAL only): the block's input is the 2^-log_expand
 * sub-sampled coefficient block (n/R >> log_expand felts in d_cols[c]; d_out[c]: n/R felts) - the zero-padded half of an
 * LDE is not materialised.  d_out = NULL: in place.  Everything is bit-identical to ss_ntt_fp252 / ss_evaluate_fp252 on the
 * gathered array (tests/test_gpu_parity.py::test_ntt_spread_over_ranks). */
enum { SS_NTT_PART_LOCAL = 0, SS_NTT_PART_CROSS = 1 };
ss_status ss_ntt_shard_fp252(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint32_t log_n, uint32_t log_ranks,
                             uint32_t rank, int direction, const uint64_t offset[4], int part, uint32_t log_expand,
                             uint64_t *const *d_out);

/* ---- H1: crypto/src/merkle/utils.rs:19-46 hash_rows::<H>.
 * d_digests[r] = H::hash_elements(row r) for r < nrows; rows are read in
 * natural index order from the column arrays. */
ss_status ss_hash_rows(ss_ctx *ctx, int hash_kind, const uint64_t *const *d_cols, uint32_t ncols,
                       uint64_t nrows, uint8_t *d_digests);
/* The same with the leaf order of the reference's proofs: row_order = SS_ORDER_BITREV makes digest i the hash of
 * matrix row bitrev(i) (index i of a committed vector is the point offset * w^bitrev(i): pinned by
 * tests/golden/make_proof_golden.py).  The matrix stays in natural order - nothing is permuted in memory. */
ss_status ss_hash_rows_ex(ss_ctx *ctx, int hash_kind, const uint64_t *const *d_cols, uint32_t ncols,
                       uint64_t nrows, int row_order, uint8_t *d_digests);

/* ---- H2/H3/H4: MatrixMerkleTree::from_matrix tree build
 *      (crypto/src/merkle/mod.rs:110-123, 289-304; node rules mixed.rs:106-155,
 *      mod.rs:419-437; builder ministark MerkleTreeImpl::new, un-vendored).
 * leaves: n digests (SS_LEAF_DIGEST) or n felts (SS_LEAF_FELT, single-column
 * matrices).  d_nodes: 2n x 32 bytes, heap layout: node k has children 2k,
 * 2k+1; root at index 1; leaf i at n+i (felt leaves stored as Montgomery-BE
 * bytes).  d_tags (SS_TREE_FRIENDLY only, may be NULL): 2n tag bytes.
 * root_out[0..32) digest, root_out[32] tag. */
ss_status ss_merkle_build(ss_ctx *ctx, int tree_kind, uint32_t n_friendly_layers, int leaf_kind,
                          const void *d_leaves, uint64_t n, uint8_t *d_nodes, uint8_t *d_tags,
                          uint8_t root_out[33]);
/* leaf_order = SS_ORDER_BITREV: for SS_LEAF_FELT the leaf slot i holds element bitrev(i) of the column (digest
 * leaves are taken as given - order them with ss_hash_rows_ex). */
ss_status ss_merkle_build_ex(ss_ctx *ctx, int tree_kind, uint32_t n_friendly_layers, int leaf_kind,
                          const void *d_leaves, uint64_t n, int leaf_order, uint8_t *d_nodes, uint8_t *d_tags,
                          uint8_t root_out[33]);
/* MerkleTree::prove: authentication paths for `nidx` leaf indices.
 * out: nidx * log2(n) sibling digests (leaf level first), 32 bytes each;
 * out_tags (may be NULL) the matching tag bytes. */
ss_status ss_merkle_open(ss_ctx *ctx, const uint8_t *d_nodes, const uint8_t *d_tags, uint64_t n,
                         const uint64_t *idx, uint32_t nidx, uint8_t *out, uint8_t *out_tags);
/* gather full rows `idx` of a column-major matrix to the host (query phase) */
ss_status ss_gather_rows(ss_ctx *ctx, const uint64_t *const *d_cols, uint32_t ncols,
                         const uint64_t *idx, uint32_t nidx, uint64_t *out /* nidx*ncols felts */);
/* The whole query phase in one round trip (ABI 10): every job gathers entries `idx` of `ncols` device arrays of `entry_bytes`-byte entries
 * (32: field elements or digests - the opened rows of a matrix, a tree's leaf digests, or authentication paths with idx = the sibling
 * node numbers over the node array as one "column"; 1: the tag bytes of a FriendlyMerkleTree's nodes, ncols = 1) into host memory
 * `out`, nidx * ncols entries, row after row - what ss_gather_rows / ss_merkle_open return, but one index upload, one download and one
 * synchronisation for all jobs (ministark's `Queries::new` - un-vendored, Cargo.lock:894-896 - with `MerkleTree::prove`,
 * crypto/src/merkle/mod.rs:258-304, over the three trace trees and every FRI layer: 27 calls of ~60 us each before).  Jobs with
 * nidx = 0 are skipped. */
typedef struct ss_gather_job {
    const void *const *d_cols;
    uint32_t ncols;
    uint32_t entry_bytes;      /* 32 or 1 */
    const uint64_t *idx;       /* host */
    uint32_t nidx;
    void *out;                 /* host: nidx * ncols * entry_bytes */
} ss_gather_job;
ss_status ss_gather_batch(ss_ctx *ctx, const ss_gather_job *jobs, uint32_t njobs);

/* ---- Q1: AirConfig::eval_constraint over the LDE domain (ministark default
 *      body; DAG built by layouts/src/{recursive,starknet}/air.rs).
 * The Rust side lowers its `Expr` DAG once per (layout, n) into this program
 * for a 4-accumulator register machine (two-address, one instruction = 2 x u32):
 *   word0: [7:0] opcode, [11:8] dst accumulator, [15:12] operand kind
 *   word1: operand payload
 * The program is executed once per LDE point i (x_i = offset * w_N^i). */
enum {
    SS_OP_MOV = 0,   /* acc[d] = src            */
    SS_OP_ADD = 1,   /* acc[d] = acc[d] + src   */
    SS_OP_SUB = 2,   /* acc[d] = acc[d] - src   */
    SS_OP_RSUB = 3,  /* acc[d] = src - acc[d]   */
    SS_OP_MUL = 4,   /* acc[d] = acc[d] * src   */
    SS_OP_INV = 5,   /* acc[d] = 1 / acc[d]  (0 -> 0), operand ignored */
    SS_OP_ST = 6,    /* slot[payload] = acc[d]  */
    SS_OP_OUT = 7,   /* out[i] = acc[d]         */
    SS_OP_CHECK = 10 /* check k = payload: acc[d] must be zero if this row is in domain k (ss_check_constraints and
                        ss_check_constraints_gl64x3 only; the ss_eval_quotient family refuses it; 8 and 9 are taken inside the library) */
};
enum {
    SS_SRC_ACC = 0,    /* payload = accumulator index                                  */
    SS_SRC_SLOT = 1,   /* payload = slot index (per-point scratch)                     */
    SS_SRC_CONST = 2,  /* payload = index into consts (challenges, hints, alpha^k ...) */
    SS_SRC_TRACE = 3,  /* payload = col << 24 | row_offset: lde[col][(i + (row_offset << log_blowup)) mod N] */
    SS_SRC_TABLE = 4,  /* payload = table index: tables[desc.offset + (i mod 2^desc.log_len)]
                          (periodic columns and X^(n/k) zerofier inverses are periodic in i) */
    SS_SRC_X = 5       /* x_i */
};
#define SS_INSTR(op, dst, kind, payload) ((uint32_t)(op) | ((uint32_t)(dst) << 8) | ((uint32_t)(kind) << 12)), ((uint32_t)(payload))
typedef struct ss_air_program {
    const uint32_t *code;        /* 2 * n_instr words (host) */
    uint32_t n_instr;
    const uint64_t *consts;      /* n_consts felts (host) */
    uint32_t n_consts;
    const uint64_t *d_tables;    /* device: concatenated tables of felts */
    const uint32_t *table_desc;  /* host: 2 * n_tables words: {offset in felts, log_len} */
    uint32_t n_tables;
    uint32_t n_slots;            /* scratch slots used by ST / SS_SRC_SLOT */
} ss_air_program;
/* Table of a single-point zerofier inverse over the whole LDE domain:
 * d_out[i] = 1 / (offset * w_N^i - c), i < 2^log_N (0 where the denominator is 0),
 * by Montgomery batch inversion.  The AIRs' first/last-row boundary terms
 * 1/(X - c) (e.g. layouts/src/recursive/air.rs:295-298) become TABLE operands of
 * length 2^log_N instead of a per-point field inversion. */
ss_status ss_inverse_table(ss_ctx *ctx, uint32_t log_N, const uint64_t offset[4], const uint64_t c[4],
                           uint64_t *d_out);
/* Copies of tables, each times a factor of its own, one after the other: with dst_j = len[0] + .. + len[j - 1],
 * d_out[dst_j + k] = d_tables[first[j] + k] * factors[j] for k < len[j] (first, len in felts; factors: n_copies interchange
 * images, host memory like first and len).  It is the launch ss_eval_quotient's compiled kernels queue in front of their parts -
 * the multiplier-only periodic tables times 2^24, and times each constraint's coefficient (csrc/quotient_derive.h) - as a call
 * of its own, for tests.  Every entry comes out fully reduced. */
ss_status ss_table_copies(ss_ctx *ctx, const uint64_t *d_tables, const uint32_t *first, const uint32_t *len,
                          const uint64_t *factors, uint32_t n_copies, uint64_t *d_out);
ss_status ss_eval_quotient(ss_ctx *ctx, const ss_air_program *prog, const uint64_t *const *d_lde_cols,
                           uint32_t ncols, uint32_t log_n, uint32_t log_blowup,
                           const uint64_t offset[4], uint64_t *d_out);
/* Row-block form, for one proof sharded over several GPUs (the reference has only rayon loops over
 * rows to replace, crypto/src/merkle/utils.rs:30-32).  The evaluation domain is cut into contiguous row blocks; a
 * rank evaluates points row0 .. row0 + nrows from column BLOCKS: d_col_blocks[c][k] = LDE row (row0 + k) mod N of
 * column c, k < block_rows, where block_rows >= nrows + (largest row offset of the program << log_blowup) - the rows
 * behind the block that its constraints reach (wrap-around included) travel with it.  Tables stay whole and are
 * indexed by the global row.  d_out[k] = what ss_eval_quotient writes at row0 + k, bit for bit. */
ss_status ss_eval_quotient_rows(ss_ctx *ctx, const ss_air_program *prog, const uint64_t *const *d_col_blocks,
                                uint32_t ncols, uint32_t log_n, uint32_t log_blowup, const uint64_t offset[4],
                                uint64_t row0, uint64_t nrows, uint64_t block_rows, uint64_t *d_out);

/* ---- a trace against its AIR, constraint by constraint (ministark runs `validate_constraints` over the trace in debug builds,
 *      before it commits to anything).  The program has one SS_OP_CHECK k per constraint and no SS_OP_OUT: the code in front of a
 * CHECK leaves that constraint's NUMERATOR in the accumulator.  It runs once per row r of the TRACE domain (x = w_n^r, no blowup, no
 * offset; d_cols are the n-row trace columns, SS_SRC_TRACE reads cols[col][(r + row_offset) mod n], a table is indexed by r mod its
 * length - a periodic column's table is its values over one period).  A domain is the pair of zerofier factor lists the AIRs use,
 * factor (p, e) = X^p - w_n^e: row r belongs to it iff some `den` factor vanishes at w_n^r and no `num` factor does, and a factor
 * vanishes iff p r = e (mod n).  On return first_row_out[k] = the smallest row of domain k at which numerator k is not zero
 * (UINT64_MAX: the constraint holds) and count_out[k] = the number of such rows; both are host arrays of n_checks entries.
 * Every check index below n_checks must appear exactly once. */
#define SS_CHECK_MAX_FACTORS 16u
typedef struct ss_check_domain {
    uint32_t n_num, n_den;                       /* <= SS_CHECK_MAX_FACTORS each */
    uint64_t num[SS_CHECK_MAX_FACTORS][2];       /* (p, e) */
    uint64_t den[SS_CHECK_MAX_FACTORS][2];
} ss_check_domain;
ss_status ss_check_constraints(ss_ctx *ctx, const ss_air_program *prog, const uint64_t *const *d_cols, uint32_t ncols, uint32_t log_n,
                               const ss_check_domain *domains, uint32_t n_checks, uint64_t *first_row_out, uint32_t *count_out);

/* ---- D1: out-of-domain evaluations + DEEP composition (ministark
 *      DeepPolyComposer, un-vendored; coefficient rule src/lib.rs:102-116).
 * ss_ood_eval: out[j] = T_{mask_col[j]}(z * w_n^{mask_off[j]}) from the
 * bit-reversed coefficient columns kept by ss_lde_fp252. */
ss_status ss_ood_eval(ss_ctx *ctx, const uint64_t *const *d_coeffs, uint32_t ncols, uint32_t log_n,
                      const uint32_t *mask_col, const uint32_t *mask_off, uint32_t nmask,
                      const uint64_t z[4], uint64_t *out /* nmask felts, host */);
/* ss_poly_eval: out[c] = P_c(x) for bit-reversed coefficient columns. */
ss_status ss_poly_eval(ss_ctx *ctx, const uint64_t *const *d_coeffs, uint32_t ncols, uint32_t log_n,
                       const uint64_t x[4], uint64_t *out /* ncols felts, host */);
/* Optional, ahead of ss_deep_compose (ABI 12): the composer's denominators 1 / (x - z w_n^o) and 1 / (x - z^ncomp) over
 * offset * <w_n> depend on the out-of-domain point alone.  Queued here - the call does not wait - they are built while
 * the host hashes the out-of-domain values into the coin (the Cairo coin: one Pedersen hash per value, crypto/src/
 * public_coin/cairo.rs reseed_with_field_elements); the next ss_deep_compose with the same (ncomp, log_n, offset, z)
 * uses them, any other makes its own. */
ss_status ss_deep_prepare(ss_ctx *ctx, uint32_t ncomp, uint32_t log_n, const uint64_t offset[4], const uint64_t z[4]);
/* d_out[i] = sum_j coeff_trace[j] (T_{col_j}(x_i) - ood_trace[j]) / (x_i - z w_n^{off_j})
 *          + sum_k coeff_comp[k]  (H_k(x_i)      - ood_comp[k])  / (x_i - z^ncomp)
 * for every x_i = offset * w_N^i of the LDE domain, natural order. */
ss_status ss_deep_compose(ss_ctx *ctx, const uint64_t *const *d_trace_lde, uint32_t ntrace_cols,
                          const uint64_t *const *d_comp_lde, uint32_t ncomp, uint32_t log_n,
                          uint32_t log_blowup, const uint64_t offset[4], const uint32_t *mask_col,
                          const uint32_t *mask_off, uint32_t nmask, const uint64_t *ood_trace,
                          const uint64_t *coeff_trace, const uint64_t *ood_comp,
                          const uint64_t *coeff_comp, const uint64_t z[4], uint64_t *d_out);
/* The two halves of ss_deep_compose, for one proof sharded over several GPUs.  The DEEP polynomial has degree < n, so
 * it is composed on the sub-coset offset * <w_n> (every blowup-th LDE row) and then interpolated and re-expanded:
 * ss_deep_compose_rows writes its values at the sub-coset points m0 <= m < m0 + count from column blocks with
 * d_*_blocks[c][k] = LDE row (m0 << log_blowup) + k (no rows behind the block are needed: DEEP reads one row per
 * point); ss_deep_extend takes all n sub-coset values (natural order, gathered from the ranks; overwritten) to the N
 * evaluations.  ss_deep_compose(...) == rows(m0 = 0, count = n) followed by extend, bit for bit. */
ss_status ss_deep_compose_rows(ss_ctx *ctx, const uint64_t *const *d_trace_blocks, uint32_t ntrace_cols,
                               const uint64_t *const *d_comp_blocks, uint32_t ncomp, uint32_t log_n,
                               uint32_t log_blowup, const uint64_t offset[4], const uint32_t *mask_col,
                               const uint32_t *mask_off, uint32_t nmask, const uint64_t *ood_trace,
                               const uint64_t *coeff_trace, const uint64_t *ood_comp,
                               const uint64_t *coeff_comp, const uint64_t z[4], uint64_t m0, uint64_t count,
                               uint64_t *d_out_subcoset);
ss_status ss_deep_extend(ss_ctx *ctx, uint64_t *d_subcoset, uint32_t log_n, uint32_t log_blowup,
                         const uint64_t offset[4], uint64_t *d_out);

/* ---- X4: the 64-bit field variant, p = 2^64 - 2^32 + 1 ("Goldilocks") with Fq3 = Fp[X]/(X^3 - 2): the pair the
 *      reference instantiates for its experimental claim (cli/src/main.rs:103-133:
 *      ministark_gpu::fields::p18446744069414584321::ark::{Fp, Fq3}; BASELINE.json configs[4]).  The same conventions as
 *      the 252-bit entry points (w = 7^((p-1)/n), evaluation at offset * w^k in natural order).  Elements are 8-byte
 *      values < p; every operation here is linear in the data, so Montgomery images (arkworks' in-memory Fp64) pass
 *      through unchanged.  `offset` / `alpha` are plain (canonical) values.  PARITY UNPINNED: the field crate is
 *      un-vendored and the reference holds no vector for it; the oracle restates the definitions (oracle/goldilocks.c). */
ss_status ss_ntt_gl64(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint32_t log_n, int direction, uint64_t offset,
                      int in_order, int out_order);
ss_status ss_lde_gl64(ss_ctx *ctx, const uint64_t *const *d_in, uint32_t ncols, uint32_t log_n, uint32_t log_blowup,
                      uint64_t offset, uint64_t *const *d_evals, uint64_t *const *d_coeffs /* nullable; bit-reversed */);
/* ss_subsample_rows over one-word cells: d_out[c][j] = d_in[c][j << log_stride], j < nrows_out.  With log_blowup above 1 the plain
 * AIR's constraints (degree 2) are still evaluated on the 2n-point coset offset*<w_2n> only: rows j << (log_blowup - 1) of the LDE,
 * which this call hands to ss_eval_quotient_gl64x3 as columns of log_blowup = 1.  A bit-exact copy of 64-bit words: nothing is
 * reduced, words >= p pass through.  d_in[c] holds at least ((nrows_out - 1) << log_stride) + 1 words, d_out[c] nrows_out, and nothing
 * beyond them is written; the two do not overlap.  nrows_out > 0; log_stride <= 4; any ncols (16 columns a launch).  On the ctx
 * stream, no host sync. */
ss_status ss_subsample_rows_gl64(ss_ctx *ctx, const uint64_t *const *d_in, uint32_t ncols, uint64_t nrows_out, uint32_t log_stride,
                                 uint64_t *const *d_out);
/* one FRI layer over Fq3-valued evaluations (interleaved [2^log_len][3]) on the Fp domain domain_offset * <w>, natural
 * order: row j = {evals[j + k len/fold]}, d_out[j] = (degree < fold interpolant of row j)(alpha), alpha in Fq3;
 * flags: SS_FRI_UNNORMALISED multiplies by fold */
ss_status ss_fri_fold_gl64x3(ss_ctx *ctx, const uint64_t *d_evals, uint32_t log_len, uint32_t fold, const uint64_t alpha[3],
                             uint64_t domain_offset, uint32_t flags, uint64_t *d_out);

/* D1 over the cubic extension (ministark's DeepPolyComposer with Fq = Fq3: the out-of-domain point and every coefficient
 * are elements of Fq3 - three values < p each - the trace columns are Fp arrays; an Fq3-valued column (extension trace,
 * composition) is passed as its three component columns, its cells carrying the coefficients c, c X, c X^2 and the
 * out-of-domain value on the first of them: the sum is linear).
 * ss_ood_eval_gl64x3: out[3 j ..) = P_{cell_col[j]}(z * w_n^{cell_off[j]}) for bit-reversed coefficient columns (as
 *   ss_lde_gl64 writes them); out is HOST memory.
 * ss_deep_compose_gl64x3: d_out[i] (interleaved [n * blowup][3], the layout ss_fri_fold_gl64x3 reads) =
 *   sum_j coeff_trace[j] (T_{col_j}(x_i) - ood_trace[j]) / (x_i - z w_n^{off_j})
 *   + sum_k coeff_comp[k] (H_k(x_i) - ood_comp[k]) / (x_i - z_comp),      x_i = offset * w_{n blowup}^i,
 *   composed on the n-point sub-coset and extended per component (the polynomial has degree < n). */
/* A2 over the cubic extension (plain layout: Trace::build_extension_columns, layouts/src/plain/trace.rs:274-330): the running
 * quotient of a permutation argument, out[k] = prod_{i<=k} (z - (alpha nv_i + na_i)) / prod_{i<=k} (z - (alpha dv_i + da_i)) in Fq3,
 * item i reading element i * stride of each input (value pointers NULL: single-column argument, terms z - a_i), written as three
 * coordinate columns at row out_offset + k * out_stride.  last_out (nullable, host): the final quotient - 1 for a permutation. */
ss_status ss_running_product_gl64x3(ss_ctx *ctx, const uint64_t *d_num_addr, const uint64_t *d_num_val, const uint64_t *d_den_addr,
                                    const uint64_t *d_den_val, uint64_t stride, uint64_t count, const uint64_t z[3], const uint64_t alpha[3],
                                    uint64_t *const d_out[3], uint64_t out_stride, uint64_t out_offset, uint64_t last_out[3]);
/* H1 / openings for matrices of 8-byte elements: digest i = Keccak-256 or Blake2s-256 (hash_kind) of row i's elements as little-endian bytes, segment by
 * segment (element e of segment s = d_segments[s][i * seg_len + e]): a trace matrix is nseg columns with seg_len 1, the rows of
 * an Fq3 FRI layer ([len][3] interleaved, row j = {evals[j + k rows]}) are nseg = fold segments d_evals + 3 k rows of seg_len 3.
 * The tree over the digests is ss_merkle_build's SS_TREE_KECCAK / SS_TREE_BLAKE2S / SS_TREE_SHA256.  (The reference instantiates this
 * field with ministark's Sha256HashFn trees, cli/src/main.rs:105,119 - SS_HASH_SHA256 / SS_TREE_SHA256 here, the hash pinned by the
 * FIPS 180-4 vectors; how ministark lays a row out as bytes is not in the reference: little-endian elements, as for the other two.)  ss_gather_rows_gl64: the opened rows, to HOST memory
 * [nidx][nseg][seg_len]. */
ss_status ss_hash_rows_gl64(ss_ctx *ctx, int hash_kind, const uint64_t *const *d_segments, uint32_t nseg, uint32_t seg_len,
                            uint64_t nrows, uint8_t *d_digests);
ss_status ss_gather_rows_gl64(ss_ctx *ctx, const uint64_t *const *d_segments, uint32_t nseg, uint32_t seg_len, uint64_t nrows,
                              const uint64_t *idx, uint32_t nidx, uint64_t *out);
/* Q1 over the cubic extension: the program format of ss_eval_quotient (ss_air_program above) with accumulators, scratch
 * slots and constants in Fq3 - prog->consts holds n_consts x 3 values < p - and trace cells, tables (prog->d_tables: 8-byte
 * elements) and x in Fp, read into the first coordinate, x_i = offset * w^i over the 2^(log_n + log_blowup)-point coset the columns
 * and the tables are laid out on.  d_out: [2^(log_n + log_blowup)][3] interleaved.  The plain layout's program runs as a compiled
 * kernel (csrc/quotient_gen_plain_gl.inc, recognised by its code), any other through the interpreter.  The provers call it with
 * log_blowup = 1 whatever the LDE's blowup is (ss_subsample_rows_gl64 hands it the coset's rows). */
ss_status ss_eval_quotient_gl64x3(ss_ctx *ctx, const ss_air_program *prog, const uint64_t *const *d_lde_cols, uint32_t ncols,
                                  uint32_t log_n, uint32_t log_blowup, uint64_t offset, uint64_t *d_out);
/* ss_check_constraints over the cubic extension: the check program's format, domains and results are ss_check_constraints' (one
 * SS_OP_CHECK k per constraint, no SS_OP_OUT; the trace domain x = w_n^r; first_row_out[k] = UINT64_MAX when constraint k holds), the
 * constants three words each as for ss_eval_quotient_gl64x3.  A numerator is an element of Fq3: it violates iff any of its three
 * coordinates is not zero.  ss_eval_quotient_gl64x3 goes on refusing SS_OP_CHECK. */
ss_status ss_check_constraints_gl64x3(ss_ctx *ctx, const ss_air_program *prog, const uint64_t *const *d_cols, uint32_t ncols,
                                      uint32_t log_n, const ss_check_domain *domains, uint32_t n_checks, uint64_t *first_row_out,
                                      uint32_t *count_out);
ss_status ss_ood_eval_gl64x3(ss_ctx *ctx, const uint64_t *const *d_coeffs_bitrev, uint32_t ncols, uint32_t log_n,
                             const uint32_t *cell_col, const uint32_t *cell_off, uint32_t ncells, const uint64_t z[3],
                             uint64_t *out);
ss_status ss_deep_compose_gl64x3(ss_ctx *ctx, const uint64_t *const *d_trace_lde, uint32_t ntrace_cols,
                                 const uint64_t *const *d_comp_lde, uint32_t ncomp, uint32_t log_n, uint32_t log_blowup,
                                 uint64_t offset, const uint32_t *mask_col, const uint32_t *mask_off, uint32_t nmask,
                                 const uint64_t *ood_trace, const uint64_t *coeff_trace, const uint64_t *ood_comp,
                                 const uint64_t *coeff_comp, const uint64_t z[3], const uint64_t z_comp[3], uint64_t *d_out);

/* ---- F1: one FRI layer fold (ministark FriProver::build_layers, un-vendored;
 *      defaults cli/src/main.rs:57-60).  d_evals: 2^log_len felts on
 *      domain_offset*<w>, natural order; row j = {evals[j + k*len/fold]};
 *      d_out[j] = degree<fold interpolant of row j evaluated at alpha.
 *      fold in {2,4,8,16}.  The next layer's offset is domain_offset^fold.
 *      The matrix whose rows get committed needs no entry point: its column k
 *      is the slice d_evals[k*len/fold ..) of the layer itself (no copy). */
ss_status ss_fri_fold(ss_ctx *ctx, const uint64_t *d_evals, uint32_t log_len, uint32_t fold,
                      const uint64_t alpha[4], const uint64_t domain_offset[4], uint64_t *d_out);
/* The same fold under the conventions found in the proof files the reference ships (data-only pin:
 * tests/golden/make_fri_golden.py, tests/golden/fri_saved_proofs.json).  flags = 0 is ss_fri_fold.
 *   SS_FRI_BITREV_ROWS    d_evals is in bit-reversed order: row r = evals[fold*r .. fold*r + fold), entry j of
 *                         the row at x_r * w_fold^bitrev(j) with x_r = domain_offset * w^bitrev(r); d_out is the
 *                         next layer, again in bit-reversed order (row r of this layer -> row r >> log2(fold),
 *                         slot r & (fold-1) of the next)
 *   SS_FRI_UNNORMALISED   d_out = fold * interpolant(alpha)  (StarkWare's fold: no 1/2 per halving)
 * example/array-sum.proof.saved and bootloader-proof.bin (masked-20 digests, the current code path) carry
 * BITREV_ROWS | UNNORMALISED; example/bootloader/bootloader-proof.bin (older path) carries flags = 0. */
enum { SS_FRI_BITREV_ROWS = 1, SS_FRI_UNNORMALISED = 2 };
ss_status ss_fri_fold_ex(ss_ctx *ctx, const uint64_t *d_evals, uint32_t log_len, uint32_t fold,
                         const uint64_t alpha[4], const uint64_t domain_offset[4], uint32_t flags,
                         uint64_t *d_out);

/* `count` rows of a layer from row `row0` on (one FRI layer folded by several GPUs): d_evals holds the
 * rows' `fold` entries column after column, entry k of row row0 + i at d_evals[k * count + i] (= the layer's
 * evals[row0 + i + k * len/fold]); d_out[i] = the fold of row row0 + i.  Natural order only (no SS_FRI_BITREV_ROWS). */
ss_status ss_fri_fold_rows(ss_ctx *ctx, const uint64_t *d_evals, uint32_t log_len, uint32_t fold,
                           const uint64_t alpha[4], const uint64_t domain_offset[4], uint32_t flags,
                           uint64_t row0, uint64_t count, uint64_t *d_out);

/* ---- C2: PublicCoin::grind_proof_of_work (crypto/src/public_coin/
 *      solidity.rs:120-141, cairo.rs:133-154).  Returns the SMALLEST nonce >= 1
 *      (the reference's non-parallel `find` semantics, solidity.rs:138). */
ss_status ss_pow_grind(ss_ctx *ctx, int coin_kind, const uint8_t digest[32], uint32_t bits,
                       uint64_t *nonce_out);

/* ---- builtins/src/pedersen/mod.rs:31-36 pedersen_hash, batched on device:
 *      d_out[i] = pedersen_hash(d_a[i], d_b[i]) (Montgomery felts in and out). */
ss_status ss_pedersen_hash(ss_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t n,
                           uint64_t *d_out);

/* ---- A2 / X1: Trace::build_extension_columns (layouts/src/recursive/trace.rs:699-814,
 *      layouts/src/starknet/trace.rs:997-1100), the sequential host loops between the base-trace and the
 *      extension-trace commitments ("TODO: multithread", trace.rs:700), as device scans.
 *
 * An operand describes `array_chunks::<STEP>()` of one column: item k is the STEP felts at d_data + k*stride.
 * Its term is   z - (alpha * item[value_offset] + item[addr_offset])    (memory: trace.rs:713-714)
 * or            z - item[addr_offset]            when value_offset < 0  (range check / diluted check: trace.rs:727-728). */
typedef struct {
    const uint64_t *d_data;    /* device column, Montgomery felts */
    uint64_t stride;           /* felts per item */
    uint64_t addr_offset;      /* felt index of a_k (or of the single value x_k) inside item k */
    int64_t value_offset;      /* felt index of v_k inside item k; negative: single-value term */
} ss_perm_operand;
/* d_out[out_offset + i*out_stride] = numerator_acc_i * batch_inversion(denominator_acc)_i for i < count, where
 * *_acc_i is the product of the first i+1 terms of the operand (trace.rs:712-719, 767-769).  Like ark-ff's
 * batch_inversion a zero denominator product inverts to zero.  last_out (nullable, host): the final value — the
 * reference asserts it is one for the range-check and diluted-check products (trace.rs:734, 757-760); that check
 * stays with the caller.  The other cells of d_out are not touched (the memory and range-check products share a
 * column). */
ss_status ss_permutation_product(ss_ctx *ctx, const ss_perm_operand *num, const ss_perm_operand *den, uint64_t count,
                                 const uint64_t z[4], const uint64_t alpha[4], uint64_t *d_out, uint64_t out_stride,
                                 uint64_t out_offset, uint64_t last_out[4]);
/* Diluted-check aggregate (trace.rs:787-803): with x_i = d_ordered[i*stride + offset],
 * d_out[out_offset] = 1 and d_out[out_offset + i*out_stride] = acc_i,
 * acc_i = acc_{i-1} * (1 + z*u_i) + alpha * u_i^2,  u_i = x_i - x_{i-1},  for 0 < i < count. */
ss_status ss_diluted_aggregate(ss_ctx *ctx, const uint64_t *d_ordered, uint64_t stride, uint64_t offset, uint64_t count,
                               const uint64_t z[4], const uint64_t alpha[4], uint64_t *d_out, uint64_t out_stride,
                               uint64_t out_offset);

/* ---- the same loops (trace.rs:699-814 "TODO: multithread") over the ROW BLOCKS of several devices (ABI 12): device r holds
 *      items [r count, (r + 1) count) of the operands.  A running product is the block's own ss_permutation_product (its
 *      last_out = the block's total) times the totals of the blocks before it: d_data[offset + i*stride] *= factor, i < count. */
ss_status ss_scale_strided(ss_ctx *ctx, uint64_t *d_data, uint64_t stride, uint64_t offset, uint64_t count,
                           const uint64_t factor[4]);
/* The aggregate's recurrence acc_i = acc_{i-1} * m_i + c_i (m_i = 1 + z*u_i, c_i = alpha*u_i^2) composes as affine maps:
 * d_maps[2i], d_maps[2i+1] = (M_i, C_i) with acc_i = M_i * start + C_i, where `start` is the value before the block.
 * starts_column != 0: item 0 is the column's first cell (acc_0 = 1, a constant map).  Otherwise item 0 is left the identity:
 * its term needs the ordered value before the block, which another device holds; the caller composes that one map from the two
 * boundary values.  total_out (nullable, host): (M, C) of the block's last item.  d_maps: 2*count felts, the caller's. */
ss_status ss_diluted_aggregate_block(ss_ctx *ctx, const uint64_t *d_ordered, uint64_t stride, uint64_t offset, uint64_t count,
                                     int starts_column, const uint64_t z[4], const uint64_t alpha[4], uint64_t *d_maps,
                                     uint64_t total_out[8]);
/* d_out[out_offset + i*out_stride] = d_maps[2i] * start + d_maps[2i+1] for i < count. */
ss_status ss_affine_apply(ss_ctx *ctx, const uint64_t *d_maps, uint64_t count, const uint64_t start[4], uint64_t *d_out,
                          uint64_t out_stride, uint64_t out_offset);

/* ---- the BASE trace on the device (ABI 11; SURVEY.md section 8a row A1 / "next" row X1).  ExecutionTrace::new
 *      (layouts/src/starknet/trace.rs:99-987, layouts/src/recursive/trace.rs:89-688, layouts/src/utils.rs:112-152,
 *      357-380) makes the 9 / 7 base columns from `cairo-run`'s trace.bin / memory.bin with rayon loops and sequential
 *      sorts on the host; uploaded, they are 3.6 - 4.8 GB of PCIe traffic for cells that are functions of ~25 MB.  These entry
 *      points make the cells in HBM from the raw files' bytes: the caller (host/device_trace.cpp, which knows the layouts)
 *      uploads the files, a placement table and one template per DISTINCT builtin instance, and calls them in the order the
 *      reference's sections run (a later section overwrites an earlier one's cells, as there).  Everything on the ctx stream,
 *      no host sync; errors of the INPUT (a cell memory.bin does not hold, memory that is not continuous, ...) are bits of a
 *      status block the caller reads once at the end (ss_trace_status).  Columns: n = 16 * num_cycles Montgomery felts. */
/* where the CPU's cells sit in a cycle's 16 rows (CYCLE_HEIGHT; the Npc / RangeCheck / Auxiliary enums of
 * layouts/src/{recursive,starknet}/air.rs): the memory pool's 8 (address, value) pairs, the range-check and the auxiliary column's 16 cells */
enum { SS_TRACE_NPC_PAD = 0,      /* (1, the value at address 1): the padding pair (trace.rs:204-207)      */
       SS_TRACE_NPC_PUBLIC = 1,   /* (0, 0): a public-memory slot (Npc::PubMemAddr)                       */
       SS_TRACE_NPC_PC = 2, SS_TRACE_NPC_OP0 = 3, SS_TRACE_NPC_DST = 4, SS_TRACE_NPC_OP1 = 5 };  /* (pc, instruction), (op0 address, op0), ... */
enum { SS_TRACE_RC_FILL = 0,      /* the column's filler (rc_max / the pool's largest value); the pool's own cells come with ss_trace_rc_pool */
       SS_TRACE_RC_ZERO = 1, SS_TRACE_RC_OFF_DST = 2, SS_TRACE_RC_OFF_OP0 = 3, SS_TRACE_RC_OFF_OP1 = 4 };
enum { SS_TRACE_AUX_ZERO = 0, SS_TRACE_AUX_AP = 1, SS_TRACE_AUX_FP = 2, SS_TRACE_AUX_TMP0 = 3, SS_TRACE_AUX_TMP1 = 4, SS_TRACE_AUX_OP0_MUL_OP1 = 5,
       SS_TRACE_AUX_RES = 6 };
typedef struct { uint8_t npc_pair[8], rc_cell[16], aux_cell[16]; } ss_trace_layout;
/* the status block: SS_TRACE_STATUS_WORDS u32 in device memory, zeroed (ss_dev_zero) before the first call of a generation.
 * word 0: SS_TRACE_ERR_* bits; word 1: ~(the smallest cycle or address an error names); the rest: the ordered memory's counters */
#define SS_TRACE_STATUS_WORDS 16u
enum { SS_TRACE_ERR_MISSING_CELL = 1,        /* the run reads a cell memory.bin does not hold                        */
       SS_TRACE_ERR_NOT_INSTRUCTION = 2,     /* pc points at a word that is not an instruction (binary/src/lib.rs:565-721) */
       SS_TRACE_ERR_BAD_OP1_SOURCE = 4, SS_TRACE_ERR_BAD_RES_LOGIC = 8,
       SS_TRACE_ERR_NOT_AN_ADDRESS = 16,     /* op0 is used as an address and does not fit one                       */
       SS_TRACE_ERR_ADDRESS_RANGE = 32,      /* an address beyond n / 2: continuous memory cannot reach it            */
       SS_TRACE_ERR_PUBLIC_ZERO = 64,        /* a public-memory entry at address 0                                   */
       SS_TRACE_ERR_PUBLIC_CELLS = 128,      /* the pool's address-0 pairs are not exactly the public-memory slots    */
       SS_TRACE_ERR_NO_ONES = 256,           /* memory does not start at address 1                                   */
       SS_TRACE_ERR_NOT_SINGLE_VALUED = 512, SS_TRACE_ERR_NOT_CONTINUOUS = 1024,      /* utils.rs:132-150            */
       SS_TRACE_ERR_TOO_MANY_GAPS = 2048,    /* more unaccessed addresses than cycles to hold them (trace.rs:594-625) */
       SS_TRACE_ERR_FILL = 4096,             /* the ordered accesses do not fill the column                          */
       SS_TRACE_ERR_PEDERSEN_INFINITY = 8192,  /* ss_trace_pedersen: a partial sum meets its constant point (see there) */
       SS_TRACE_ERR_PEDERSEN_INSTANCE = 16384, /* ss_trace_pedersen: an instance's index is beyond the blocks, or an input has a bit from 252 up: skipped */
       SS_TRACE_ERR_BITWISE_INSTANCE = 32768,  /* ss_trace_bitwise: the same, for a bitwise instance                    */
       SS_TRACE_ERR_POSEIDON_INSTANCE = 65536, /* ss_trace_poseidon: the same, for a Poseidon instance                  */
       SS_TRACE_ERR_EC_OP_INSTANCE = 131072, /* ss_trace_ec_op: the same, for an EC-op instance                        */
       SS_TRACE_ERR_EC_OP_DIVISOR = 262144,  /* ss_trace_ec_op: a doubling of Q whose y is zero (the tangent's slope divides by it) */
       SS_TRACE_ERR_EC_OP_MEETS = 524288,    /* ss_trace_ec_op: a partial sum shares its x with its step's point (see there) */
       SS_TRACE_ERR_ECDSA_INSTANCE = 1 << 20, /* ss_trace_ecdsa: an instance's index is beyond the blocks, or an input has a bit from 252 up: skipped */
       SS_TRACE_ERR_ECDSA_INVALID = 1 << 21,  /* ss_trace_ecdsa: neither root of the key verifies the signature, or a scalar is zero or has bit 251 set */
       SS_TRACE_ERR_ECDSA_DIVISOR = 1 << 22,  /* ss_trace_ecdsa: a doubling whose y is zero, or a chord between points that share their x   */
       SS_TRACE_ERR_ECDSA_MEETS = 1 << 23 };  /* ss_trace_ecdsa: a partial sum meets its step's point above the scalar's highest set bit (see there) */
/* memory.bin on the device: d_records = the file's bytes (n_records x (u64 address, 32-byte little-endian word), uploaded by
 * the caller) -> d_image[address] as 4 x u64; cells the file does not name are marked (all-ones: not a field element).
 * cells: entries of d_image; records beyond it are dropped (no address above n / 2 can be accessed by a valid run). */
ss_status ss_trace_memory_image(ss_ctx *ctx, const uint64_t *d_records, uint64_t n_records, uint64_t *d_image, uint64_t cells);
/* The CPU's cells (starknet trace.rs:177-244, 294-302; recursive 172-232): one lane per cycle decodes the instruction at pc,
 * reads dst / op0 / op1 from d_image, computes res (dst^-1 for a conditional jump), tmp0, tmp1, op0 * op1, and the workgroup
 * writes the cycle's 16 rows of the flags, memory-pool, range-check and auxiliary columns whole (every cell: what no later
 * call overwrites keeps the padding written here) and the pool's 8 addresses per cycle as integers (d_pool_addr, n / 2 u32).
 * d_states: trace.bin's bytes ((ap, fp, pc) u64 triples).  pad_value: the value at address 1, Montgomery.  rc_fill: the
 * range-check column's filler. */
ss_status ss_trace_cpu_cells(ss_ctx *ctx, const ss_trace_layout *layout, const uint64_t *d_states, uint64_t num_cycles, const uint64_t *d_image,
                             uint64_t cells, const uint64_t pad_value[4], uint64_t rc_fill, uint64_t *d_flags, uint64_t *d_pool, uint64_t *d_range_check,
                             uint64_t *d_auxiliary, uint32_t *d_pool_addr, uint32_t *d_status);
/* A builtin's instances (Pedersen trace.rs:304-386, ECDSA 428-523, bitwise 525-705, EC op 707-777, Poseidon 779-888): block i
 * of `block_rows` rows holds one instance; cell e of the instance's template goes to column d_cells[e].col, row
 * i * block_rows + d_cells[e].off, and is the template's value e (SS_TRACE_CELL_VALUE: d_values[template * n_cells + e],
 * Montgomery) or the felt of the address addr_begin + addr_per_block * i + d_cells[e].arg (SS_TRACE_CELL_ADDRESS: an even row of
 * the memory pool; d_pool_addr gets the integer).  d_template_of_block: the template of every block (NULL: template 0
 * everywhere - a run whose instances are all the dummy one); n_templates: templates in d_values. */
typedef struct { uint32_t col, off, kind, arg; } ss_trace_cell;
enum { SS_TRACE_CELL_VALUE = 0, SS_TRACE_CELL_ADDRESS = 1 };
ss_status ss_trace_builtin(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, const ss_trace_cell *d_cells, uint32_t n_cells, const uint64_t *d_values,
                           uint32_t n_templates, const uint32_t *d_template_of_block, uint64_t n_blocks, uint64_t block_rows, uint64_t addr_begin,
                           uint64_t addr_per_block, uint32_t *d_pool_addr);
/* A GIVEN Pedersen instance's cells from its two inputs, computed on the device (builtins/src/pedersen/mod.rs:81-163; starknet
 * trace.rs:304-386, recursive 300-400) - no template, 72 bytes per instance.  d_instances: n_given records of 9 u64 = index, a[4],
 * b[4] (canonical little-endian limbs, both below 2^252); instance `index` owns rows [index * block_rows, (index + 1) * block_rows)
 * of the columns (col_rows felts each; n_blocks * block_rows <= col_rows).  For each of the 512 steps j - the bits of a, then of b -
 * row off_* + row_stride * j of the block gets the partial sum before the step (col_x, col_y), the suffix input >> (j mod 256)
 * (col_suffix) and the slope of the step's addition (col_slope; zero where the bit is clear); then, per input, the cells
 * bit251 && bit196 (col_flag2, off_flag2) and bit251 && bit196 && bit192 (col_flag3, off_flag3) - the second input's 256 *
 * row_stride rows further down - and the three memory-pool pairs (addr_begin + 3 * index + k, value) for a, b and the hash at rows
 * off_input0 / off_input1 / off_output (even) of col_pool, their integer addresses in d_pool_addr[row / 2] (col_rows / 2 u32).
 * All values Montgomery felts, bit-identical to the host generator's.  Call it AFTER ss_trace_builtin has written the dummy
 * instance's template over all blocks: it overwrites the given ones.  The indices must be distinct.
 * Refused with an error (nothing launched): NULL pointers (also with n_given = 0), blocks that do not fit the columns, a column
 * >= ncols, a cell that leaves its block.  Found on the device, as bits of d_status: an index >= n_blocks or an input with a bit
 * from 252 up - the instance is skipped, nothing is written for it (SS_TRACE_ERR_PEDERSEN_INSTANCE); a partial sum that meets its
 * constant point, where the chord's slope does not exist (SS_TRACE_ERR_PEDERSEN_INFINITY: no input is known to reach it; the
 * instance's cells are then unfinished - its step-511 suffix cell holds all ones, no field element - and the caller must refuse
 * the generation - host/device_trace.hpp does, with the host generator's "point at infinity in a Pedersen partial sum"; the tangent
 * case, which the host generator could still trace, is refused too). */
typedef struct {
    uint32_t col_x, off_x, col_y, off_y, col_suffix, off_suffix, col_slope, off_slope;   /* step j: row off + row_stride * j */
    uint32_t row_stride;                                                                  /* 1 starknet, 4 recursive */
    uint32_t col_flag2, off_flag2, col_flag3, off_flag3;                                  /* + 256 * row_stride for the second input */
    uint32_t col_pool, off_input0, off_input1, off_output;                                /* the three (address, value) pairs */
} ss_trace_pedersen_layout;
ss_status ss_trace_pedersen(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const ss_trace_pedersen_layout *layout,
                            const uint64_t *d_instances, uint64_t n_given, uint64_t n_blocks, uint64_t block_rows, uint64_t addr_begin, uint32_t *d_pool_addr,
                            uint32_t *d_status);
/* A GIVEN bitwise instance's cells from x and y, computed on the device (builtins/src/bitwise/mod.rs:23-133; starknet
 * trace.rs:525-667, recursive 420-588) - no template, 72 bytes per instance.  d_instances: n_given records of 9 u64 = index, x[4],
 * y[4] (canonical little-endian limbs, both below 2^252); instance `index` owns rows [index * block_rows, (index + 1) * block_rows)
 * of the columns (col_rows felts each; n_blocks * block_rows <= col_rows).  With SS_TRACE_BITWISE_CELLS in `what`: for value p of
 * x, y, x & y, x ^ y, 64-bit word c and sg < 4 the diluted part (word >> sg) & 0x1111...1 at row off_part + stride_p * p + stride_c * c
 * + stride_s * sg of col_diluted (starknet 1 + 256 p + 64 c + 16 sg, recursive 32 p + 8 c + 2 sg), and the four top segments of
 * x & y + x ^ y shifted left by 4, 4, 4, 8 at rows off_shifted[k].  With SS_TRACE_BITWISE_PAIRS: the five memory-pool pairs
 * (addr_begin + 5 * index + k, value) of x, y, x & y, x ^ y, x | y at rows off_pair[k] (even) of col_pool, their integer addresses in
 * d_pool_addr[row / 2] (col_rows / 2 u32).  (The recursive layout writes the cells before the CPU's section and the pairs after it -
 * ss_trace_cpu_cells writes the pool's rows whole -, the starknet layout both at once.)  All values Montgomery felts, bit-identical
 * to the host generator's.  Call it AFTER ss_trace_builtin has written the dummy instance's template over all blocks: it overwrites
 * the given ones.  The indices must be distinct.  Bit 251 of x | y does not fit the last shifted cell: the host generator refuses such
 * an instance ("top segment does not fit") and so must the caller - host/device_trace.hpp does, before the upload.
 * Refused with an error (nothing launched): NULL pointers (also with n_given = 0), `what` without either bit, blocks that do not fit
 * the columns, a column >= ncols, a cell that leaves its block, an odd pool offset.  Found on the device, as a bit of d_status: an index
 * >= n_blocks or an input with a bit from 252 up - the instance is skipped, nothing is written for it (SS_TRACE_ERR_BITWISE_INSTANCE). */
typedef struct {
    uint32_t col_diluted, off_part, stride_p, stride_c, stride_s;                         /* the 4 x 4 x 4 diluted parts */
    uint32_t off_shifted[4];                                                              /* the shifted top segments (col_diluted) */
    uint32_t col_pool, off_pair[5];                                                       /* x, y, x & y, x ^ y, x | y */
} ss_trace_bitwise_layout;
enum { SS_TRACE_BITWISE_CELLS = 1, SS_TRACE_BITWISE_PAIRS = 2 };
ss_status ss_trace_bitwise(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const ss_trace_bitwise_layout *layout,
                           const uint64_t *d_instances, uint64_t n_given, uint64_t n_blocks, uint64_t block_rows, uint64_t addr_begin, uint32_t what,
                           uint32_t *d_pool_addr, uint32_t *d_status);
/* A GIVEN Poseidon instance's cells from its three inputs, computed on the device (builtins/src/poseidon/mod.rs:45-152; starknet
 * trace.rs:779-888) - no template, 104 bytes per instance.  d_instances: n_given records of 13 u64 = index, in0[4], in1[4], in2[4]
 * (canonical little-endian limbs below 2^252).  d_round_keys: the 91 rounds' keys (4 full, 83 partial, 4 full rounds), 3 Montgomery
 * felts each, in the order the rounds take them (the caller's: the library derives no constants of its own).  Per full round r < 8 the
 * state after the key addition at rows full_stride * r + off_full[j] and its squares at + off_full_sq[j] of col_full; per partial
 * round k the third element after the key addition and its square at partial_stride * k + off_partial / off_partial_sq of
 * col_partial for k < n_partial and at tail_stride * (k - tail_first) + off_tail / off_tail_sq of col_tail for k >= tail_first
 * (starknet: rounds 0 .. 63 in the range-check column at 8 k + 3 / 7, rounds 61 .. 82 in the auxiliary column at 16 (k - 61) + 6 / 14);
 * the six memory-pool pairs (addr_begin + 6 * index + k, value) of the three inputs and the three outputs at rows off_pair[k] (even)
 * of col_pool, their integer addresses in d_pool_addr[row / 2].  All values Montgomery felts, bit-identical to the host generator's.
 * Call it AFTER ss_trace_builtin has written the dummy instance's template over all blocks; the indices must be distinct.
 * Refused with an error (nothing launched): NULL pointers (also with n_given = 0), blocks that do not fit the columns, a column
 * >= ncols, a cell that leaves its block, n_partial or tail_first above 83, an odd pool offset.  Found on the device: an index
 * >= n_blocks or an input with a bit from 252 up - skipped, nothing written (SS_TRACE_ERR_POSEIDON_INSTANCE). */
typedef struct {
    uint32_t col_full, full_stride, off_full[3], off_full_sq[3];
    uint32_t col_partial, partial_stride, off_partial, off_partial_sq, n_partial;
    uint32_t col_tail, tail_stride, off_tail, off_tail_sq, tail_first;
    uint32_t col_pool, off_pair[6];
} ss_trace_poseidon_layout;
ss_status ss_trace_poseidon(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const ss_trace_poseidon_layout *layout,
                            const uint64_t *d_round_keys, const uint64_t *d_instances, uint64_t n_given, uint64_t n_blocks, uint64_t block_rows,
                            uint64_t addr_begin, uint32_t *d_pool_addr, uint32_t *d_status);
/* A GIVEN EC-op instance's cells from P, Q and m, computed on the device (builtins/src/ec_op/mod.rs:40-130; starknet trace.rs:707-777)
 * - no template, 168 bytes per instance.  d_instances: n_given records of 21 u64 = index, P.x[4], P.y[4], Q.x[4], Q.y[4], m[4]
 * (canonical little-endian limbs below 2^252); instance `index` owns rows [index * block_rows, (index + 1) * block_rows) of the
 * columns (col_rows felts each; n_blocks * block_rows <= col_rows).  For each of the 256 steps j, row off_* + row_stride * j of the
 * block in column `col` gets the doubling point 2^j Q (off_dbl_x, off_dbl_y) with its tangent's slope (3 x^2 + 1) / (2 y)
 * (off_dbl_slope), the partial sum before the step - P plus the 2^i Q of the set bits i < j of m - (off_sum_x, off_sum_y), the suffix
 * m >> j (off_suffix) and, for j != 255 only, the chord's slope (off_slope; zero where bit j is clear) and 1 / (partial.x - point.x)
 * (off_x_diff_inv): those two cells of step 255 are the ECDSA section's and are neither written nor read.  Then the cells
 * bit251 && bit196 (off_flag2) and bit251 && bit196 && bit192 (off_flag3) of m, and the seven memory-pool pairs
 * (addr_begin + 7 * index + k, value) of P.x, P.y, Q.x, Q.y, m, R.x, R.y - R the partial sum at step 255 - at rows off_pair[k] (even) of
 * col_pool, their integer addresses in d_pool_addr[row / 2] (col_rows / 2 u32).  All values Montgomery felts, bit-identical to the
 * host generator's.  No cell of the columns ever holds an intermediate value: the chains' scratch is LDS, and the doubling points are
 * read back from their own cells once they are final.
 * Call it AFTER ss_trace_builtin has laid the ECDSA templates and the EC-op dummy instance's template over all blocks: it
 * overwrites the given ones.  The indices must be distinct.
 * Refused with an error (nothing launched): NULL pointers (also with n_given = 0), blocks that do not fit the columns, a column
 * >= ncols, a cell that leaves its block, an odd pool offset.  Found on the device, as bits of d_status: an index >= n_blocks or an
 * input with a bit from 252 up - skipped, nothing written (SS_TRACE_ERR_EC_OP_INSTANCE); a doubling of Q whose y is zero
 * (SS_TRACE_ERR_EC_OP_DIVISOR: the host generator's "a curve step divides by zero"); a partial sum that shares its x with its step's
 * point, at any of the 256 steps, bit set or clear (SS_TRACE_ERR_EC_OP_MEETS: "a partial sum meets the fixed point").  After either of
 * the last two the instance's cells are unfinished and the caller must refuse the generation - host/device_trace.hpp does, the divisor
 * first, as the host generator reaches it first. */
typedef struct {
    uint32_t col, row_stride;                                                             /* step j: row off + row_stride * j (64 starknet) */
    uint32_t off_dbl_x, off_dbl_y, off_dbl_slope, off_sum_x, off_sum_y, off_suffix, off_slope, off_x_diff_inv;
    uint32_t off_flag2, off_flag3;                                                        /* (col) */
    uint32_t col_pool, off_pair[7];                                                       /* P.x, P.y, Q.x, Q.y, m, R.x, R.y */
} ss_trace_ec_op_layout;
ss_status ss_trace_ec_op(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const ss_trace_ec_op_layout *layout,
                         const uint64_t *d_instances, uint64_t n_given, uint64_t n_blocks, uint64_t block_rows, uint64_t addr_begin, uint32_t *d_pool_addr,
                         uint32_t *d_status);
/* A GIVEN ECDSA instance's cells from the public key, the message and the signature, computed on the device
 * (builtins/src/ecdsa/mod.rs:85-147 InstanceTrace::new, 157-206 the chains, 275-304 verify and mimic_ec_mad_air; starknet trace.rs:428-523)
 * - no template, 168 bytes per instance.  d_instances: n_given records of 21 u64 = index, key.x[4], key.y[4], message[4], r[4], w[4]
 * (canonical little-endian limbs below 2^252); key.y is EITHER square root of x^3 + x + beta (the caller's: the device takes no roots) and
 * the kernel orders the two candidates y, p - y itself, the canonically larger first, as `verify` does.  instance `index` owns rows
 * [index * block_rows, (index + 1) * block_rows) of the columns (col_rows felts each; n_blocks * block_rows <= col_rows).  d_points: 252
 * affine points as Montgomery felts (x, y) - entries 0 .. 250 the 2^i G, entry 251 the shift point P0 (the caller's: the library derives
 * no constants of its own).  All cells are in column `col`:
 *   the generator's chain z G from -P0 (point i = d_points[min(i, 250)]): for each of the 256 steps j, row off_gen_* + gen_stride * j gets
 *     the partial sum before the step (off_gen_x, off_gen_y), the chord's slope (off_gen_slope; zero where bit j is clear),
 *     1 / (partial.x - point.x) (off_gen_x_diff_inv) and message >> j (off_gen_suffix);
 *   half 0, the key's: for each step j, row off_* + row_stride * j gets the doubling point 2^j Q (off_dbl_x, off_dbl_y) with its tangent's
 *     slope (off_dbl_slope) and, of the chain r Q from P0, the partial sum (off_sum_x, off_sum_y), the slope (off_slope), the x-difference's
 *     inverse (off_x_diff_inv) and r >> j (off_suffix);
 *   half 1, B = z G + r Q: the same cells 256 * row_stride rows further down, for B's doublings and the chain w B from P0;
 *   then - last, as four of them are step-255 cells of the chains in the starknet layout - the slope of the chord through w B and -P0
 *     (off_r_point_slope) and 1 / (w B.x - P0.x) (off_r_point_x_diff_inv), 1 / r, 1 / w, 1 / message in the field (off_r_inv, off_w_inv,
 *     off_message_inv), key.x^2 (off_pubkey_x_squared), the slope of the chord through z G and r Q (off_b_slope) and 1 / (z G.x - r Q.x)
 *     (off_b_x_diff_inv);
 * and the two memory-pool pairs (addr_begin + 2 * index + k, value) of key.x and the message at rows off_pair[k] (even) of col_pool, their
 * integer addresses in d_pool_addr[row / 2] (col_rows / 2 u32).  All values Montgomery felts, bit-identical to the host generator's.  No
 * cell of the columns ever holds an intermediate value of another kind: the chains' scratch is LDS, the doubling points are read back from
 * their own cells.  The candidate Q = (x, root) is accepted when x(w B - P0) = r; a candidate that fails, or whose partial sum meets its
 * step's point at a step up to the scalar's highest set bit (where mimic_ec_mad_air gives up), is rejected and the other root runs the same
 * way over the same cells: a full second pass that writes every cell of the first again.
 * Call it AFTER ss_trace_builtin has laid the dummy signature's template over all blocks and BEFORE ss_trace_ec_op (the EC-op section
 * leaves its step-255 slope cells to this one).  The indices must be distinct.
 * Refused with an error (nothing launched): NULL pointers (also with n_given = 0), blocks that do not fit the columns, a column >= ncols,
 * a cell that leaves its block (2 * 256 steps at row_stride, 256 at gen_stride), an odd pool offset, n_given > n_blocks.  Found on the
 * device, as bits of d_status: an index >= n_blocks or an input with a bit from 252 up - skipped, nothing written
 * (SS_TRACE_ERR_ECDSA_INSTANCE); message, r or w zero or with bit 251 set - no chain is run -, or both roots rejected
 * (SS_TRACE_ERR_ECDSA_INVALID: the host generator's "signature is invalid"; a key.y that is no root of the curve's equation ends here or at
 * the next); a doubling whose y is zero - key.y = 0 is one -, or a zero z G.x - r Q.x or w B.x - P0.x (SS_TRACE_ERR_ECDSA_DIVISOR: "a curve
 * step divides by zero"); a partial sum that meets its step's point ABOVE the scalar's highest set bit, which mimic_ec_mad_air does not
 * see and gen_ec_mad_steps divides by (SS_TRACE_ERR_ECDSA_MEETS: "a partial sum meets the fixed point").  The last two end the instance at
 * the candidate that finds them (the reference would still try the other root); with a key on the curve neither is reachable - the start
 * points are fixed and the group's order is prime.  After any of the last three the instance's cells are unfinished and the caller must
 * refuse the generation - host/device_trace.hpp does. */
typedef struct {
    uint32_t col, row_stride, gen_stride;                                                 /* 64 and 128 in the starknet layout */
    uint32_t off_dbl_x, off_dbl_y, off_dbl_slope, off_sum_x, off_sum_y, off_slope, off_x_diff_inv, off_suffix;   /* a half's step j: row off + row_stride * (256 * half + j) */
    uint32_t off_gen_x, off_gen_y, off_gen_slope, off_gen_x_diff_inv, off_gen_suffix;     /* step j: row off + gen_stride * j */
    uint32_t off_r_point_slope, off_r_point_x_diff_inv, off_r_inv, off_w_inv, off_message_inv, off_pubkey_x_squared, off_b_slope, off_b_x_diff_inv;
    uint32_t col_pool, off_pair[2];                                                       /* key.x, message */
} ss_trace_ecdsa_layout;
ss_status ss_trace_ecdsa(ss_ctx *ctx, uint64_t *const *d_cols, uint32_t ncols, uint64_t col_rows, const ss_trace_ecdsa_layout *layout,
                         const uint64_t *d_points, const uint64_t *d_instances, uint64_t n_given, uint64_t n_blocks, uint64_t block_rows,
                         uint64_t addr_begin, uint32_t *d_pool_addr, uint32_t *d_status);
/* The 16-bit range-check pool (utils.rs:357-380; starknet trace.rs:142-165, 246-292, 388-426).  The caller counts the pool's
 * values (65536 bins: the instructions' offsets, the builtin's parts) and hands over
 *   d_first[j], j <= rc_hi - rc_lo + 1: ordered values before value rc_lo + j (every value of [rc_lo, rc_hi] max(count, 1) times),
 *   d_padding[n_padding]: the values of [rc_lo, rc_hi] nothing uses, ascending (then rc_hi forever).
 * ss_trace_rc_pool writes, per cycle, its 16 / ordered_step ordered values at rows ordered_step * j + ordered_off and, on odd
 * cycles, padding value pad0 + cycle / 2 at row unused_off; ss_trace_rc_builtin slot s < n_slots of slot_rows rows: instance s of
 * d_given (3 u64 each: index, value low, value high) or, from n_given on, a dummy instance whose 8 parts are padding values
 * 8 (s - n_given) ...; the parts at rows part_stride * k + part_off of the range-check column, (addr_begin + index, value) at
 * rows pair_off, pair_off + 1 of the memory pool. */
typedef struct {
    uint64_t n_slots, n_given, slot_rows, addr_begin, n_padding, pad0;
    uint32_t part_stride, part_off, pair_off, rc_lo, rc_hi, ordered_step, ordered_off, unused_off;
} ss_trace_rc_plan;
ss_status ss_trace_rc_pool(ss_ctx *ctx, const ss_trace_rc_plan *plan, const uint32_t *d_first, const uint16_t *d_padding, uint64_t num_cycles,
                           uint64_t *d_range_check);
ss_status ss_trace_rc_builtin(ss_ctx *ctx, const ss_trace_rc_plan *plan, const uint64_t *d_given, const uint16_t *d_padding, uint64_t *d_range_check,
                              uint64_t *d_pool, uint32_t *d_pool_addr);
/* An ordered pool's column (the diluted check: starknet trace.rs:695-705, recursive 560-588): slot k < slots goes to
 * d_col[k * stride + offset]: zero for k < d_first[0], else the value lo + j with d_first[j] <= k < d_first[j + 1]
 * (j < n_values; d_first has n_values + 1 entries), diluted (bit i -> bit 4 i) if asked. */
ss_status ss_trace_ordered_runs(ss_ctx *ctx, uint64_t *d_col, uint64_t stride, uint64_t offset, uint64_t slots, const uint32_t *d_first,
                                uint32_t n_values, uint32_t lo, int diluted);
/* d_col[d_rows[k]] = felt(d_values[k]) for k < count (rows >= col_rows are skipped): the cells that are neither per cycle
 * nor per instance (the diluted pool's padding values: trace.rs:668-693) */
ss_status ss_trace_patch(ss_ctx *ctx, uint64_t *d_col, uint64_t col_rows, const uint64_t *d_rows, const uint64_t *d_values, uint64_t count);
/* get_ordered_memory_accesses (utils.rs:112-152) and the gap fillers before it (trace.rs:594-625 / 890-925), without a sort:
 * the pool's n / 2 accesses (d_pool_addr; values in d_pool) and the public memory's entries (d_public_addr / d_public_value
 * [n_public], the latter Montgomery; its remaining public_cells - n_public entries are (1, pad_value)) are counted per address,
 * the unaccessed addresses between the lowest and the highest become (address, 0) pairs at row unused_off of cycles 0, 1, ...
 * of d_pool, and d_memory receives (a, value(a)) x count(a) for a = 1, 2, ...; the reference's checks set SS_TRACE_ERR_* bits. */
ss_status ss_trace_ordered_memory(ss_ctx *ctx, uint64_t n, uint64_t *d_pool, uint64_t *d_memory, uint32_t *d_pool_addr, const uint32_t *d_public_addr,
                                  const uint64_t *d_public_value, uint32_t n_public, uint64_t public_cells, const uint64_t pad_value[4],
                                  uint32_t unused_off, uint32_t *d_status);
/* ---- the base trace of the PLAIN layout over the 64-bit field p = 2^64 - 2^32 + 1 (the claim of cli/src/main.rs:103-133; ExecutionTrace::new,
 *      layouts/src/plain/trace.rs:60-262, which cli/src/main.rs:186-202 runs inside its "Proof generated in" timer).  The pipeline above over
 *      one-word cells: five columns of n = 16 * num_cycles plain u64 values below p - NOT Montgomery: what every *_gl64* entry point takes -
 *      with that layout's placement, the only one the field has (layouts/src/plain/air.rs:560-760):
 *        flags        the 16 flag prefixes
 *        pool (Npc)   (pc, instruction) at rows 0, 1; (op0) 4, 5; (dst) 8, 9; (op1) 12, 13; the public-memory slots (0, 0) at 2, 3 and 10, 11; the
 *                     padding pair (1, value at address 1) at 6, 7 and 14, 15 - the latter the gap cell (Npc::GapAddr / GapVal)
 *        range check  off_dst / off_op1 / off_op0 at 0 / 4 / 8; ap, op0 * op1, fp, res at 3 / 7 / 11 / 15; the ordered values at 4 j + 2 and the
 *                     unused value at 12 (ss_trace_gl64_rc_pool); the filler rc_fill at 1, 5, 9, 13
 *        auxiliary    tmp0 at 0, tmp1 at 8, zero elsewhere
 *      Same stream, same status block and SS_TRACE_ERR_* bits as above, with one difference: the CPU's five error bits (MISSING_CELL ..
 *      NOT_AN_ADDRESS, bits b = 0 .. 4) each name their smallest cycle in a word of their own, status[SS_TRACE_STATUS_GL_CYCLE + b] = ~cycle, and
 *      word 1 names addresses only (the ordered memory's errors): a location is never reported for another error's bit.  Every writer takes
 *      the columns' length col_rows and refuses a size that would write past it. */
#define SS_TRACE_STATUS_GL_CYCLE 7u
/* memory.bin (plain/trace.rs:60-75 reads it through binary/src/lib.rs Memory): d_image[address] = the record's word as ONE u64.  All ones
 * (>= p: no field element) marks a cell no record names and a cell whose word has a nonzero upper 24 bytes or a low word >= p: the run
 * that reads it is refused as a missing cell.  Records at or beyond `cells` are dropped. */
ss_status ss_trace_gl64_memory_image(ss_ctx *ctx, const uint64_t *d_records, uint64_t n_records, uint64_t *d_image, uint64_t cells);
/* The CPU's cells (plain/trace.rs:100-215): one lane per cycle decodes the word at pc, reads dst / op0 / op1 from d_image, computes res
 * (dst^-1 for a conditional jump, zero for dst = 0), tmp0, tmp1 and op0 * op1; the workgroup writes the cycle's 16 rows of the four
 * columns whole, and the pool's 8 addresses per cycle into d_pool_addr (n / 2 u32).  pad_value: the value at address 1.  An op0 used as
 * an address that has more than 32 bits sets SS_TRACE_ERR_NOT_AN_ADDRESS. */
ss_status ss_trace_gl64_cpu_cells(ss_ctx *ctx, const uint64_t *d_states, uint64_t num_cycles, const uint64_t *d_image, uint64_t cells, uint64_t pad_value,
                                  uint64_t rc_fill, uint64_t col_rows, uint64_t *d_flags, uint64_t *d_pool, uint64_t *d_range_check, uint64_t *d_auxiliary,
                                  uint32_t *d_pool_addr, uint32_t *d_status);
/* The range-check pool (plain/trace.rs:216-240; utils.rs:357-380) from the plan ss_trace_rc_pool takes (ordered_step 4, ordered_off 2,
 * unused_off 12; d_first, d_padding as there): the ordered values at rows 4 j + 2 and padding value pad0 + c at row 12 of EVERY cycle c -
 * the 252-bit layouts place one on odd cycles -, then rc_hi forever. */
ss_status ss_trace_gl64_rc_pool(ss_ctx *ctx, const ss_trace_rc_plan *plan, const uint32_t *d_first, const uint16_t *d_padding, uint64_t num_cycles, uint64_t col_rows,
                                uint64_t *d_range_check);
/* The gap cells and the ordered memory column (plain/trace.rs:92-98, 241-262; utils.rs:112-152), as ss_trace_ordered_memory: counts per
 * address from d_pool_addr and the public memory (d_public_value: values below p; the other n / 8 - n_public entries are (1, pad_value)),
 * the unaccessed addresses between the lowest and the highest as (address, 0) at rows 14, 15 of cycles 0, 1, ..., the sorted (address,
 * value) pairs into d_memory's even / odd rows; the reference's checks set the same SS_TRACE_ERR_* bits. */
ss_status ss_trace_gl64_ordered_memory(ss_ctx *ctx, uint64_t n, uint64_t col_rows, uint64_t *d_pool, uint64_t *d_memory, uint32_t *d_pool_addr,
                                       const uint32_t *d_public_addr, const uint64_t *d_public_value, uint32_t n_public, uint64_t pad_value, uint32_t *d_status);
/* waits for the stream and reads the status block (SS_TRACE_STATUS_WORDS u32) */
ss_status ss_trace_status(ss_ctx *ctx, const uint32_t *d_status, uint32_t *status_out);

/* ---- per-kernel timing (bench.py's roofline leg): when enabled, every launch of
 *      the named kernel family on the ctx stream is bracketed by HIP events.
 *      ss_profile_read synchronises the stream and returns the accumulated device
 *      time and launch count since the last reset. */
enum { SS_PROF_NTT_PASS = 0, SS_PROF_HASH_ROWS = 1, SS_PROF_MERKLE = 2, SS_PROF_FRI = 3, SS_PROF_QUOTIENT = 4,
       SS_PROF_DEEP = 5, SS_PROF_EXT = 6, SS_PROF_TRACE = 7, SS_PROF_KINDS = 8 };
ss_status ss_profile_enable(ss_ctx *ctx, int on);
ss_status ss_profile_reset(ss_ctx *ctx);
ss_status ss_profile_read(ss_ctx *ctx, int kind, double *total_ms, uint64_t *launches);
/* ss_profile_enable(ctx, 2): besides the events, every profiled scope stamps the chip's constant-rate reference counter
 * (s_memrealtime, 100 MHz) before and after its launches, and ONE monitor wave on a stream of its own samples its shader-cycle
 * counter (s_memtime: one per compute unit, so only a single wave's readings are comparable) against that reference every ~20 us
 * for as long as level 2 is on (at most 3 s per read interval).  ss_profile_read_clock: the shader cycles - the monitor's count
 * interpolated at the scopes' reference stamps - and the reference ticks accumulated over this kernel family's scopes since the
 * last reset: cycles / ticks x 100 MHz is the clock the chip granted those kernels, in the run it is read in.  The stamps cost a
 * few microseconds per scope: level 2 is for a measuring pass, not a timed one.  (Up to 8192 scopes between two reads.) */
ss_status ss_profile_read_clock(ss_ctx *ctx, int kind, double *shader_cycles, double *ref_ticks);

/* Host-side pedersen_hash for the Fiat-Shamir coin (CairoVerifierPublicCoin::
 * reseed_with_field_elements hashes the OOD evaluations with a sequential
 * Pedersen chain, crypto/src/public_coin/cairo.rs:76-80; the coin stays on the
 * host).  Montgomery felts in and out; no device involved. */
ss_status ss_pedersen_hash_host(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]);

/* Host-side Keccak-256 for the SolidityVerifierPublicCoin (crypto/src/public_coin/
 * solidity.rs:36-53 hashes 32..64-byte messages hundreds of times per proof: one
 * reseed per out-of-domain evaluation).  No device involved. */
ss_status ss_keccak256_host(const uint8_t *msg, size_t len, uint8_t out[32]);

/* ---- micro-benchmark hook: d_out[i] = d_a[i] * d_b[i] repeated `reps` times
 *      (dependent chain), used by bench.py to report mulmod/s. */
ss_status ss_fp252_mul_bench(ss_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, uint64_t n,
                             uint32_t reps, uint64_t *d_out);

#ifdef __cplusplus
}
#endif
#endif
