"""The commitment path's Keccak kernels (hash.hip) against the oracle's hashes and trees: row digests at the widths that have an
instantiation (1, 2, 4, 7, 8, 9, 10) and at widths the generic kernel serves, felt-pair leaves read in place for the bit-reversed
order, and trees below, at and above the size from which one workgroup finishes a tree.  Bit-exact."""
import numpy as np
import pytest

from tests.util import random_column

pytestmark = pytest.mark.gpu

# kernels.h KECCAK_TREE_TOP_LOG: a level of <= 2^13 nodes is the last one built by a launch of its own; one workgroup builds the
# levels above it.  Trees of 2 and 4 leaves are that launch alone, 2^13 leaves start in it, 2^14 and 2^15 take one and two
# level launches first.
TREE_TOP_LOG = 13

WIDTHS = [1, 2, 3, 4, 5, 8, 9, 10, 16]          # 4 -> 5 felts crosses the 136-byte rate; 9 and 10 are three-block messages
ROWS = [1, 64, 256, 1024, 4096]                 # 4096 rows are more than one workgroup's; 1 and 64 leave lanes idle
MAX_ROWS = max(ROWS)


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def be():
    from sandstorm_amd import backend
    return backend


_COLS = {}


def _col(c):
    """column c of the shared matrix, MAX_ROWS rows, with the field's edge values mixed into its first rows (tests/edge_values.py)"""
    if c not in _COLS:
        from tests.edge_values import EDGE_LIMBS
        col = random_column(MAX_ROWS, 300 + c).copy()
        k = len(EDGE_LIMBS)
        col[1:1 + k] = np.roll(EDGE_LIMBS, c, axis=0)
        col.setflags(write=False)
        _COLS[c] = col
    return _COLS[c]


_REF = {}


def _row_digests(oracle, kind, width, n):
    key = (kind, width, n)
    if key not in _REF:
        _REF[key] = oracle.hash_rows(kind, [_col(c)[:n] for c in range(width)])
    return _REF[key]


def _bitrev(n):
    bits = n.bit_length() - 1
    return [int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(n)]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("width", WIDTHS)
def test_row_digests(ctx, be, oracle, width, n):
    m = be.Matrix.from_host(ctx, [_col(c)[:n] for c in range(width)])
    perm = _bitrev(n)
    for kind in (be.HASH_KECCAK, be.HASH_KECCAK_M20):
        want = _row_digests(oracle, kind, width, n)
        assert np.array_equal(m.hash_rows(kind).download(np.uint8, (n, 32)), want), (kind, "natural")
        assert np.array_equal(m.hash_rows(kind, be.BITREV).download(np.uint8, (n, 32)), want[perm]), (kind, "bit-reversed")


@pytest.mark.parametrize("pairs", [1, 2, 64, 1 << 12])
@pytest.mark.parametrize("tree", [0, 1, 3])
def test_felt_pair_leaves(ctx, be, oracle, tree, pairs):
    """both orders against the oracle, and the ordered mode against a bit-reversed copy (ss_bitrev_permute32) hashed in natural order:
    the leaf slots and the first level of digests (the Blake2s twin of the kernel takes the same mode)"""
    n = 2 * pairs
    log_n = n.bit_length() - 1
    col = np.concatenate([_col(3), _col(4)])[:n]
    perm = _bitrev(n)
    d_col = ctx.column(col)
    nat, ordered, copied = ctx.alloc(64 * n), ctx.alloc(64 * n), ctx.alloc(64 * n)
    ctx.merkle_build(tree, 0, 1, d_col, n, nat)
    ctx.merkle_build(tree, 0, 1, d_col, n, ordered, None, be.BITREV)
    d_perm = ctx.alloc(32 * n)
    ctx.bitrev_permute32(d_col, log_n, d_perm)
    ctx.merkle_build(tree, 0, 1, d_perm, n, copied)
    got_nat, got_ord, got_cp = (b.download(np.uint8, (2 * n, 32)) for b in (nat, ordered, copied))
    assert np.array_equal(got_ord[1:], got_cp[1:])
    assert pairs == 1 or not np.array_equal(got_ord[pairs:], got_nat[pairs:])
    if tree == 3:
        return                                                          # (the oracle's Blake2s trees take digests as leaves)
    want_nat, _ = oracle.merkle_build(tree, 0, 1, col)
    want_rev, _ = oracle.merkle_build(tree, 0, 1, col[perm])
    assert np.array_equal(got_nat[pairs:], want_nat[pairs:])            # leaf slots and the pairs' digests
    assert np.array_equal(got_ord[pairs:], want_rev[pairs:])
    assert np.array_equal(got_ord[1:], want_rev[1:])


_LEAVES = {}


def _leaves(oracle, leaf_kind, n):
    key = (leaf_kind, n)
    if key not in _LEAVES:
        col = random_column(n, 411)
        _LEAVES[key] = col if leaf_kind == 1 else oracle.hash_rows(0, [col, random_column(n, 412)])
    return _LEAVES[key]


@pytest.mark.parametrize("log_n", [1, 2, TREE_TOP_LOG, TREE_TOP_LOG + 1, TREE_TOP_LOG + 2])
@pytest.mark.parametrize("leaf_kind", [0, 1])
@pytest.mark.parametrize("tree", [0, 1])
def test_trees(ctx, be, oracle, tree, leaf_kind, log_n):
    n = 1 << log_n
    leaves = _leaves(oracle, leaf_kind, n)
    want_nodes, _ = oracle.merkle_build(tree, 0, leaf_kind, leaves)
    nodes = ctx.alloc(64 * n)
    root, _ = ctx.merkle_build(tree, 0, leaf_kind, ctx.alloc(32 * n).upload(leaves), n, nodes)
    got = nodes.download(np.uint8, (2 * n, 32))
    for d in range(log_n + 1):                                           # every stored level, the leaf slots included
        assert np.array_equal(got[1 << d:2 << d], want_nodes[1 << d:2 << d]), "level %d" % d
    assert root == bytes(want_nodes[1])
    # openings at the first, the last and a middle leaf verify: the path's siblings hash up to the root
    idx = sorted(set([0, n // 2, n - 1]))
    paths, _ = ctx.merkle_open(nodes, None, n, idx)
    for q, i in enumerate(idx):
        k, cur = n + i, got[n + i]
        for lvl in range(log_n):
            sib = paths[q, lvl]
            pair = np.stack([cur, sib] if k % 2 == 0 else [sib, cur])
            if lvl == 0 and leaf_kind == 1:
                pair = leaves[[(i & ~1), (i | 1)]]                      # the leaf level hashes the elements themselves
            two, _ = oracle.merkle_build(tree, 0, leaf_kind if lvl == 0 else 0, pair)
            cur, k = two[1], k >> 1
            if lvl == 0 and leaf_kind == 1:
                assert bytes(sib) == bytes(got[(n + i) ^ 1])
        assert bytes(cur) == root
