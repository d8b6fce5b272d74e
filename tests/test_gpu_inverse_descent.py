"""The inverse tables D[i] = 1 / (offset w_N^i - z) (deep.hip launch_batch_inverse) against pow(x - z, p - 2, p): the chunked kernel
below 2^DESCENT_MIN_LOG entries, the descent by squaring from there on, the fallback to the (zero-aware) chunked kernel when the
last level of the descent meets a zero, and the range form of the row blocks against slices of the whole table.

The library descends from 2^22 entries on (a last level of 2^19 or 2^20 entries: deep.hip BATCH_INVERSE_DESCENT_LAST_LOG);
SS_BATCH_INV_DESCENT_LAST_LOG=11 brings that down to 2^14 (from 2^11 / 2^12) for every test here but the last, which runs one
table at the library's own threshold.

The plain table is ss_inverse_table's output.  The R280 form (entries times 2^24) and the range form are what the DEEP composer reads:
composing ONE constant column T = 1 with one mask cell (coefficient 1, out-of-domain value 0) gives out[i] = D[i] * (1 * T[i] - 0) on
the sub-coset, which the composer hands back as every second row of its extension (ss_deep_compose) or as they are
(ss_deep_compose_rows)."""
import numpy as np
import pytest

from tests.util import P

pytestmark = pytest.mark.gpu

LAST_LOG = 11                   # SS_BATCH_INV_DESCENT_LAST_LOG for these tests
DESCENT_MIN_LOG = LAST_LOG + 3  # deep.hip launch_batch_inverse: 2^14 entries and more descend (from 2^12; 2^15 from 2^11; 2^16 in two launches)
DEFAULT_MIN_LOG = 22            # the same with the library's own BATCH_INVERSE_DESCENT_LAST_LOG = 19
SIZES = list(range(3, DESCENT_MIN_LOG + 3))                    # 3 .. 16: both kernels, both parities of the descent's last level
RNG_Z = pow(0x2545F4914F6CDD1D, 3, P)
# z with top-of-field limbs (tests/edge_values.py: stored values in [2^251, p) and the ends of the field)
TOP_Z = [P - 2, 2**251 + 2**192 + 12345, 2**251 - 1]


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


@pytest.fixture(autouse=True)
def small_last_level(monkeypatch):
    monkeypatch.setenv("SS_BATCH_INV_DESCENT_LAST_LOG", str(LAST_LOG))


def _domain(log_N, offset):
    w = pow(3, (P - 1) >> log_N, P)
    xs, x = [], offset % P
    for _ in range(1 << log_N):
        xs.append(x)
        x = x * w % P
    return xs


_WANT = {}


def _want(log_N, offset, z):
    """the reference, once per case: 0 where x == z (what the batched inversion leaves there)"""
    key = (log_N, offset, z)
    if key not in _WANT:
        _WANT[key] = [pow(x - z, P - 2, P) for x in _domain(log_N, offset)]
    return _WANT[key]


def _plain(ctx, oracle, log_N, offset, z):
    out = ctx.alloc(32 << log_N)
    ctx.inverse_table(log_N, oracle.to_mont([offset])[0], oracle.to_mont([z])[0], out)
    raw = out.download(np.uint64, (1 << log_N, 4))
    return raw, list(oracle.from_mont(raw))


def _through_deep(ctx, oracle, log_N, offset, z, blocks=None):
    """the R280 table as the composer multiplies by it: whole (None), or the row blocks [(m0, count)] of the range form"""
    n = 1 << log_N
    one = oracle.to_mont([1])[0]
    zero = np.zeros((1, 4), dtype=np.uint64)
    none = np.zeros((0, 4), dtype=np.uint64)
    g, zm = oracle.to_mont([offset])[0], oracle.to_mont([z])[0]
    if blocks is None:
        col = ctx.column(np.tile(one, (2 * n, 1)))
        out = ctx.alloc(64 * n)
        ctx.deep_compose([col], [], log_N, 1, g, [0], [0], zero, one[None, :], none, none, zm, out)
        return list(oracle.from_mont(out.download(np.uint64, (2 * n, 4))[::2]))
    got = []
    for m0, count in blocks:
        col = ctx.column(np.tile(one, (2 * count, 1)))
        out = ctx.alloc(32 * count)
        ctx.deep_compose_rows([col], [], log_N, 1, g, [0], [0], zero, one[None, :], none, none, zm, m0, count, out)
        got.append(list(oracle.from_mont(out.download(np.uint64, (count, 4)))))
    return got


@pytest.mark.parametrize("log_N", SIZES)
@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("zkind", ["random", "top"])
def test_plain_table(ctx, oracle, log_N, offset, zkind):
    z = RNG_Z if zkind == "random" else TOP_Z[log_N % len(TOP_Z)]
    raw, got = _plain(ctx, oracle, log_N, offset, z)
    assert got == _want(log_N, offset, z)
    from tests.edge_values import below_p
    assert below_p(raw).all()                                   # fully reduced images


@pytest.mark.parametrize("log_N", SIZES)
@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("zkind", ["random", "top"])
def test_r280_table(ctx, oracle, log_N, offset, zkind):
    z = RNG_Z if zkind == "random" else TOP_Z[(log_N + 1) % len(TOP_Z)]
    assert _through_deep(ctx, oracle, log_N, offset, z) == _want(log_N, offset, z)


# Which z send the descent back to the chunked kernel: those with z^(2^J) = x^(2^J) for a domain point x, i.e. z = x * (a 2^J-th root
# of unity).  With 2^J <= N those roots are powers of w_N, so such a z is a domain point itself: the last level has a zero exactly
# when the table has one.  In particular -x = x w_N^(N/2) is a domain point, and a z with z^2 equal to a domain point's square that
# is neither a point nor the negative of one cannot exist (z^2 = x^2 <=> z = +-x) - nothing to test there.
@pytest.mark.parametrize("log_N", [5, DESCENT_MIN_LOG - 1, DESCENT_MIN_LOG, DESCENT_MIN_LOG + 1, 16])
@pytest.mark.parametrize("r280", [False, True])
def test_z_on_the_domain(ctx, oracle, log_N, r280):
    """z a domain point: that entry is 0 (pow(0, p - 2) == 0), every other entry is right - the last level's zero sends the launch
    back to the chunked kernel, which zeroes that entry alone"""
    xs = _domain(log_N, 3)
    i = (5 << (log_N - 3)) + 1
    z = xs[i]
    got = _through_deep(ctx, oracle, log_N, 3, z) if r280 else _plain(ctx, oracle, log_N, 3, z)[1]
    want = _want(log_N, 3, z)
    assert want[i] == 0 and sum(1 for v in want if v == 0) == 1
    assert got == want


@pytest.mark.parametrize("log_N", [5, DESCENT_MIN_LOG - 1, DESCENT_MIN_LOG, DESCENT_MIN_LOG + 1, 16])
@pytest.mark.parametrize("r280", [False, True])
def test_z_minus_a_domain_point(ctx, oracle, log_N, r280):
    """z = -(x_i): the first squaring already meets x_i^2, so the descent falls back here too.  The domain is closed under negation
    (-x_i = x_{i + N/2}), so the one zero of the table sits at i + N/2; entry i and every other one are non-zero and right."""
    N = 1 << log_N
    xs = _domain(log_N, 3)
    i = 7 % (N // 2)
    z = (P - xs[i]) % P
    got = _through_deep(ctx, oracle, log_N, 3, z) if r280 else _plain(ctx, oracle, log_N, 3, z)[1]
    want = _want(log_N, 3, z)
    assert [k for k, v in enumerate(want) if v == 0] == [i + N // 2]
    assert got == want


@pytest.mark.parametrize("log_N", [DESCENT_MIN_LOG, DESCENT_MIN_LOG + 1])
def test_z_between_two_domain_points(ctx, oracle, log_N):
    """z = x_7 w_2N: as close to the domain as a point outside it gets (its square lies between two points of the squared domain);
    no level has a zero, every entry is non-zero and right"""
    xs = _domain(log_N, 3)
    z = xs[7] * pow(3, (P - 1) >> (log_N + 1), P) % P
    want = _want(log_N, 3, z)
    assert all(v != 0 for v in want)
    assert _plain(ctx, oracle, log_N, 3, z)[1] == want


def test_range_form_is_a_slice_of_the_table(ctx, oracle):
    log_N, z = 12, TOP_Z[0]
    blocks = [(0, 1024), (1024, 2048), (3072 + 512, 512)]
    want = _want(log_N, 3, z)
    got = _through_deep(ctx, oracle, log_N, 3, z, blocks)
    for (m0, count), g in zip(blocks, got):
        assert g == want[m0:m0 + count], (m0, count)


def test_table_at_the_library_threshold(ctx, oracle, monkeypatch):
    """2^22 entries with no override: the descent as a proof runs it (two launches from a last level of 2^20).  Every entry equals the
    chunked kernel's (the same call with the descent moved out of reach), 4096 of them - the first, the last, both sides of every
    quarter, a stride through the rest - equal pow()."""
    log_N, offset, z = DEFAULT_MIN_LOG, 3, TOP_Z[1]
    N = 1 << log_N
    monkeypatch.delenv("SS_BATCH_INV_DESCENT_LAST_LOG")
    descended, _ = None, None
    out = ctx.alloc(32 * N)
    om, zm = oracle.to_mont([offset])[0], oracle.to_mont([z])[0]
    ctx.inverse_table(log_N, om, zm, out)
    descended = out.download(np.uint64, (N, 4))
    monkeypatch.setenv("SS_BATCH_INV_DESCENT_LAST_LOG", "40")
    ctx.inverse_table(log_N, om, zm, out)
    assert np.array_equal(descended, out.download(np.uint64, (N, 4)))
    idx = sorted(set([0, 1, N - 1, N - 2] + [k * (N // 4) + d for k in range(1, 4) for d in (-1, 0, 1)] + list(range(5, N, N // 4080))))
    w = pow(3, (P - 1) >> log_N, P)
    want = [pow(offset * pow(w, i, P) - z, P - 2, P) for i in idx]
    assert list(oracle.from_mont(descended[idx])) == want
