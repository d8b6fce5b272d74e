"""Pure-Python big-integer restatements used to cross-check the C oracle on
small cases (test infrastructure).  Definitions follow SURVEY.md §8(a)."""
import hashlib

P = 2**251 + 17 * 2**192 + 1
BETA = 3141592653589793238462643383279502884197169399375105820974944592307816406665


def root_of_unity(n):
    return pow(3, (P - 1) // n, P)


def ec_double(pt):
    x, y = pt
    lam = (3 * x * x + 1) * pow(2 * y, -1, P) % P
    x3 = (lam * lam - 2 * x) % P
    return x3, (lam * (x - x3) - y) % P


def ec_add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2) = p1, p2
    if x1 == x2:
        return ec_double(p1) if y1 == y2 else None
    lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def make_pedersen(points):
    """points: the five StarkWare constants P0..P4 (tests/golden/pedersen.json)."""
    p0, p1, p2, p3, p4 = points

    def pedersen(a, b):
        acc = p0
        for val, lo, hi in ((a, p1, p2), (b, p3, p4)):
            for bits, base in ((val & (2**248 - 1), lo), (val >> 248, hi)):
                pt = base
                while bits:
                    if bits & 1:
                        acc = ec_add(acc, pt)
                    pt = ec_double(pt)
                    bits >>= 1
        return acc[0]
    return pedersen


def blake2s(b):
    return hashlib.blake2s(b).digest()


def mask_blake(d):
    return bytes(12) + d[12:]


def mask_keccak(d):
    return d[:20] + bytes(12)


def interpolate_eval(xs, ys, t):
    """value at t of the Lagrange interpolant through (xs, ys)."""
    acc = 0
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        num, den = 1, 1
        for j, xj in enumerate(xs):
            if i != j:
                num = num * (t - xj) % P
                den = den * (xi - xj) % P
        acc = (acc + yi * num * pow(den, -1, P)) % P
    return acc


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _fft(a, w):
    """values of the polynomial with coefficients a at w^0 .. w^(n-1), w of order n = len(a) (radix 2, recursive)"""
    n = len(a)
    if n == 1:
        return list(a)
    even, odd = _fft(a[0::2], w * w % P), _fft(a[1::2], w * w % P)
    out, t = [0] * n, 1
    for k in range(n // 2):
        u = odd[k] * t % P
        out[k], out[k + n // 2] = (even[k] + u) % P, (even[k] - u) % P
        t = t * w % P
    return out


def ntt(coeffs, offset=1):
    """natural order: value k is sum_j coeffs[j] (offset w_n^k)^j"""
    n = len(coeffs)
    return _fft([c * pow(offset, j, P) % P for j, c in enumerate(coeffs)], root_of_unity(n))


def intt(values, offset=1):
    """the inverse of ntt(., offset): the coefficients, natural order"""
    n = len(values)
    a = _fft(list(values), pow(root_of_unity(n), -1, P))
    inv_n, inv_off = pow(n, -1, P), pow(offset, -1, P)
    return [v * inv_n * pow(inv_off, j, P) % P for j, v in enumerate(a)]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def fri_fold(evals, fold, alpha, offset, bitrev_rows=False, unnormalised=False):
    """fri.hip's header formula: row j holds f at x_j w_fold^k, k < fold, and folds to
    (1/fold) sum_m (alpha / x_j)^m sum_k f(x_j w_fold^k) w_fold^(-k m)  (no 1/fold when unnormalised).
    Natural order: f(x_j w_fold^k) = evals[j + k rows], x_j = offset w^j.  Bit-reversed rows: row r = evals[fold r .. fold r + fold),
    entry i at x_r w_fold^bitrev(i), x_r = offset w^bitrev(r); the output is in bit-reversed order too."""
    n = len(evals)
    rows, log_fold = n // fold, fold.bit_length() - 1
    w, wf_inv = root_of_unity(n), pow(root_of_unity(fold), -1, P)
    scale = 1 if unnormalised else pow(fold, -1, P)
    out = []
    for j in range(rows):
        if bitrev_rows:
            x = offset * pow(w, _bitrev(j, (rows.bit_length() - 1)), P) % P
            v = [evals[fold * j + _bitrev(k, log_fold)] for k in range(fold)]
        else:
            x = offset * pow(w, j, P) % P
            v = [evals[j + k * rows] for k in range(fold)]
        t = alpha * pow(x, -1, P) % P
        acc = 0
        for m in range(fold):
            s = sum(v[k] * pow(wf_inv, k * m, P) for k in range(fold)) % P
            acc = (acc + s * scale * pow(t, m, P)) % P
        out.append(acc)
    return out
