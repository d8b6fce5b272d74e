"""fl_scale<C> (csrc/fl252.h): the small integer multiples of a lazy 9 x 28-bit value that the generated constraint kernels take
instead of a product by a structural constant - run on the host (tests/cpp/fl_scale_test.cpp) for every (C, input bound) pair
tools/gen_quotient.py can emit and held to Python's integers: the limb vector of C x is EXACTLY C times the input's (so is the value,
and no limb wrapped), its negative is exactly C' p - C x over non-negative limbs, both within the bounds fl252.h documents (value in
units of p, limbs in units of 2^28), and their canonical images are C x and -C x modulo p.  The inputs: 0, 1, p - 1, seeded random
values, and limb vectors at the top of every input bound.  The program is built twice: plain, and with the address and undefined-
behaviour sanitizers, and run stand-alone both times."""
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "fl_scale_test.cpp")
P = 2**251 + 17 * 2**192 + 1
MAX_BOUND = 8                       # tools/gen_quotient.py: a lazy value of bound b is < 2 b p with limbs as limb_tops(b) allows
# What the generator's values of bound 1 look like at most: a normalised value (limbs <= 2^28 - 1), or what one borrow-free
# subtraction fl_sub_c<2, 1> adds to a bound - its constant 2p written limb-wise is (2^28 + 2, 2^28 - 1 x 5, 2^28 - 1 + 2^25, 2^28 + 1,
# 2^28 - 1): 2^28 - 1 per limb and a little of p's own shape on limbs 0, 6 and 7.  Bounds add and scale limb-wise, so a value of bound
# b has limbs <= b x these - and fl_sub_c<8, 2> / <16, 4>, which negate a scaled value of bound 2 / 4, leave exactly that room.
UNIT = [(1 << 28) + 2, (1 << 28) - 1, (1 << 28) - 1, (1 << 28) - 1, (1 << 28) - 1, (1 << 28) - 1, (1 << 28) - 1 + (1 << 25), (1 << 28) + 1, (1 << 28) - 1]


def limb_tops(b):
    """limbs 0 .. 7 by the unit; the top limb by the value bound 2 b p (it absorbs the carries: fl_sub_c states its own condition on it)"""
    return [b * u for u in UNIT[:8]] + [(2 * b * P) >> 224]


def limbs_of(v):
    """a value < 2^256 as normalised limbs: eight of 28 bits and the top one"""
    return [(v >> (28 * i)) & ((1 << 28) - 1) for i in range(8)] + [v >> 224]


def value_of(limbs):
    return sum(l << (28 * i) for i, l in enumerate(limbs))


def within(limbs, b):
    """the limb vector with its top limb lowered until the value is below 2 b p (limbs 0 .. 7 stay where they are: at most 2^224 each
    way, the top limb's unit)"""
    low = value_of(limbs[:8])
    return limbs[:8] + [min(limbs[8], (2 * b * P - 1 - low) >> 224)]


def inputs():
    rng = random.Random(20251)
    out = []
    for b in range(1, MAX_BOUND // 2 + 1):                      # C >= 2: input bounds 1 .. 4
        tops = limb_tops(b)
        for v in (0, 1, P - 1, P, P + 1, (1 << 251), (1 << 252) - 1):
            out.append((limbs_of(v), b))                         # normalised values of bound 1 are values of every bound
        out.append((within(list(tops), b), b))                   # every limb at the top of the bound, the top one as far as 2 b p allows
        for i in range(9):                                       # one limb at the top, the others random
            l = [rng.randrange(t + 1) for t in tops]
            l[i] = tops[i]
            out.append((within(l, b), b))
        for _ in range(40):
            out.append((limbs_of(rng.randrange(1 << 252)), b))   # normalised, < 2^252 (what a weak reduction leaves)
            out.append((within([rng.randrange(t + 1) for t in tops], b), b))
    return out


def build(tmp, flags, name):
    exe = os.path.join(tmp, name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + flags + ["-o", exe, CPP])
    return exe


NEGATION = {1: (2, 1, 2), 2: (8, 2, 4), 3: (16, 4, 8), 4: (16, 4, 8)}        # scaled bound -> fl_sub_c<C', F>, the result's bound


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_fl_scale_against_integers(tmp_path, flags):
    tmp = str(tmp_path)
    exe = build(tmp, flags, "fl_scale_test")
    cases = inputs()
    path_in, path_out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for limbs, b in cases:
            f.write(struct.pack("<10I", *(limbs + [b])))
    subprocess.check_call([exe, path_in, path_out])
    with open(path_out, "rb") as f:
        words = struct.unpack("<%dI" % (os.path.getsize(path_out) // 4), f.read())
    at, seen = 0, set()
    for limbs, b in cases:
        x = value_of(limbs)
        assert x < 2 * b * P and all(l <= t for l, t in zip(limbs, limb_tops(b)))           # the test's own inputs are within the bound they claim
        for c in range(2, 9):
            if c * b > MAX_BOUND:
                continue
            rec = words[at:at + 35]
            at += 35
            assert rec[0] == c
            s, n, s_fp, n_fp = list(rec[1:10]), list(rec[10:19]), rec[19:27], rec[27:35]
            seen.add((c, b))
            # C x: limb for limb, hence exactly - value < C (2 b p), limbs within C times the input's
            assert s == [c * l for l in limbs], (c, b, limbs)
            assert value_of(s) == c * x and value_of(s) < 2 * c * b * P and all(l <= t for l, t in zip(s, limb_tops(c * b)))
            assert sum(w << (32 * i) for i, w in enumerate(s_fp)) == c * x % P
            # -(C x) = C' p - C x (after a weak reduction where C b > 4: then 2 p - (C x - q p))
            sb = c * b
            if sb <= 4:
                cc, _, nb = NEGATION[sb]
                assert value_of(n) == cc * P - c * x, (c, b, limbs)
            else:
                nb = 2
                assert 0 <= value_of(n) <= 2 * P and (value_of(n) + c * x) % P == 0
            assert value_of(n) <= 2 * nb * P and all(l <= t for l, t in zip(n, limb_tops(nb))), (c, b, limbs)          # (C' p itself for x = 0)
            assert sum(w << (32 * i) for i, w in enumerate(n_fp)) == -c * x % P
    assert at == len(words)
    assert seen == {(c, b) for c in range(2, 9) for b in range(1, 5) if c * b <= MAX_BOUND}
