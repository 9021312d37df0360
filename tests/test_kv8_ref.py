"""tests/kv8_ref.py, the numpy definition of the fp8 K/V panel format (cross_kv_fp8): the properties the rest of the
test plan rests on.  CPU only."""
import numpy as np
import torch

from tests import kv8_ref as kv8


def bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).bfloat16().float().numpy()


def random_rows(n, seed, lo=-20, hi=20):
    """bf16-valued rows whose magnitudes span the binades [lo, hi)."""
    g = np.random.default_rng(seed)
    scale = np.ldexp(1.0, g.integers(lo, hi, size=(n, 1)))
    x = g.standard_normal((n, 64)) * scale * np.ldexp(1.0, g.integers(-6, 1, size=(n, 64)))
    return bf16(x)


def test_scaled_amax_lies_in_224_448():
    x = random_rows(4000, 0)
    codes, b = kv8.quantize_rows(x)
    e = b.astype(np.int64) - 127
    amax = np.abs(x.astype(np.float64)).max(axis=1)
    s = np.ldexp(amax, -e)
    nz = amax > 0
    assert nz.all()
    assert np.all(s[nz] > 224.0) and np.all(s[nz] <= 448.0)
    # so the row's largest code is in the top binade of e4m3: no precision is given away
    assert np.all((codes & 0x7F).max(axis=1) >= 0x76)             # >= 224


def test_exponent_rule_at_the_boundary():
    # m = 1.75 exactly (bf16 mantissa 0x60) scales to 448; the next bf16 (mantissa 0x61) takes the next exponent
    for k in (-30, -1, 0, 5, 40):
        at = np.float32(np.ldexp(1.75, k))
        above = kv8.from_bf16_bits(kv8.bf16_bits(np.array([at])) + np.uint16(1))[0]
        x = np.zeros((2, 64), np.float32)
        x[0, 3], x[1, 3] = at, -above
        codes, b = kv8.quantize_rows(x)
        assert int(b[0]) - 127 == k - 8 and codes[0, 3] == 0x7E             # 448
        assert int(b[1]) - 127 == k - 7 and codes[1, 3] == 0xF6             # 1.7578 * 128 = 225 -> -224


def test_dequantised_values_are_bf16():
    x = random_rows(4000, 1, -100, 100)
    codes, b = kv8.quantize_rows(x)
    d = kv8.dequantize_rows(codes, b)
    assert np.isfinite(d).all()
    assert np.array_equal(bf16(d).view(np.uint32), d.view(np.uint32))
    # and the float32 cast inside dequantize_rows did not round either
    e = b.astype(np.int64) - 127
    assert np.array_equal(d.astype(np.float64), np.ldexp(kv8.e4m3_value(codes), e[:, None]))
    # every code of the clamp range dequantises to a normal bf16 number (or zero)
    allc = np.tile(np.arange(256, dtype=np.uint8), (2, 1))[:, :64 * 4].reshape(8, 64)
    for ee in (kv8.E_MIN, kv8.E_MAX):
        dd = kv8.dequantize_rows(allc, np.full(8, ee + 127, np.uint8))
        fin = np.isfinite(dd)
        assert np.array_equal(bf16(dd[fin]).view(np.uint32), dd[fin].view(np.uint32))
        nzv = np.abs(dd[fin & (dd != 0)])
        assert nzv.min() >= np.ldexp(1.0, -126)


def test_requantising_is_a_fixed_point():
    """Quantising a dequantised row returns the same codes and byte, with one exception that follows from the exponent
    rule itself: a row whose scaled amax lies in (224, 232] rounds to 224 = 1.75 * 2^7, the dequantised row's amax then
    has m = 1.75 exactly and takes the exponent one lower (its 224 becomes 448).  Such a row (largest code 0x76) keeps
    its VALUES (every code's value doubles exactly), which is what the kernels' bit identity needs."""
    x = random_rows(4000, 2, -60, 60)
    x[7] = 0
    x[8, ::2] = -0.0
    codes, b = kv8.quantize_rows(x)
    d = kv8.dequantize_rows(codes, b)
    c2, b2 = kv8.quantize_rows(d)
    top = (codes & 0x7F).max(axis=1)
    same = top != 0x76
    assert same.sum() > 3000 and (~same).sum() > 10
    assert np.array_equal(b2[same], b[same])
    assert np.array_equal(c2[same], codes[same])
    assert np.array_equal(b2[~same].astype(int), b[~same].astype(int) - 1)
    assert ((c2[~same] & 0x7F).max(axis=1) == 0x7E).all()
    d2 = kv8.dequantize_rows(c2, b2)
    assert np.array_equal(d2.view(np.uint32), d.view(np.uint32))


def test_error_bound_of_a_row():
    # a value's error is at most half an e4m3 step of the row's top binade: 2^(e + 8 - 4) = amax_scaled-binade / 16
    x = random_rows(2000, 3)
    codes, b = kv8.quantize_rows(x)
    e = b.astype(np.int64) - 127
    err = np.abs(kv8.dequantize_rows(codes, b).astype(np.float64) - x)
    assert np.all(err <= np.ldexp(16.0, e)[:, None])


def test_zero_row_and_negative_zero():
    x = np.zeros((2, 64), np.float32)
    x[0, 5] = -0.0
    x[1] = bf16(np.linspace(-3, 3, 64))
    x[1, 9] = -0.0
    codes, b = kv8.quantize_rows(x)
    assert b[0] == 127 and not codes[0].any()                  # amax == 0: every code 0x00, the sign of -0 included
    assert codes[1, 9] == 0x80                                 # inside a live row -0 keeps its sign


def test_non_finite_rows():
    x = random_rows(3, 4)
    x[0, 11] = np.nan
    x[1, 0] = np.inf
    x[2, 63] = -np.inf
    codes, b = kv8.quantize_rows(x)
    assert np.all(codes == 0x7F) and np.all(b == 127)
    assert np.isnan(kv8.dequantize_rows(codes, b)).all()


def test_clamp_ends():
    x = np.zeros((4, 64), np.float32)
    big = kv8.from_bf16_bits(np.array([0x7F7F], np.uint16))[0]          # largest finite bf16, 1.99 * 2^127
    x[0, 0], x[0, 1] = big, np.float32(np.ldexp(1.0, 112))
    x[1, 0] = np.float32(np.ldexp(1.75, 118))                           # e = 110 exactly: the last unclamped row
    tiny = kv8.from_bf16_bits(np.array([0x0001], np.uint16))[0]         # smallest bf16 subnormal
    x[2, 0], x[2, 1] = tiny, -tiny
    x[3, 0], x[3, 1] = np.float32(np.ldexp(1.0, -110)), np.float32(-np.ldexp(1.0, -118))
    x[3, 2], x[3, 3] = np.float32(-np.ldexp(1.0, -120)), np.float32(np.ldexp(1.5, -120))
    codes, b = kv8.quantize_rows(x)
    assert b[0] == 127 + kv8.E_MAX and codes[0, 0] == 0x7E              # saturated to 448
    assert codes[0, 1] == 0x48                                          # 2^112 * 2^-110 = 4: exact
    assert kv8.dequantize_rows(codes, b)[0, 1] == np.float32(np.ldexp(1.0, 112))
    assert b[1] == 127 + kv8.E_MAX and codes[1, 0] == 0x7E
    assert b[2] == 127 + kv8.E_MIN and codes[2, 0] == 0x00 and codes[2, 1] == 0x80
    assert b[3] == 127 + kv8.E_MIN and codes[3, 0] == 0x38              # 2^-110 * 2^110 = 1.0
    assert codes[3, 1] == 0x82                                          # 2^-8: two subnormal steps of 2^-9
    assert codes[3, 2] == 0x80                                          # 2^-10: a tie between 0 and one step -> even
    assert codes[3, 3] == 0x01                                          # 1.5 * 2^-10 -> one step
