"""The numpy definition of the projected form's fp8 K/V panels (engine option cross_kv_fp8; the C definition is the
comment of wm_cross_kv_fp8_quantize in include/whisper_mi355.h), built on oracle.fp8's e4m3 rounding.

A quantisation row is 64 bf16 values.  Per row: 64 OCP e4m3 codes and one exponent byte b = e + 127; the stored value
is e4m3(code) * 2^e.  Everything is computed in float64 from the bf16 bit patterns, so no step here rounds except the
e4m3 rounding itself.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from oracle.fp8 import e4m3_bits, e4m3_round

E_MIN, E_MAX = -110, 110


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """uint16 patterns of float32 values that are exactly bf16 (asserted)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not np.any(u & np.uint32(0xFFFF)), "input is not bf16-valued"
    return (u >> np.uint32(16)).astype(np.uint16)


def from_bf16_bits(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def row_exponent(amax_bits: np.ndarray) -> np.ndarray:
    """e of the definition from the bf16 pattern of amax (> 0, finite): amax = m 2^k, 1 <= m < 2, 448 = 1.75 2^8,
    e = k - 8 if m <= 1.75 else k - 7, clamped.  (A subnormal amax has exponent field 0: its k <= -127 lands on the
    lower clamp whichever way it is counted.)"""
    a = np.asarray(amax_bits, dtype=np.int64)
    k = (a >> 7) - 127
    e = np.where((a & 0x7F) <= 0x60, k - 8, k - 7)
    return np.clip(e, E_MIN, E_MAX)


def quantize_rows(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """x [N][64] bf16-valued float32 -> (codes uint8 [N][64], exponent bytes uint8 [N])."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2 and x.shape[1] == 64
    bits = bf16_bits(x)
    mag = (bits & np.uint16(0x7FFF)).astype(np.int64)
    amax = mag.max(axis=1)                                   # integer order = float order for magnitudes
    bad = (mag >= 0x7F80).any(axis=1)
    zero = amax == 0
    live = ~bad & ~zero
    e = np.zeros(x.shape[0], dtype=np.int64)
    e[live] = row_exponent(amax[live])
    codes = np.zeros(x.shape, dtype=np.uint8)
    if live.any():
        with np.errstate(over="ignore", under="ignore"):
            scaled = np.ldexp(x[live].astype(np.float64), (-e[live])[:, None].astype(np.int64))
            codes[live] = e4m3_bits(e4m3_round(scaled.astype(np.float32)))
    codes[bad] = 0x7F
    return codes, (e + 127).astype(np.uint8)


def e4m3_value(codes: np.ndarray) -> np.ndarray:
    """float64 values of e4m3 codes (0x7F / 0xFF: NaN)."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    s = np.where(c & 0x80, -1.0, 1.0)
    ex, m = (c >> 3) & 0xF, c & 7
    v = np.where(ex == 0, m * 2.0 ** -9, (8 + m) * np.ldexp(1.0, ex - 10))
    v = np.where((c & 0x7F) == 0x7F, np.nan, v)
    return s * v


def dequantize_rows(codes: np.ndarray, exps: np.ndarray) -> np.ndarray:
    """-> float32 [N][64]: e4m3(code) * 2^(b - 127), exact (float64 product, then a cast that does not round: see
    tests/test_kv8_ref.py)."""
    e = np.asarray(exps, dtype=np.uint8).astype(np.int64) - 127
    return np.ldexp(e4m3_value(codes), e[:, None]).astype(np.float32)
