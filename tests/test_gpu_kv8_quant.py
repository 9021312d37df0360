"""wm_cross_kv_fp8_quantize (the quantiser of the projected form's fp8 K/V panels, option cross_kv_fp8) against its
numpy definition tests/kv8_ref.py: codes and exponent bytes bit for bit, on ~1000 random rows spanning 40 binades plus
the forcing rows of the definition's corners, with guard bytes around both outputs and a row count that is no
multiple of the kernel's 32 rows per block."""
import numpy as np
import pytest
import torch

from tests import kv8_ref as kv8
from vlog_amd.dims import model_dims
from vlog_amd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

GUARD = 256


def _bits_row(patterns):
    """A 64-value row from bf16 bit patterns (zero-filled)."""
    r = np.zeros(64, np.uint16)
    r[:len(patterns)] = patterns
    return kv8.from_bf16_bits(r)


def forcing_rows():
    rows = []
    for k in (-100, -20, -1, 0, 3, 60, 100):
        at = int(kv8.bf16_bits(np.array([np.ldexp(1.75, k)], np.float32))[0])       # amax = 448 * 2^(k - 8) exactly
        rows.append(_bits_row([at, at | 0x8000]))
        rows.append(_bits_row([at + 1, 0x8000 | (at - 1)]))                          # the next bf16 above it
    # e4m3 ties: a row with amax 256 * 2^-1 ... scaled values are the bf16 values themselves times a power of two, so
    # bf16 mantissas xxx1000 are exactly half way between two codes, for even and odd xxx, in several binades
    amax = int(kv8.bf16_bits(np.array([np.ldexp(1.5, 4)], np.float32))[0])
    ties = []
    for ex in range(118, 132):
        for xxx in range(8):
            ties.append((ex << 7) | (xxx << 4) | 0x8)
    for s in range(0, len(ties), 31):
        part = ties[s:s + 31]
        rows.append(_bits_row([amax] + part + [p | 0x8000 for p in part]))
    # in and below the e4m3 subnormal range of the row: amax 1.0 * 2^8 scales to 256 (e = 0), subnormals are below 2^-6
    sub = []
    for ex in range(127 - 14, 127 - 5):
        for m in (0x00, 0x08, 0x10, 0x40, 0x48, 0x7F):
            sub.append((ex << 7) | m)
    a256 = int(kv8.bf16_bits(np.array([256.0], np.float32))[0])
    for s in range(0, len(sub), 31):
        part = sub[s:s + 31]
        rows.append(_bits_row([a256] + part + [p | 0x8000 for p in part]))
    rows.append(_bits_row([a256, 0x8000, 0x0000, 0x8000]))                           # -0 inside a live row
    rows.append(_bits_row([0x8000] * 5))                                             # zeros and -0 only: amax == 0
    rows.append(np.zeros(64, np.float32))
    rows.append(_bits_row([0x7FC0, a256]))                                           # NaN
    rows.append(_bits_row([a256, 0x7F80]))                                           # +inf
    rows.append(_bits_row([0xFF80] + [a256] * 63))                                   # -inf
    rows.append(_bits_row([0x7F7F, 0x7A00, 0xFF7F]))                                 # past the upper clamp: saturation
    rows.append(_bits_row([0x0001, 0x8001, 0x007F]))                                 # bf16 subnormals: the lower clamp
    rows.append(_bits_row([(17 << 7), 0x8000 | (10 << 7), (12 << 7) | 0x40]))        # amax 2^-110 at the lower clamp
    return np.stack(rows)


@pytest.fixture(scope="module")
def eng():
    from vlog_amd.engine import GpuEngine
    dims = model_dims("tiny")
    return GpuEngine(dims, synthetic_state_dict(dims, seed=0), 0)


def test_quantize_kernel_bit_exact_with_guards(eng):
    g = np.random.default_rng(11)
    n_rand = 1000
    scale = np.ldexp(1.0, g.integers(-20, 20, size=(n_rand, 1)))
    x = (g.standard_normal((n_rand, 64)) * scale * np.ldexp(1.0, g.integers(-8, 1, size=(n_rand, 64)))).astype(np.float32)
    x = torch.from_numpy(x).bfloat16().float().numpy()
    x = np.concatenate([x, forcing_rows()])
    if x.shape[0] % 32 == 0:
        x = x[:-1]
    n = x.shape[0]
    assert n % 32 != 0
    xb = torch.from_numpy(kv8.bf16_bits(x).astype(np.int16)).view(torch.bfloat16).cuda()
    cbuf = torch.full((GUARD + n * 64 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ebuf = torch.full((GUARD + n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    codes, exps = eng.cross_kv_fp8_quantize(xb, cbuf[GUARD:GUARD + n * 64], ebuf[GUARD:GUARD + n])
    torch.cuda.synchronize()
    rc, rb = kv8.quantize_rows(x)
    gc, gb = codes.cpu().numpy().reshape(n, 64), exps.cpu().numpy()
    bad_b = np.flatnonzero(gb != rb)
    assert bad_b.size == 0, (bad_b[:8], gb[bad_b[:8]], rb[bad_b[:8]])
    bad_c = np.argwhere(gc != rc)
    assert bad_c.size == 0, [(int(r), int(c), hex(kv8.bf16_bits(x[r:r + 1, c:c + 1])[0, 0]), hex(gc[r, c]), hex(rc[r, c]))
                             for r, c in bad_c[:8]]
    cb, eb = cbuf.cpu().numpy(), ebuf.cpu().numpy()
    assert (cb[:GUARD] == 0xA5).all() and (cb[-GUARD:] == 0xA5).all()
    assert (eb[:GUARD] == 0x5A).all() and (eb[-GUARD:] == 0x5A).all()


def test_quantize_rejects_bad_calls(eng):
    x = torch.zeros((3, 32), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        eng.cross_kv_fp8_quantize(x)
    codes, exps = eng.cross_kv_fp8_quantize(torch.zeros((0, 64), dtype=torch.bfloat16, device="cuda"))
    assert codes.numel() == 0 and exps.numel() == 0
