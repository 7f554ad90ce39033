"""Host reference of the counter-based normal generator (include/mdt_hip.h; normal4() in csrc/k_elem.hip), numpy only.

Contract: for the global element index e = (sample0 + b) * C * L + c * L + l (a multiple of 4), quad = e >> 2; one Philox4x32-10
block (Salmon et al., SC'11) with counter (quad & 0xffffffff, quad >> 32, draw, 0) and key (seed & 0xffffffff, seed >> 32) gives
four 32-bit words r0..r3; Box-Muller turns them into the four normals of elements e .. e + 3:

    u0 = (float32(r0) + 1) * 2^-32, u1 = float32(r1) * 2^-32           (float32 arithmetic, bit-exact; u0 in (0, 1])
    ra = sqrt(-2 log u0), a = float32(6.283185307179586) * u1           (the product in float32)
    (ra cos a, ra sin a, rb cos b, rb sin b)                             (u2, u3 likewise for rb, b)

log, sqrt, sin and cos are evaluated in float64 on those float32 inputs, so the result is the value a correctly rounded fp32
device library would approach; the kernel's deviation from it is its logf / sqrtf / sincosf error alone.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or ints) holding 32-bit words, key: two.  Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def box_muller(r):
    """r: four arrays of 32-bit words.  Returns float64 (..., 4): the normals in the kernel's order."""
    k = np.float32(2.0 ** -32)
    one, two_pi = np.float32(1.0), np.float32(6.283185307179586)
    f = [np.asarray(w, dtype=np.uint64).astype(np.uint32).astype(np.float32) for w in r]       # round to nearest even, as (float)r
    u0, u1, u2, u3 = (f[0] + one) * k, f[1] * k, (f[2] + one) * k, f[3] * k
    assert all(u.dtype == np.float32 for u in (u0, u1, u2, u3))
    a, b = two_pi * u1, two_pi * u3
    assert a.dtype == np.float32
    ra = np.sqrt(-2.0 * np.log(u0.astype(np.float64)))
    rb = np.sqrt(-2.0 * np.log(u2.astype(np.float64)))
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], axis=-1)


def normals(seed, draw, sample0, B, C, L):
    """The (B, C, L) float64 normals of draw index `draw` for global samples sample0 .. sample0 + B - 1."""
    assert L % 4 == 0 and 0 <= seed < 2 ** 64 and 0 <= draw < 2 ** 32
    n = B * C * L
    quad = np.uint64(sample0 * C * L // 4) + np.arange(n // 4, dtype=np.uint64)
    r = philox4x32_10((quad & MASK, quad >> S32, draw, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return box_muller(r).reshape(B, C, L)
