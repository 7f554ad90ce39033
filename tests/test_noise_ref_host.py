"""CPU: the host reference of the counter-based generator (tests/noise_ref.py) against the published Philox4x32-10 known answers,
at the edges of the uniforms, and for the sharding rule the kernels promise."""
import math

import numpy as np

import noise_ref

# Random123's known-answer vectors for philox4x32 with 10 rounds (kat_vectors): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for counter, key, want in KAT:
        got = tuple(int(w) for w in noise_ref.philox4x32_10(counter, key))
        assert got == want, (counter, key, [hex(g) for g in got])
    # vectorised over arrays: the three blocks at once (one key per call: the third's)
    ctr = [np.array([k[0][j] for k in KAT], dtype=np.uint64) for j in range(4)]
    got = noise_ref.philox4x32_10(ctr, KAT[2][1])
    assert tuple(int(w[2]) for w in got) == KAT[2][2]


def test_edge_uniforms():
    # r0 = 2^32 - 1: float32(r0) + 1 rounds to 2^32, u0 == 1, log u0 == 0: a normal of exactly 0 whatever the angle
    z = noise_ref.box_muller((0xffffffff, 0x12345678, 0xffffffff, 0xffffffff))
    assert z.shape == (4,) and np.all(z == 0.0)
    # r0 = 0: the smallest u0 = 2^-32, the largest radius sqrt(-2 ln 2^-32) ~ 6.66
    rmax = math.sqrt(-2.0 * math.log(2.0 ** -32))
    assert 6.66 < rmax < 6.67
    r1 = np.array([0, 0x40000000, 0x80000000, 0xc0000000, 0xffffffff], dtype=np.uint64)
    z = noise_ref.box_muller((np.zeros(5, dtype=np.uint64), r1, np.zeros(5, dtype=np.uint64), r1))
    assert np.all(np.abs(z) <= rmax) and abs(z[0, 0] - rmax) < 1e-12 and z[0, 1] == 0.0
    # float32(r1) * 2^-32 reaches 1 for the largest words: the angle is then fp32(2 pi), the normals stay finite
    assert np.all(np.isfinite(z))
    # the order inside a quad: (ra cos a, ra sin a, rb cos b, rb sin b); a quarter turn swaps the roles
    q = noise_ref.box_muller((0, 0x40000000, 0x80000000, 0))
    assert abs(q[0]) < 1e-6 and abs(q[1] - rmax) < 1e-12
    rb = math.sqrt(-2.0 * math.log((2.0 ** 31 + 1) * 2.0 ** -32))
    assert abs(q[2] - rb) < 1e-6 and q[3] == 0.0


def test_sharding_and_keying():
    C, L = 16, 64
    for seed, draw in ((1234, 3), (0x9E3779B97F4A7C15, 0xFFFFFFFF)):
        for s, b in ((0, 4), (3, 2), (2 ** 24 - 2, 4)):
            whole = noise_ref.normals(seed, draw, 0, 5, C, L) if s < 5 else None
            part = noise_ref.normals(seed, draw, s, b, C, L)
            assert part.shape == (b, C, L) and part.dtype == np.float64
            if whole is not None:
                assert np.array_equal(part, whole[s: s + b])
    # across the 32-bit boundary of the quad index: a long batch ending past it equals the shard that starts before it
    s = 2 ** 24 - 2
    tail = noise_ref.normals(1234, 3, s + 1, 3, C, L)
    assert np.array_equal(tail, noise_ref.normals(1234, 3, s, 4, C, L)[1:])
    # every word of the key and the counter matters
    base = noise_ref.normals(1234, 3, 0, 2, C, L)
    for other in ((1234 + 2 ** 32, 3, 0), (1235, 3, 0), (1234, 4, 0), (1234, 3, 2 ** 24), (1234, 3, 1)):
        assert not np.array_equal(noise_ref.normals(*other, 2, C, L), base), other
    f = noise_ref.normals(7, 0, 0, 64, C, L)
    assert abs(f.mean()) < 4 / math.sqrt(f.size) and abs(f.var() - 1) < 0.02
