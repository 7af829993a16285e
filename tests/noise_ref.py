"""The device's inlet-noise stream restated on the host (not a test module): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel
random numbers: as easy as 1, 2, 3", SC'11) and the two mappings include/beacon_hip.h documents -- bcn_set_noise: the inlet value of
replica b, draw counter ctr, timestep k; bcn_shkadov_reset_random: the number of warm-up steps of a reset.  NumPy only, written from
the header and the paper: nothing here reads the kernels' constants."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
# the paper's multipliers and key increments (Weyl sequence: golden ratio, sqrt(3) - 1)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def _u32(x):
    """integers (any width or sign convention below 2^64) -> uint64 array holding the low 32 bits"""
    return np.asarray(x).astype(np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four 32-bit words per (counter, key), vectorised: every argument broadcasts against the others; uint64 arrays masked to
    32 bits, so the 32 x 32 -> 64 bit products are exact."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u32(x) for x in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def _key(seed):
    seed = int(seed)
    assert 0 <= seed < 1 << 64
    return seed & 0xFFFFFFFF, seed >> 32


def device_noise(seed, replica_offset, b, ctr, k, sigma, dtype):
    """uniform(-sigma, sigma) of replica b (local index; b, ctr, k broadcast), in the env's precision `dtype` (np.float32 /
    np.float64): counter (b + replica_offset, ctr, k, 0), key (low, high word of the seed); r = (w0 >> 8) 2^-24 in float32,
    ((w0 << 21) ^ (w1 >> 11)) 2^-53 in float64; (2 r - 1) sigma.  r and 2 r - 1 are exact in either precision: the product with
    sigma is the one rounding."""
    dtype = np.dtype(dtype).type
    k0, k1 = _key(seed)
    w0, w1, _, _ = philox4x32_10(np.asarray(b, dtype=np.int64) + int(replica_offset), ctr, k, 0, k0, k1)
    if dtype is np.float32:
        r = (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    else:
        assert dtype is np.float64
        r = ((w0 << np.uint64(21)) ^ (w1 >> np.uint64(11))).astype(np.float64) * 2.0 ** -53
    out = (dtype(2) * r - dtype(1)) * dtype(sigma)
    assert out.dtype == dtype
    return out


def drawn_count(seed, replica_offset, b, ctr, rand_steps):
    """The number of warm-up action steps a random-start reset draws for replica b at draw counter ctr: counter
    (b + replica_offset, ctr, 0, 1), the high word of w0 (rand_steps + 1) -- uniform on {0 .. rand_steps}."""
    k0, k1 = _key(seed)
    w0, _, _, _ = philox4x32_10(np.asarray(b, dtype=np.int64) + int(replica_offset), ctr, 0, 1, k0, k1)
    return ((w0 * np.uint64(int(rand_steps) + 1)) >> S32).astype(np.int64)
