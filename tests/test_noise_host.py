"""tests/noise_ref.py, the host restatement of the device's noise stream, checked on its own (no GPU): the known-answer vectors
published with Random123 for philox4x32-10, a scalar big-integer form of the same rounds, the law of both mappings and of the
drawn counts, and the high word of the seed.  tests/test_gpu_noise.py then holds the kernels to this restatement bit for bit."""
import numpy as np
import pytest

import noise_ref as NR

# Random123 examples/kat_vectors, philox4x32 with 10 rounds: (counter, key, expected)
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox_scalar(ctr, key, rounds=10):
    """the rounds of the paper on Python integers, one (counter, key) at a time"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_known_answer_vectors(ctr, key, want):
    assert philox_scalar(ctr, key) == want
    got = NR.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want
    assert philox_scalar(ctr, key, rounds=9) != want                     # the vectors tell 10 rounds from 9


def test_vectorised_form_equals_the_scalar_form_on_mixed_counters():
    rng = np.random.default_rng(1)
    args = rng.integers(0, 1 << 32, (6, 200), dtype=np.uint64)
    args[:, :8] = np.array([0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0xFFFF0000, 0x0000FFFF, 2], dtype=np.uint64)[None, :]
    args[2, 8:16] = np.arange(8)                                         # timesteps
    args[3, 8:16] = [0, 1] * 4                                           # noise draws and count draws
    got = np.stack(NR.philox4x32_10(*args))
    want = np.array([philox_scalar(tuple(int(x) for x in args[:4, i]), tuple(int(x) for x in args[4:, i])) for i in range(200)]).T
    assert np.array_equal(got, want.astype(np.uint64))
    # broadcasting: a column of replicas against a row of timesteps, scalars for the rest
    grid = np.stack(NR.philox4x32_10(np.arange(5)[:, None], 3, np.arange(7)[None, :], 0, 11, 22))
    assert grid.shape == (4, 5, 7)
    for b in range(5):
        for k in range(7):
            assert tuple(int(w) for w in grid[:, b, k]) == philox_scalar((b, 3, k, 0), (11, 22))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_law_of_the_mapping(dtype):
    """uniform(-sigma, sigma): |n| <= sigma, |mean| < 4 sigma / sqrt(3 N) (four standard errors), std within 1 % of
    sigma / sqrt(3) (its standard error at N = 65536 is 0.25 %)."""
    N, sigma = 65536, 0.1
    n = NR.device_noise(5, 0, np.arange(N), 0, 0, sigma, dtype)
    assert n.dtype == dtype and n.shape == (N,)
    n = n.astype(np.float64)
    print("MEASURED %s: max |n| %.6f mean %.2e (bound %.2e) std %.6f (sigma / sqrt 3 = %.6f)"
          % (np.dtype(dtype).name, np.abs(n).max(), n.mean(), 4 * sigma / np.sqrt(3 * N), n.std(), sigma / np.sqrt(3)))
    assert np.abs(n).max() <= float(dtype(sigma))
    assert abs(n.mean()) < 4 * sigma / np.sqrt(3 * N)
    assert abs(n.std() / (sigma / np.sqrt(3)) - 1.0) < 0.01
    # replicas, draw counters and timesteps are three different coordinates of the stream
    base = NR.device_noise(5, 0, np.arange(64), 0, 0, sigma, dtype)
    assert not np.array_equal(base, NR.device_noise(5, 0, np.arange(64), 1, 0, sigma, dtype))
    assert not np.array_equal(base, NR.device_noise(5, 0, np.arange(64), 0, 1, sigma, dtype))
    assert not np.array_equal(NR.device_noise(5, 0, np.arange(64), 1, 0, sigma, dtype), NR.device_noise(5, 0, np.arange(64), 0, 1, sigma, dtype))
    # the replica offset of a shard is added to the replica's index, nothing else
    assert np.array_equal(NR.device_noise(5, 37, np.arange(27), 2, 3, sigma, dtype), NR.device_noise(5, 0, np.arange(64), 2, 3, sigma, dtype)[37:])


def test_float64_mapping_uses_53_bits():
    """Two draws whose first words agree still differ in float64 through the second word; the float32 form reads the first alone."""
    n = NR.device_noise(5, 0, np.arange(4096), 0, 0, 1.0, np.float64)
    r = (n + 1.0) / 2.0 * 2.0 ** 53                                      # exact: 2 r - 1 and the product with sigma = 1 are
    assert np.array_equal(r, np.round(r)) and np.any(r.astype(np.uint64) & np.uint64((1 << 21) - 1))
    w0, w1, _, _ = NR.philox4x32_10(np.arange(4096), 0, 0, 0, 5, 0)
    assert np.array_equal(r.astype(np.uint64), (w0 << np.uint64(21)) ^ (w1 >> np.uint64(11)))


@pytest.mark.parametrize("R", [3, 400])
def test_drawn_count_stays_in_range_and_reaches_both_ends(R):
    n = NR.drawn_count(5, 0, np.arange(65536), 0, R)                     # a miss of one end: (R / (R + 1))^65536 < 1e-70
    assert n.dtype == np.int64 and int(n.min()) == 0 and int(n.max()) == R
    assert len(np.unique(n)) == R + 1
    # word 3 separates the count from the noise draw at the same (replica, counter, timestep 0)
    w_count = NR.philox4x32_10(np.arange(16), 0, 0, 1, 5, 0)[0]
    w_noise = NR.philox4x32_10(np.arange(16), 0, 0, 0, 5, 0)[0]
    assert not np.array_equal(w_count, w_noise)
    assert np.array_equal(NR.drawn_count(5, 1, np.arange(15), 2, R), NR.drawn_count(5, 0, np.arange(16), 2, R)[1:])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_high_word_of_the_seed_is_part_of_the_key(dtype):
    lo, full = 5, (7 << 32) | 5
    a = NR.device_noise(lo, 0, np.arange(64), 0, 0, 0.1, dtype)
    b = NR.device_noise(full, 0, np.arange(64), 0, 0, 0.1, dtype)
    assert not np.array_equal(a, b) and np.count_nonzero(a == b) <= 1
    assert not np.array_equal(NR.drawn_count(lo, 0, np.arange(64), 0, 400), NR.drawn_count(full, 0, np.arange(64), 0, 400))
    with pytest.raises(AssertionError):
        NR.device_noise(1 << 64, 0, 0, 0, 0, 0.1, dtype)
