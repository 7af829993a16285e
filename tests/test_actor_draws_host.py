"""The conditions that tests/test_gpu_actor_edges.py relies on, checked with the reference alone (no GPU): the constructed draws
of tests/actor_draws.py reach both tails of Box-Muller in both precisions, the global replica index wraps inside the batch, the
per-radius error metric separates the header's float32 formula from its obvious mis-statement, and the categorical tail case
keeps enough draws outside its exemption."""
import numpy as np
import pytest

import actor_draws as D
import actor_ref as R
import noise_ref as N

DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


def test_scan_is_deterministic_and_chunking_does_not_show():
    ctr = D.extreme_counters()
    assert ctr is D.extreme_counters()                       # one scan serves every caller
    assert ctr.shape == (D.B,) and ctr.dtype == np.int64 and ctr.min() >= 0 and ctr.max() < D.N_SCAN and not ctr.flags.writeable
    # against a plain per-row scan of a short range that crosses a chunk border
    n = D.CHUNK + 37
    got = D.extreme_counters(D.SEED, D.OFFSET, 5, n)
    assert np.array_equal(got, D.extreme_counters.__wrapped__(D.SEED, D.OFFSET, 5, n))       # a second scan finds the same
    for b in range(5):
        k = R.words(D.SEED, D.OFFSET, b, np.arange(n), 0)[0] >> R.U8
        assert got[b] == (k.argmin() if b % 2 == 0 else k.argmax()), b
    # another key or another offset gives other counters: the scan reads both
    assert not np.array_equal(got, D.extreme_counters(D.SEED & 0xFFFFFFFF, D.OFFSET, 5, n))
    assert not np.array_equal(got, D.extreme_counters(D.SEED, 0, 5, n))


@DTYPES
def test_radii_reach_both_tails(dtype):
    u1, _, radius = D.pair0(D.extreme_counters(), dtype)
    print("radii %s: even %.3g .. %.3g, odd %.3g .. %.3g" % (np.dtype(dtype).name, radius[0::2].min(), radius[0::2].max(),
                                                            radius[1::2].min(), radius[1::2].max()))
    assert radius[0::2].min() >= 4.0 and radius[1::2].max() <= 1e-2
    assert radius.min() > 0.0 and np.isfinite(radius).all()
    # the odd rows are in the branch k >= 2^23 of the float32 formula, the even rows in the other
    assert (u1[1::2] > 0.5).all() and (u1[0::2] < 0.5).all()


def test_global_index_wraps_inside_the_batch():
    assert N._u32(np.arange(5) + D.OFFSET).tolist() == [0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF, 0, 1]
    k0, k1 = N._key(D.SEED)
    assert (k0, k1) == (0x87654321, 0x12345678)
    ctr = D.extreme_counters()[:5]
    for j in (0, 1):
        mine = np.stack(R.words(D.SEED, D.OFFSET, np.arange(5), ctr, j))
        wrapped = np.stack(N.philox4x32_10(np.array([0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF, 0, 1], dtype=np.uint64), ctr, j, 2, k0, k1))
        assert np.array_equal(mine, wrapped)
        # rows 3 and 4 are the rows 0 and 1 of an unsharded batch
        assert np.array_equal(mine[:, 3:], np.stack(R.words(D.SEED, 0, np.arange(2), ctr[3:], j)))
    # the draw counter is a 32-bit word as well: 2^32 - 1 is followed by 0
    assert np.array_equal(np.stack(R.words(D.SEED, D.OFFSET, 7, 2 ** 32, 0)), np.stack(R.words(D.SEED, D.OFFSET, 7, 0, 0)))
    assert not np.array_equal(np.stack(R.words(D.SEED, D.OFFSET, 7, 2 ** 32 - 1, 0)), np.stack(R.words(D.SEED, D.OFFSET, 7, 0, 0)))


def test_metric_separates_the_float32_formula_from_its_misstatement():
    """max |z - z_ref| / radius_ref over the odd rows (small radii): forming u1 in float32 and taking its log is wrong by more than
    1e-2 there, the header's complement form stays below 1e-6.  This pins the metric's sensitivity, not the kernel."""
    ctr = D.extreme_counters()
    w = R.words(D.SEED, D.OFFSET, np.arange(D.B), ctr, 0)
    z_ref = R.normals(D.SEED, D.OFFSET, np.arange(D.B), ctr, 2, np.float32)
    radius = D.pair0(ctr, np.float32)[2]
    err = {}
    for complement in (False, True):
        z = np.stack(D.f32_pair(w[0], w[1], complement), axis=1).astype(np.float64)
        e = np.abs(z - z_ref).max(axis=1) / radius
        err[complement] = (e[0::2].max(), e[1::2].max())
        # what the suite's case-wide metric makes of the same draws
        print("f32 pair, complement form %s: even rows %.3e, odd rows %.3e; / max(1, max |z|): %.3e"
              % (complement, e[0::2].max(), e[1::2].max(), np.abs(z - z_ref).max() / max(1.0, np.abs(z_ref).max())))
    assert err[False][1] > 1e-2, err
    assert max(err[True]) < 1e-6, err
    assert err[False][0] < 1e-6, err                       # the large radii do not tell the two apart: the small ones are needed


@DTYPES
def test_categorical_tail_case_conditions(dtype):
    """The reference alone on the case of test_gpu_actor_edges.py: the exemption is rare enough to rely on, every class keeps at
    least 10 draws outside it, and the two rare classes are drawn."""
    bias = np.log(np.array(D.TAIL_P)).astype(dtype).astype(np.float64)        # what a device buffer of this precision stores
    dist = R.log_softmax(np.tile(bias, (D.B, 1)))
    a, exempt, u = D.tail_classes(dist, D.extreme_counters(), dtype)
    counts = np.bincount(a[~exempt], minlength=4)
    print("categorical tails %s: exempt %d of %d, classes outside the exemption %s" % (np.dtype(dtype).name, exempt.sum(), D.B, counts.tolist()))
    assert exempt.mean() <= D.CAP_TAIL, exempt.mean()
    assert counts.min() >= 10, counts
    assert (a[0::2] <= 1).all() and (a[1::2] >= 2).all()                      # small u on even rows, u near 1 on odd rows
    # the rare classes are rarer than the suite's general exemption is wide: only DELTA_TAIL can check them
    assert min(D.TAIL_P) < 1e-5 and D.DELTA_TAIL < min(D.TAIL_P) / 8
