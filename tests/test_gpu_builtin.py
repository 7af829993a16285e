"""The rows of csrc/ns2d_builtin.h on the device: an env of each constructs on the library's own register-resident kernel, and a
grid that is no row gets a plugin.  No step is taken.

Nothing here reads the reference tree."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

if torch.cuda.is_available():
    from beacon_amd import vec as V


def _env(kind, nx, ny, f64, batch=2):
    from beacon_amd import jit
    n = (50.0, 100.0)[kind]
    dt = "f64" if f64 else "f32"
    if kind == 0:
        return V.VecRayleigh(batch, DEV, dt, None, L=jit._extent(nx, n), H=jit._extent(ny, n))
    return V.VecMixing(batch, DEV, dt, L=jit._extent(nx, n), H=jit._extent(ny, n))


def test_every_builtin_row_constructs_on_the_librarys_own_kernel():
    from beacon_amd import jit
    rows = jit.builtin_rows()
    assert len(rows) == 10
    for b in rows:
        env = _env(b["kind"], b["nx"], b["ny"], b["f64"])
        try:
            assert (env.nx, env.ny) == (b["nx"], b["ny"])
            assert env.set_variant(1) == 1 and getattr(env, "_plugin", None) is None, b
        finally:
            env.close()
    # 150x50 is a row in float32 only: in float64 it is an on-demand grid
    assert (150, 50, True, 0) not in jit.BUILTIN_GRIDS and (150, 50, True, 0) in jit.TEST_GRIDS
    env = _env(0, 150, 50, True)
    try:
        p = getattr(env, "_plugin", None)
        assert (env.nx, env.ny) == (150, 50) and p is not None and p.verified is True and env.set_variant(1) == 1
    finally:
        env.close()
