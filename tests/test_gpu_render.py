"""GPU tests of the device frames (VecEnv.renderer, Renderer.draw, bcn_render; csrc/render.hip): every frame BYTE-EQUAL to the NumPy
restatement of the pixel rules (tests/render_ref.py, itself checked on the CPU by tests/test_render_host.py) on the state downloaded
with get_state() and the stored action read from a snapshot -- field panels through the dword and the byte-wise store path, line
panels wider and narrower than the grid, non-finite values, the control strips after real steps --, then the replica list, a draw
replayed from a graph, both bindings, and the single-env mirror's render(mode="rgb_array").  States are written with set_state (and
stored actions with restore), so most tests take no solver step."""
import os

import numpy as np
import pytest
import torch

import render_ref as R
from beacon_amd import vec as V
from beacon_amd.envs import packaged_init
from beacon_amd.render import colormap_lut

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {"f32": np.float32, "f64": np.float64}
LUT = colormap_lut()


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")


def field_state(env, dtype, seed):
    """[B, 4, ny + 2, nx + 2]: seeded values reaching beyond (-0.5, 0.5) and (0, 1), with exact bin edges of both ranges and their
    neighbours, a NaN and both infinities planted in the scalar plane and in u"""
    dt = NP[dtype]
    rng = np.random.default_rng(seed)
    st = rng.uniform(-0.7, 1.2, (env.batch,) + env.state_shape()).astype(dt)
    edges = np.concatenate([(-0.5 + np.arange(257) / 256.0).astype(dt), (np.arange(257) / 256.0).astype(dt)])
    edges = np.concatenate([edges, np.nextafter(edges, dt(-np.inf)), np.nextafter(edges, dt(np.inf))])
    for plane in (0, 3):
        for b in range(env.batch):
            flat = st[b, plane, 1:-1, 1:-1].reshape(-1)
            pos = rng.choice(flat.size, edges.size + 3, replace=False)
            flat[pos[:-3]] = edges
            flat[pos[-3:]] = [np.nan, np.inf, -np.inf]
            st[b, plane, 1:-1, 1:-1] = flat.reshape(env.ny, env.nx)
    return st


def put_actions(env, values):
    """write the stored action (a_last / ia_last) of every replica through a snapshot"""
    snap = env.snapshot()
    name = "ia_last" if isinstance(env, V.VecMixing) else "a_last"
    v = snap.view(name)
    v.copy_(torch.as_tensor(np.asarray(values), device=DEV).to(v.dtype).reshape(v.shape))
    env.restore(snap)


def stored_actions(env):
    name = "ia_last" if isinstance(env, V.VecMixing) else "a_last"
    return env.snapshot().view(name).cpu().numpy()


def field_ref(env, dtype, st, ctrl, plane, scale, vmin, vmax, strip=None, lut=LUT):
    return np.stack([R.field_frame(st[b, plane], ctrl[b], scale, vmin, vmax, lut, NP[dtype], strip) for b in range(st.shape[0])])


def assert_same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ" % (what, bad, want.size))
    assert bad == 0, what


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_rayleigh_128x64_dword_path(dtype):
    _need_gpu()
    env = V.VecRayleigh(3, DEV, dtype, L=2.56, H=1.28)
    assert (env.nx, env.ny) == (128, 64)
    env.set_state(field_state(env, dtype, 1))
    acts = np.random.default_rng(2).uniform(-1.3, 1.3, (3, env.n_sgts))
    acts[0, :4] = [0.0625, -0.0625, 1.0, np.nan]
    put_actions(env, acts)
    st, ctrl = env.get_state().cpu().numpy(), stored_actions(env)
    assert st.dtype == NP[dtype] and np.isnan(st[:, 3]).sum() == 3 and np.isinf(st[:, 3]).sum() == 6
    for scale in (1, 2, 3):
        rd = env.renderer(scale=scale)
        assert rd.shape == (64 * scale + 64 * scale // 8, 128 * scale) and rd.shape[1] % 4 == 0
        assert_same(rd.draw(), field_ref(env, dtype, st, ctrl, 3, scale, -0.5, 0.5), "rayleigh %s scale %d" % (dtype, scale))
    for name, plane in (("u", 0), ("v", 1), ("p", 2)):
        got = env.renderer(scale=2, field=name, vmin=0.0, vmax=1.0, strip=0).draw()
        assert_same(got, field_ref(env, dtype, st, ctrl, plane, 2, 0.0, 1.0, strip=0), "rayleigh %s field %s" % (dtype, name))
    # a caller's table, an odd strip, a range that is no power of two
    lut = np.random.default_rng(3).integers(0, 256, (256, 3)).astype(np.uint8)
    got = env.renderer(scale=1, vmin=-0.3, vmax=0.9, strip=7, lut=lut).draw()
    assert_same(got, field_ref(env, dtype, st, ctrl, 3, 1, -0.3, 0.9, strip=7, lut=lut), "rayleigh %s own table" % dtype)
    env.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_odd_widths_byte_path(dtype):
    _need_gpu()
    env = V.VecRayleigh(2, DEV, dtype)                       # 50 x 50: 150 and 450 bytes per row, no multiple of 4
    assert (env.nx, env.ny) == (50, 50)
    env.set_state(field_state(env, dtype, 4))
    put_actions(env, np.random.default_rng(5).uniform(-1, 1, (2, env.n_sgts)))
    st, ctrl = env.get_state().cpu().numpy(), stored_actions(env)
    for scale in (1, 3):
        rd = env.renderer(scale=scale)
        assert (rd.shape[1] * 3) % 4 != 0
        assert_same(rd.draw(), field_ref(env, dtype, st, ctrl, 3, scale, -0.5, 0.5), "50x50 %s scale %d" % (dtype, scale))
    env.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_mixing_100x100(dtype):
    _need_gpu()
    env = V.VecMixing(2, DEV, dtype)
    env.set_ndt_act(1)                                       # one timestep per action step: the strip needs the stored action only
    env.reset()
    env.set_state(field_state(env, dtype, 6))
    st = env.get_state().cpu().numpy()
    rd = env.renderer(scale=2)
    assert rd.shape == (200 + 25, 200)
    # a reset stores action 1, as the reference's does (mixing.py:102)
    ctrl = [R.mixing_controls(1)] * 2
    assert_same(rd.draw(), field_ref(env, dtype, st, ctrl, 3, 2, 0.0, 1.0), "mixing %s after reset" % dtype)
    env.reset()                                              # the steps start from the reset fields: the planted values are no flow
    for a in range(5):
        env.step(np.asarray([a, (a + 2) % 5]))
        st = env.get_state().cpu().numpy()
        ctrl = [R.mixing_controls(a), R.mixing_controls((a + 2) % 5)]
        assert_same(rd.draw(), field_ref(env, dtype, st, ctrl, 3, 2, 0.0, 1.0), "mixing %s action %d" % (dtype, a))
    env.close()


LINE = {"burgers": (lambda dt: V.VecBurgers(3, DEV, dt), (0.3, 0.7, 0.5)),
        "shkadov": (lambda dt: V.VecShkadov(3, DEV, dt), (0.0, 2.0, 1.0)),
        "sloshing": (lambda dt: V.VecSloshing(3, DEV, dt, packaged_init("sloshing")), (0.25, 1.75, 1.0))}


def line_samples(name, st):
    return st[:, 0, 1:-1] if name == "sloshing" else st[:, 0]


def line_ref(name, dtype, st, ctrl, W, H, rng3):
    y = line_samples(name, st)
    return np.stack([R.line_frame(y[b], ctrl[b], W, H, rng3[0], rng3[1], rng3[2], NP[dtype]) for b in range(y.shape[0])])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", ["burgers", "shkadov", "sloshing"])
def test_line_panels(name, dtype):
    _need_gpu()
    make, table = LINE[name]
    env = make(dtype)
    env.reset()
    n = env.nx
    axes = lo, hi, ref = env._render_range()                # the reference's axes: what renderer() takes by default
    assert axes == pytest.approx(table, abs=1e-12)
    # a curve that leaves the axes on both sides, steps of many rows between neighbours, exact row edges; a NaN and an infinity in replica 1
    rng = np.random.default_rng(7)
    st = env.get_state().cpu().numpy()
    y = line_samples(name, st)
    x = np.linspace(0.0, 1.0, n)
    for b in range(3):
        y[b] = lo + (hi - lo) * (0.5 + 0.6 * np.sin(2 * np.pi * (b + 1.5) * x) + 0.2 * rng.uniform(-1, 1, n))
        y[b, rng.choice(n, 64, replace=False)] = hi - (hi - lo) * rng.integers(0, 129, 64) / 128.0
    y[1, n // 3] = np.nan
    y[1, n - 1] = np.inf
    env.set_state(st)
    st, ctrl = env.get_state().cpu().numpy(), stored_actions(env)
    assert not ctrl.any()
    small = {"burgers": 150, "shkadov": 300, "sloshing": 90}[name]      # fewer columns than samples, not dividing them; 150, 90: byte path
    assert small < n and n % small != 0
    for W, H in ((512, 128), (small, 50)):
        rd = env.renderer(width=W, height=H)
        assert rd.shape == (H + H // 8, W)
        want = line_ref(name, dtype, st, ctrl, W, H, axes)
        assert (want[1, :H] == R.RED).all(axis=2).all(axis=0).sum() >= 2          # the blown-up replica shows
        assert_same(rd.draw(), want, "%s %s %dx%d after reset" % (name, dtype, W, H))
    # one step with known actions from the reset state: the strip shows what the step stored
    env.reset()
    acts = np.asarray([[0.8, -0.55, 0.07, -1.0, 0.3][:env.n_actions], [-0.26, 0.9, -0.01, 0.5, 1.0][:env.n_actions], [0.0] * env.n_actions])
    env.step(acts if env.n_actions > 1 else acts[:, 0])
    st, ctrl = env.get_state().cpu().numpy(), stored_actions(env)
    assert ctrl.shape == (3, env.n_actions) and ctrl[:2].all()
    rd = env.renderer(width=256, height=64)
    want = line_ref(name, dtype, st, ctrl, 256, 64, axes)
    strip = want[:, 64:]
    assert (strip[0] == R.RED).all(axis=2).any() and (strip[1] == R.NEG).all(axis=2).any() and (strip[2] == 255).all()
    assert_same(rd.draw(), want, "%s %s after a step" % (name, dtype))
    # explicit axes
    rd = env.renderer(width=64, height=40, vmin=lo - 0.1, vmax=hi + 0.3, ref=lo, strip=5)
    want = np.stack([R.line_frame(line_samples(name, st)[b], ctrl[b], 64, 40, lo - 0.1, hi + 0.3, lo, NP[dtype], 5) for b in range(3)])
    assert_same(rd.draw(), want, "%s %s own axes" % (name, dtype))
    env.close()


def test_replicas_in_order_and_nothing_else_written():
    _need_gpu()
    env = V.VecRayleigh(3, DEV, "f32")
    env.reset()
    env.set_state(field_state(env, "f32", 8))
    put_actions(env, np.random.default_rng(9).uniform(-1, 1, (3, env.n_sgts)))
    every = env.renderer(scale=2).draw().clone()
    before = (env.snapshot().buf.clone(), env.out_buf.clone())
    rd = env.renderer(replicas=[2, 0], scale=2)
    got = rd.draw()
    assert got.shape[0] == 2 and torch.equal(got[0], every[2]) and torch.equal(got[1], every[0])
    assert torch.equal(env.snapshot().buf, before[0]) and torch.equal(env.out_buf, before[1])
    # a device tensor is not read on the host: an index outside the batch leaves its frame as it was
    rd = env.renderer(replicas=torch.tensor([1, 7, -1], device=DEV), scale=2)
    rd.frames.fill_(77)
    got = rd.draw()
    assert torch.equal(got[0], every[1]) and bool((got[1:] == 77).all())
    with pytest.raises(ValueError, match="replica indices"):
        env.renderer(replicas=[0, 3])
    # a caller's buffer, and its checks
    out = torch.zeros_like(every)
    assert env.renderer(scale=2).draw(out=out) is out and torch.equal(out, every)
    with pytest.raises(ValueError, match="out must be"):
        env.renderer(scale=2).draw(out=out[:2])
    env.close()
    with pytest.raises(RuntimeError, match="closed"):
        rd.draw()


def test_draw_in_a_graph_and_both_bindings():
    _need_gpu()
    env = V.VecBurgers(4, DEV, "f32")
    env.reset()
    rd = env.renderer(width=128, height=32)
    first = rd.draw().clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rd.draw()
    env.step(np.asarray([0.9, -0.9, 0.3, 0.0]))
    g.replay()
    replayed = rd.frames.clone()
    eager = env.renderer(width=128, height=32).draw()
    assert torch.equal(replayed, eager) and not torch.equal(replayed, first)
    had = env.use_torch_ops(False)                             # the same entry point through ctypes
    assert env._ops is None
    assert torch.equal(env.renderer(width=128, height=32).draw(), eager) and torch.equal(rd.draw(), eager)
    env.use_torch_ops(True)
    assert torch.equal(rd.draw(), eager)
    # the library's own argument checks
    from beacon_amd import _lib
    cfg = env._render_cfg(1, 128, 32, None, "scalar", None, None, None)
    cfg.hi = cfg.lo
    with pytest.raises(_lib.BeaconHipError, match="hi must exceed lo"):
        V.Renderer(env, cfg, None, None)
    env.close()
    ode = V.VecLorenz(2, DEV, "f32")
    import ctypes as C
    H, W = C.c_int(), C.c_int()
    assert ode.lib.bcn_render_shape(ode.h, C.byref(cfg), C.byref(H), C.byref(W)) == 3      # BCN_ERR_UNSUPPORTED
    ode.close()


def test_renderer_survives_set_ndt_act():
    _need_gpu()
    env = V.VecRayleigh(2, DEV, "f32")
    rd = env.renderer(scale=1)
    env.set_ndt_act(2)                                         # a new handle: fields all zero again
    env.set_state(field_state(env, "f32", 10))
    st, ctrl = env.get_state().cpu().numpy(), stored_actions(env)
    assert_same(rd.draw(), field_ref(env, "f32", st, ctrl, 3, 1, -0.5, 0.5), "after set_ndt_act")
    env.close()


def test_mirror_rgb_array(tmp_path):
    _need_gpu()
    from beacon_amd import envs
    env = envs.rayleigh(dtype="f32")
    env.reset()
    env.vec.set_ndt_act(2)
    env.reset()
    env.step([0.5, -0.5] * 5)
    img = env.render(mode="rgb_array")
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (50 + 6, 50, 3)
    assert np.array_equal(img, env.vec.render_rgb()[0].cpu().numpy())
    st, ctrl = env.vec.get_state().cpu().numpy(), stored_actions(env.vec)
    assert np.array_equal(img, field_ref(env.vec, "f32", st, ctrl, 3, 1, -0.5, 0.5)[0]) and (img[50:] != 255).any()
    pytest.importorskip("matplotlib")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        assert env.render() is None                            # the default mode still writes what it wrote
        assert os.path.exists(os.path.join("render", "temperature", "0.png"))
        assert os.path.exists(os.path.join("render", "field", "field_0.dat")) and os.path.exists(os.path.join("render", "action", "a_0.dat"))
    finally:
        os.chdir(cwd)
    env.close()
