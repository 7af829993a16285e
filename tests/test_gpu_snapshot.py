"""Full on-device env snapshots on the GPU: VecEnv.snapshot / restore / fork (csrc/snapshot.hip, include/beacon_hip.h:
bcn_snapshot_*).  The feature moves bytes, so every comparison is bitwise (torch.equal): there is no tolerance to state.
That a replica's result depends neither on the run nor on its index is established by tests/test_gpu_parity.py; these tests
lean on it.  No test passes an out-of-range index in a device tensor (the kernel's guard exists for memory safety)."""
import numpy as np
import pytest
import torch

import beacon_amd
from beacon_amd import jit
from beacon_amd import vec as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (class, constructor kwargs, batch, what to do after construction)
CASES = {
    "rayleigh": (V.VecRayleigh, {}, 37, None),                          # 50x50: the built-in register-resident kernel
    "rayleigh_generic": (V.VecRayleigh, {}, 37, lambda e: e.set_variant(0)),
    "mixing": (V.VecMixing, {}, 37, lambda e: e.set_ndt_act(5)),        # 100x100
    "burgers500": (V.VecBurgers, dict(nx=500), 37, None),
    "burgers497": (V.VecBurgers, dict(nx=497), 37, None),               # rows of 1988 / 3976 bytes: not multiples of 16
    "shkadov": (V.VecShkadov, dict(n_jets=10), 37, None),
    "sloshing": (V.VecSloshing, {}, 37, None),
    "lorenz": (V.VecLorenz, {}, 300, None),
    "vortex": (V.VecVortex, {}, 300, None),
}


def _on_demand(env):
    """a grid the library does not carry: its register-resident kernel is compiled for it (beacon_amd/jit.py)"""
    env.set_ndt_act(20)
    assert getattr(env, "_plugin", None) is not None and env.set_variant(1) == 1


# odd 2D grids without a built-in kernel (rows of 53 x 67 / 52 x 131 cells: not multiples of 16 bytes in float32)
CASES["rayleigh_51x65"] = (V.VecRayleigh, dict(L=jit._extent(51, 50.0), H=jit._extent(65, 50.0)), 37, _on_demand)    # two rows per lane
CASES["rayleigh_50x129"] = (V.VecRayleigh, dict(L=jit._extent(50, 50.0), H=jit._extent(129, 50.0)), 37, _on_demand)  # hybrid: fields in HBM
ON_DEMAND = ("rayleigh_51x65", "rayleigh_50x129")
TWO_D = ("rayleigh", "rayleigh_generic", "mixing")
NOISY = ("burgers500", "burgers497", "shkadov")
K, M = 3, 4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")


def make(case, dtype, batch=None):
    cls, kw, B, post = CASES[case]
    env = cls(B if batch is None else batch, DEV, dtype, **kw)
    if post is not None:
        post(env)
    return env


def actions(env, n, seed):
    """n steps of seeded random actions [n, B, ...] on the device, in the env's action type"""
    g = torch.Generator().manual_seed(seed)
    if env.action_is_int:
        hi = 4 if isinstance(env, V.VecMixing) else 3
        return torch.randint(0, hi, (n, env.batch), generator=g, dtype=torch.int32).to(DEV)
    shape = (n, env.batch) if env.n_actions == 1 and not isinstance(env, V.VecRayleigh) else (n, env.batch, env.n_actions)
    return (2.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 1.0).to(device=DEV, dtype=env.tdtype)


def noises(env, n):
    return [env.draw_noise() for _ in range(n)] if env.needs_noise else [None] * n


def outputs(env):
    out = [env.obs.clone(), env.rwd.clone(), env.done.clone(), env.trunc.clone(), env.status.clone()]
    if hasattr(env, "sweeps"):
        out.append(env.sweeps.clone())
    return out


def run(env, acts, nz, repeat_last=False):
    """step through acts (the last one as step(None) when repeat_last) and record every step's outputs"""
    rec = []
    for i in range(acts.shape[0]):
        a = None if (repeat_last and i == acts.shape[0] - 1) else acts[i]
        env.step(a, nz[i])
        rec.append(outputs(env))
    return rec


def same(r0, r1):
    return all(torch.equal(x, y) for s0, s1 in zip(r0, r1) for x, y in zip(s0, s1))


def stp_of(env):
    return torch.as_tensor(env.get_stp().astype(np.int32))


# ---- 1. resume is exact: every env, both dtypes -----------------------------------------------------------------------------------
BUILT_IN = [c for c in CASES if c not in ON_DEMAND]
RESUME = ([(c, dt, "plain") for c in BUILT_IN for dt in ("f32", "f64")] +
          [(c, "f32", fl) for c in BUILT_IN for fl in ("episode_end", "repeat_last")] +
          [(c, dt, "explicit_noise") for c in NOISY for dt in ("f32", "f64")])


@pytest.mark.parametrize("case,dtype,flavour", RESUME)
def test_resume_is_exact(case, dtype, flavour):
    """reset, K steps, snapshot, M steps recorded, restore, the same M steps again: every output of every step equal, and the
    outputs restore() returns are those of step K.  flavour: plain (burgers / shkadov: device noise, so the draw counters matter),
    episode_end (the episode ends inside the M steps: a wrong stp shows), repeat_last (the last step is step(None): a wrong stored
    action shows), explicit_noise.  rayleigh and shkadov, plain: set_state + set_stp alone do NOT reproduce the M steps."""
    _need_gpu()
    env = make(case, dtype)
    env.reset()
    if flavour == "episode_end":
        env.set_stp(env.n_act - K - 2)
    acts = actions(env, K + M, 11)
    nz = noises(env, K + M) if flavour == "explicit_noise" else [None] * (K + M)
    run(env, acts[:K], nz[:K])
    at_k = outputs(env)
    state_k, stp_k = env.get_state(), env.get_stp()
    snap = env.snapshot()
    rec0 = run(env, acts[K:], nz[K:], flavour == "repeat_last")
    if flavour == "episode_end":
        assert int(rec0[1][2].min()) == 1 and int(rec0[0][2].max()) == 0          # done raised in the second of the M steps
    obs, rwd, done, trunc = env.restore(snap)
    assert obs is env.obs and rwd is env.rwd and done is env.done and trunc is env.trunc
    assert all(torch.equal(x, y) for x, y in zip(outputs(env)[:5], at_k[:5]))
    rec1 = run(env, acts[K:], nz[K:], flavour == "repeat_last")
    assert same(rec0, rec1)
    if flavour == "plain" and case in ("rayleigh", "shkadov"):
        # negative control: what existed before snapshots carries the fields and the episode counter only
        env.set_state(state_k)
        env.set_stp(stp_k)
        assert not same(rec0, run(env, acts[K:], nz[K:]))


@pytest.mark.parametrize("case,dtype", [("rayleigh_51x65", "f32"), ("rayleigh_50x129", "f32"), ("rayleigh_51x65", "f64")])
def test_resume_on_an_on_demand_grid_in_a_used_handle(case, dtype):
    """An odd grid on its on-demand kernel: the snapshot continues exactly in the same env and in ANOTHER handle that has run
    something else before (so us / vs, the work arrays and the kernel's field scratch hold another run's leftovers: they are
    not state)."""
    _need_gpu()
    env, other = make(case, dtype), make(case, dtype)
    env.reset()
    acts = actions(env, K + M, 13)
    run(env, acts[:K], [None] * K)
    snap = env.snapshot()
    rec0 = run(env, acts[K:], [None] * M)
    assert int(rec0[-1][5].max()) > 1                                  # the Jacobi solve has work to do
    env.restore(snap)
    assert same(rec0, run(env, acts[K:], [None] * M))
    other.reset()
    run(other, actions(other, 2, 14), [None] * 2)
    other.restore(snap)
    assert same(rec0, run(other, acts[K:], [None] * M))


def test_generator_comes_back_on_an_identity_restore_only():
    _need_gpu()
    env = make("burgers500", "f32")
    env.reset()
    run(env, actions(env, K, 15), noises(env, K))
    snap = env.snapshot()
    n1 = env.draw_noise()
    env.draw_noise()
    env.restore(snap)
    assert torch.equal(env.draw_noise(), n1)
    env.restore(snap, src=torch.arange(env.batch, dtype=torch.int32, device=DEV))      # a gather leaves the generator alone
    assert not torch.equal(env.draw_noise(), n1)


@pytest.mark.parametrize("case", ["burgers500", "shkadov"])
def test_forks_of_one_source_draw_different_device_noise(case):
    """The draw counter is copied, the Philox counter is keyed by the replica's own index: copies of replica 0 part under device
    noise and stay identical under an explicit noise tensor with equal rows."""
    _need_gpu()
    env = make(case, "f32", 64)
    env.reset()
    run(env, actions(env, K, 16), [None] * K)
    zero = torch.zeros(env.batch, dtype=torch.int32, device=DEV)
    a = actions(env, 1, 17)[0]
    a = a[:1].expand_as(a).contiguous()
    env.fork(zero)
    st = env.get_state()
    assert torch.equal(st, st[:1].expand_as(st))
    pre = env.snapshot()
    env.step(a, None)
    st = env.get_state()
    assert not torch.equal(st[1], st[0]) and not torch.equal(st[2], st[1])
    env.restore(pre)
    nz = env.draw_noise()
    env.step(a, nz[:1].expand_as(nz).contiguous())
    st = env.get_state()
    assert torch.equal(st, st[:1].expand_as(st))


# ---- 2. fork is a gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [("rayleigh", "f32"), ("mixing", "f64"), ("shkadov", "f32"), ("vortex", "f64"),
                                        ("burgers497", "f64"), ("burgers497", "f32")])
def test_fork_is_a_gather(case, dtype):
    _need_gpu()
    B = 64
    g = torch.Generator().manual_seed(5)
    src = torch.cat([torch.randperm(B // 2, generator=g), torch.randint(0, B, (B // 2,), generator=g)]).to(torch.int32)
    A, T = make(case, dtype, B), make(case, dtype, B)
    A.reset()
    T.reset()
    acts = actions(A, K + 1, 23)
    run(A, acts[:K], noises(A, K))
    T.restore(A.snapshot())
    assert torch.equal(T.snapshot().buf, A.snapshot().buf)
    A.fork(src.to(DEV))
    sd = src.long().to(DEV)
    sa, st = A.snapshot(), T.snapshot()
    assert torch.equal(A.get_state(), T.get_state()[sd])
    assert torch.equal(sa.view("stp"), st.view("stp")[sd])
    assert torch.equal(A.obs, T.obs[sd])
    nz = noises(T, 1)[0]
    A.step(acts[K][sd], None if nz is None else nz[sd])
    T.step(acts[K], nz)
    assert torch.equal(A.obs, T.obs[sd]) and torch.equal(A.rwd, T.rwd[sd]) and torch.equal(A.done, T.done[sd])
    assert torch.equal(A.get_state(), T.get_state()[sd])
    # the scratch snapshot is kept and reused
    p = A._fork_snap.buf.data_ptr()
    A.fork(list(range(B)))
    assert A._fork_snap.buf.data_ptr() == p


# ---- 3. a bank taken from another batch, with a mask ------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype,other_grid", [("rayleigh", "f32", dict(L=2.0)), ("burgers497", "f32", dict(nx=500)),
                                                   ("lorenz", "f64", dict(rho=20.0))])
def test_bank_of_another_batch_with_mask(case, dtype, other_grid):
    _need_gpu()
    NB, B = 5, 37
    bank_env, env = make(case, dtype, NB), make(case, dtype, B)
    bank_env.reset()
    env.reset()
    ab = actions(bank_env, K + 1, 31)
    run(bank_env, ab[:K], noises(bank_env, K))
    run(env, actions(env, 2, 32), noises(env, 2))
    bank = bank_env.snapshot()
    assert bank.batch == NB and bank.buf.numel() < env.snapshot().buf.numel()
    pre = env.snapshot()
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, NB, (B,), generator=g, dtype=torch.int32).to(DEV)
    mask = (torch.arange(B) % 3 != 0).to(torch.uint8).to(DEV)

    # refused on the host, before any launch, and nothing changes
    cls, kw, _, _ = CASES[case]
    others = [cls(NB, DEV, dtype, **dict(kw, **other_grid)), make(case, "f64" if dtype == "f32" else "f32", NB),
              (V.VecVortex if case == "lorenz" else V.VecLorenz)(NB, DEV, dtype)]
    with pytest.raises(ValueError):
        env.restore(bank)                                            # 5 replicas into 37 without src
    for o in others:
        o.reset()
        with pytest.raises(ValueError):
            env.restore(o.snapshot(), src=src)
    with pytest.raises(ValueError):
        env.restore(bank, src=[NB] * B)                              # host indices are checked
    with pytest.raises(ValueError):
        env.restore(bank, src=np.full(B, -1))
    with pytest.raises(ValueError):
        env.restore(bank.to("cpu"), src=src)
    assert torch.equal(env.snapshot().buf, pre.buf)

    env.restore(bank, src=src, mask=mask)
    post = env.snapshot()
    on, sd = mask.bool(), src.long()
    for name in post.names():
        v, v0, vb = post.view(name), pre.view(name), bank.view(name)
        if name == "fields":                                         # [planes, n, ...]: replicas on axis 1
            v, v0, vb = v.transpose(0, 1), v0.transpose(0, 1), vb.transpose(0, 1)
        assert torch.equal(v[~on], v0[~on]), name                    # masked-off replicas keep state, stp and output rows
        assert torch.equal(v[on], vb[sd][on]), name                  # the others equal their source
    assert torch.equal(env.get_state()[on], bank_env.get_state()[sd][on])
    assert torch.equal(env.obs[on], bank_env.obs[sd][on]) and torch.equal(env.obs[~on], pre.view("obs")[~on])
    # and they continue like their source
    nz = noises(bank_env, 1)[0]
    bank_env.step(ab[K], nz)
    env.step(ab[K][sd], None if nz is None else nz[sd])
    assert torch.equal(env.obs[on], bank_env.obs[sd][on]) and torch.equal(env.rwd[on], bank_env.rwd[sd][on])


# ---- 4. inside a captured graph -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [("rayleigh", "f32"), ("burgers500", "f32"), ("lorenz", "f32")])
def test_restore_and_steps_in_a_graph(case, dtype):
    _need_gpu()
    env = make(case, dtype)
    B = env.batch
    env.reset()
    acts = actions(env, K + 3, 41)
    run(env, acts[:K], [None] * K)
    snap = env.snapshot()
    g = torch.Generator().manual_seed(9)
    perm = [torch.randperm(B, generator=g).to(torch.int32).to(DEV) for _ in range(2)]
    static_src, static_act = perm[0].clone(), acts[K:].clone()

    def eager(src):
        env.restore(snap, src=src)
        for k in range(3):
            env._step(static_act[k], None)
        return outputs(env)[:5] + [env.get_state()]

    want = [eager(p) for p in perm]
    assert not all(torch.equal(x, y) for x, y in zip(*want))
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        env.restore(snap, src=static_src)
        for k in range(3):
            env._step(static_act[k], None)
    got = []
    for _ in range(2):
        graph.replay()
        got.append(outputs(env)[:5] + [env.get_state()])
    for r in got:
        assert all(torch.equal(x, y) for x, y in zip(r, want[0]))
    static_src.copy_(perm[1])                                         # the graph reads the index vector at every replay
    graph.replay()
    assert all(torch.equal(x, y) for x, y in zip(outputs(env)[:5] + [env.get_state()], want[1]))


# ---- 5. views and the file round trip -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [("rayleigh", "f32"), ("mixing", "f32"), ("burgers497", "f64"), ("shkadov", "f64"),
                                        ("sloshing", "f32"), ("lorenz", "f64"), ("vortex", "f32")])
def test_views_and_file_round_trip(case, dtype, tmp_path):
    _need_gpu()
    env = make(case, dtype)
    env.reset()
    acts = actions(env, K + M, 51)
    run(env, acts[:K], [None] * K)
    snap = env.snapshot()
    state, fields = env.get_state(), snap.view("fields")
    if case in ("lorenz", "vortex"):                                  # [n_real, B] columns; lorenz keeps its action index apart
        assert torch.equal(fields.t(), state[:, :fields.shape[0]])
        if case == "lorenz":
            assert torch.equal(snap.view("iu").to(state.dtype), state[:, 7])
    else:
        assert fields.shape == (state.shape[1], env.batch) + tuple(state.shape[2:])
        assert torch.equal(fields.transpose(0, 1), state)
    assert torch.equal(snap.view("stp").cpu(), stp_of(env)) and int(snap.view("stp")[0]) == K
    assert torch.equal(snap.view("obs"), env.obs) and torch.equal(snap.view("rwd"), env.rwd)
    assert torch.equal(snap.view("done"), env.done) and torch.equal(snap.view("status"), env.status)
    with pytest.raises(KeyError):
        snap.view("no_such_segment")
    ptr = snap.buf.data_ptr()
    assert env.snapshot(out=snap) is snap and snap.buf.data_ptr() == ptr
    rec0 = run(env, acts[K:], [None] * M)
    snap.save(tmp_path / "s.pt")
    loaded = beacon_amd.Snapshot.load(tmp_path / "s.pt", device=DEV)
    assert loaded.meta["ctor"] == snap.meta["ctor"] and torch.equal(loaded.buf, snap.buf)
    fresh = make(case, dtype)
    fresh.restore(loaded)
    assert same(rec0, run(fresh, acts[K:], [None] * M))
    assert env.snapshot(out=snap) is snap and snap.buf.data_ptr() == ptr


# ---- 6. both bindings ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rayleigh", "mixing", "burgers497", "shkadov", "sloshing", "lorenz", "vortex"])
def test_both_bindings_give_the_same_bytes(case):
    _need_gpu()
    env = make(case, "f32")
    env.reset()
    run(env, actions(env, K, 61), [None] * K)
    assert env.use_torch_ops(True)
    s_ops = env.snapshot()
    assert not env.use_torch_ops(False)
    s_ct = env.snapshot()
    assert torch.equal(s_ops.buf, s_ct.buf)
    run(env, actions(env, 1, 62), [None])
    env.restore(s_ops)                                                # through ctypes
    assert torch.equal(env.snapshot().buf, s_ops.buf)
    env.use_torch_ops(True)
    run(env, actions(env, 1, 62), [None])
    env.restore(s_ct, src=torch.arange(env.batch, dtype=torch.int32, device=DEV))   # through the op
    assert torch.equal(env.snapshot().buf, s_ops.buf)


def test_double_buffer_restore_writes_the_current_buffer():
    _need_gpu()
    env = make("burgers500", "f32")
    env.reset()
    env.double_buffer(True)
    run(env, actions(env, K, 71), [None] * K)
    snap = env.snapshot()
    at_k = outputs(env)
    run(env, actions(env, 1, 72), [None])
    cur = env.out_buf.data_ptr()
    env.restore(snap)
    assert env.out_buf.data_ptr() == cur
    assert all(torch.equal(x, y) for x, y in zip(outputs(env), at_k))
