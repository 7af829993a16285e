"""Per-jet rewards and returns of the multi-agent shkadov on the GPU: VecShkadov.set_jet_rewards / rwd_jets / jet_episodes /
obs_jets (csrc/shkadov_jets.hip, include/beacon_hip.h: bcn_shkadov_jet_rewards) and the single-env mirror envs.shkadov_separable
that reads them.  Yardsticks: the fixture captured from the reference's shkadov_separable (tests/golden/shkadov_separable.npz),
the reference's formula (shkadov.py:474-479) evaluated in NumPy float64 on the env's own state, and plain torch bookkeeping.

The tolerance of the kernel against the NumPy formula is derived, not measured: every term (h - 1)^2 is non-negative, so the sum
has no cancellation, and there is at most one rounding per square, one per addition and one each for `* dx` and the division:
|rwd_jets - ref| <= (l_rwd + 3) u |ref|, u = 2^-53 (float64) or 2^-24 (float32).  The sum over the jets against the scalar reward
of the step kernel: (n_jets l_rwd + 3) u |rwd| by the same count."""
import numpy as np
import pytest
import torch

from beacon_amd import _lib
from beacon_amd import envs as E
from beacon_amd import vec as V
from beacon_amd.envs import packaged_init
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3                        # B * n_jets is no multiple of the four (replica, jet) pairs of a workgroup in any shape below
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}

# the smallest geometries at which the wavefront-per-pair mapping can go wrong (cells: dx = 0.2, l_rwd = 50)
SHAPES = {
    "default": dict(n_jets=5),                                           # nx = 1100, jet_space = l_rwd = 50 cells: the zones abut
    "one_jet": dict(n_jets=1),
    "twenty": dict(n_jets=20),                                           # 60 pairs: 15 workgroups
    "overlap": dict(L0=30.0, jet_pos=30.0, jet_space=7.3, n_jets=4),     # jet_space = 36 cells < l_rwd: the zones overlap
    "gaps": dict(L0=30.0, jet_pos=30.0, jet_space=25.0, n_jets=3),       # jet_space = 125 cells: gaps between the zones
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")


def make(shape, dtype, **kw):
    cfg = dict(SHAPES[shape])
    cfg.update(kw)
    return V.VecShkadov(B, DEV, dtype, init_fields=packaged_init("shkadov"), **cfg)


def inputs(env, n, seed):
    """n steps of distinct random actions per replica [n, B, n_jets] and explicit inlet noise [n, B, ndt_act], on the device"""
    g = torch.Generator().manual_seed(seed)
    a = 2.0 * torch.rand((n, env.batch, env.n_jets), generator=g, dtype=torch.float64) - 1.0
    z = (2.0 * torch.rand((n, env.batch, env.ndt_act), generator=g, dtype=torch.float64) - 1.0) * env.sigma
    return a.to(device=DEV, dtype=env.tdtype), z.to(device=DEV, dtype=env.tdtype)


def formula(env, state=None):
    """shkadov.py:474-479 in NumPy float64 on the env's own film: [B, n_jets]"""
    h = (env.get_state() if state is None else state)[:, 0].double().cpu().numpy()
    out = np.zeros((env.batch, env.n_jets))
    with np.errstate(all="ignore"):                                       # (a blown-up replica's row is not looked at)
        for j in range(env.n_jets):
            s = env.jet_pos + j * env.jet_space
            assert s + env.l_rwd <= env.nx
            out[:, j] = -(np.sum(np.square(h[:, s:s + env.l_rwd] - 1.0), axis=1) * env.dx) / (env.n_jets * env.l_rwd)
    return out


def assert_within_bound(env, dtype, rows=None, what=""):
    got = env.rwd_jets.double().cpu().numpy()
    ref = formula(env)
    rows = range(env.batch) if rows is None else rows
    for b in rows:
        err, bound = np.abs(got[b] - ref[b]), (env.l_rwd + 3) * U[dtype] * np.abs(ref[b])
        print("%s %s replica %d: max err / bound = %.3g" % (what, dtype, b, float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(err <= bound), (what, dtype, b, err, bound)
        assert np.all(ref[b] < 0.0)                                       # a developed film: no zone is trivially zero


# ---- 1. against the reference ----------------------------------------------------------------------------------------------------
def test_rwd_jets_and_obs_jets_match_the_reference_fixture():
    _need_gpu()
    g = golden("shkadov_separable")
    env = V.VecShkadov(B, DEV, "f64", init_fields=packaged_init("shkadov"), n_jets=5).set_jet_rewards()
    env.reset()
    for r in range(3):
        a = np.broadcast_to(g["actions"][r], (B, 5)).copy()
        z = np.broadcast_to(g["noise"][r], (B, env.ndt_act)).copy()
        env.step(a, z)
        assert env.rwd_jets.shape == (B, 5) and env.obs_jets.shape == (B, 5, 10)
        assert env.obs_jets.data_ptr() == env.obs.data_ptr()                                  # a view, not a copy
        rj, oj = env.rwd_jets.cpu().numpy(), env.obs_jets.cpu().numpy()
        for b in range(B):
            for j in range(5):
                assert abs(rj[b, j] - g["rwd"][5 * r + j]) <= 1e-13, (r, b, j)
                assert np.max(np.abs(oj[b, j] - g["obs"][5 * r + j])) <= 1e-12, (r, b, j)
    env.close()


# ---- 2. the kernel alone, 3. consistency with the scalar reward, 4. run to run ---------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_matches_the_formula_on_the_envs_own_state(shape, dtype):
    _need_gpu()
    env = make(shape, dtype).set_jet_rewards(True, stats=False)
    cells = {"default": (1100, 50), "one_jet": (900, 50), "twenty": (1850, 50), "overlap": (369, 36), "gaps": (775, 125)}[shape]
    assert (env.nx, env.jet_space) == cells and env.l_rwd == 50
    a, z = inputs(env, 2, 5)
    env.reset()
    for k in range(2):
        env.step(a[k], z[k])
    assert int(env.status.max()) == 0
    assert_within_bound(env, dtype, what=shape)
    if shape in ("default", "twenty"):                                                        # 3: the rows sum to the step's reward
        tot, rwd = env.rwd_jets.double().sum(1).cpu().numpy(), env.rwd.double().cpu().numpy()
        bound = (env.n_jets * env.l_rwd + 3) * U[dtype] * np.abs(rwd)
        print("%s %s sum over jets vs rwd: max err / bound = %.3g" % (shape, dtype, float(np.max(np.abs(tot - rwd) / bound))))
        assert np.all(np.abs(tot - rwd) <= bound), (tot, rwd, bound)
    # 4: the same state evaluated again gives the same bits
    first = env.rwd_jets.clone()
    env._jets.buf.zero_()
    env._after_step()
    assert torch.equal(env.rwd_jets, first) and not torch.equal(first, torch.zeros_like(first))
    env.close()


# ---- 5. blow-up ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_blown_up_replica_gets_blowup_rwd_in_every_jet(dtype):
    _need_gpu()
    env = make("default", dtype).set_jet_rewards()
    a, z = inputs(env, 1, 9)
    env.reset()
    st = env.get_state()
    st[1, 0, 300] = 30.0                                                                      # beyond 5 h_max = 25 (shkadov.py:176)
    env.set_state(st)
    env.step(a[0], z[0])
    status = env.status.cpu().numpy()
    assert status[1] & _lib.ST_BLOWUP and not status[0] & _lib.ST_BLOWUP and not status[2] & _lib.ST_BLOWUP
    assert torch.equal(env.rwd_jets[1], torch.full((5,), -1.0, dtype=env.tdtype, device=DEV))
    assert float(env.rwd[1]) == -1.0 and bool(env.done[1]) and not bool(env.trunc[1])
    assert_within_bound(env, dtype, rows=(0, 2), what="blow-up")
    # the blown-up episode ended: its per-jet return moved on
    je = env.jet_episodes
    assert torch.equal(je.last_ret[1], env.rwd_jets[1]) and float(je.ret[1].abs().max()) == 0.0
    assert torch.equal(je.ret[0], env.rwd_jets[0]) and float(je.last_ret[0].abs().max()) == 0.0
    env.close()


# ---- 6. mask ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_masked_replica_keeps_its_rows_bit_for_bit(dtype):
    _need_gpu()
    env = make("default", dtype).set_jet_rewards()
    a, z = inputs(env, 1, 11)
    env.reset()
    je = env.jet_episodes
    sentinel = -7.25
    for name in V.JetStats.NAMES:
        getattr(je, name).fill_(sentinel)
    before = je.buf.clone()
    env.step(a[0], z[0], mask=torch.as_tensor(np.array([1, 0, 1], dtype=np.uint8)))
    for name in V.JetStats.NAMES:
        v = getattr(je, name)
        assert torch.equal(v[1], torch.full_like(v[1], sentinel)), name
    assert_within_bound(env, dtype, rows=(0, 2), what="mask")
    for b in (0, 2):
        assert torch.equal(je.ret[b], torch.full_like(je.ret[b], sentinel) + je.rwd_jets[b])
        assert torch.equal(je.last_ret[b], torch.full_like(je.last_ret[b], sentinel))        # no episode ended
    assert not torch.equal(before, je.buf)
    # an explicit clear(mask) zeroes the selected replicas alone
    je.clear(np.array([0, 1, 0]))
    assert float(je.ret[1].abs().max()) == 0.0 and torch.equal(je.last_ret[0], torch.full_like(je.last_ret[0], sentinel))
    env.close()


# ---- 7. statistics across episode ends -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rand_init", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_per_jet_returns_follow_a_host_accumulation_across_episode_ends(dtype, rand_init):
    _need_gpu()
    env = make("default", dtype, t_act=0.15).set_jet_rewards()
    assert env.n_act == 2                                                                     # int(0.15 / 0.05): episodes of two steps
    if rand_init:
        env.set_random_init(5)
    a, _ = inputs(env, 7, 13)
    env.reset()
    env.set_stp(np.array([0, 1, 0]))                                                          # the replicas end at different steps
    ret = torch.zeros((B, 5), dtype=env.tdtype, device=DEV)
    last, total = ret.clone(), torch.zeros((B, 5), dtype=torch.float64, device=DEV)
    ended = 0
    for k in range(7):
        _, _, done, trunc, info = env.step_autoreset(a[k])
        rj, fin = env.rwd_jets.clone(), ((done | trunc) != 0).clone()
        ended += int(fin.sum())
        ret = ret + rj
        last = torch.where(fin[:, None], ret, last)
        total = torch.where(fin[:, None], total + ret.double(), total)
        ret = torch.where(fin[:, None], torch.zeros_like(ret), ret)
        je = env.jet_episodes
        assert torch.equal(je.ret, ret) and torch.equal(je.last_ret, last), (dtype, rand_init, k)
        assert bool(((je.sum_ret - total).abs() <= 1e-15 * total.abs()).all()), (dtype, rand_init, k)
        assert torch.equal(info.finished != 0, fin)
    assert ended >= 2 * B and float(last.abs().min()) > 0.0                                   # every replica finished, twice
    if rand_init:
        assert int(env.n_rand.max()) <= 5
    # checkpointing the statistics
    d = env.jet_episodes.state_dict()
    env.jet_episodes.clear()
    assert float(env.jet_episodes.sum_ret.abs().max()) == 0.0
    env.jet_episodes.load_state_dict(d)
    assert torch.equal(env.jet_episodes.last_ret, last)
    env.close()


# ---- 8. graphs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_captured_rollout_carries_rwd_jets_and_returns(dtype):
    _need_gpu()
    n = 4
    G, T = make("default", dtype, t_act=0.15).set_jet_rewards(), make("default", dtype, t_act=0.15).set_jet_rewards()
    a, z = inputs(G, n, 17)
    for env in (G, T):
        env.reset()
        env.set_stp(np.array([0, 1, 0]))
    g = G.capture(a, z, n_steps=n, autoreset=True)
    assert g.rwd_jets_seq.shape == (n, B, 5)
    g.replay()
    torch.cuda.synchronize()
    for k in range(n):
        _, rwd, done, _, _ = T.step_autoreset(a[k], z[k])
        assert torch.equal(g.rwd_jets_seq[k], T.rwd_jets), (dtype, k)
        assert torch.equal(g.rwd_seq[k], rwd) and torch.equal(g.done_seq[k], done)
    assert int(g.done_seq.sum()) >= B
    for name in V.JetStats.NAMES:
        assert torch.equal(getattr(G.jet_episodes, name), getattr(T.jet_episodes, name)), name
    assert torch.equal(G.jet_episodes.buf, T.jet_episodes.buf) and torch.equal(G.get_state(), T.get_state())
    G.close(), T.close()


# ---- 9. off means off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_feature_changes_nothing_else(dtype):
    _need_gpu()
    on, off = make("default", dtype, t_act=0.15).set_jet_rewards(True), make("default", dtype, t_act=0.15)
    a, _ = inputs(on, 4, 19)
    for env in (on, off):
        env.reset()
    with pytest.raises(AttributeError, match="set_jet_rewards"):
        off.rwd_jets
    sig = off.snapshot_signature()
    for k in range(4):
        on.step_autoreset(a[k])
        off.step_autoreset(a[k])
    for name in ("obs", "rwd", "done", "trunc", "status"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    assert torch.equal(on.get_state(), off.get_state()) and torch.equal(on.episodes.buf, off.episodes.buf)
    assert int(on.episodes.count.sum()) == 2 * B                                              # episodes of two steps
    assert on.snapshot_signature() == sig and on.snapshot().buf.numel() == off.snapshot().buf.numel()
    assert off._jets is None                                                                  # nothing allocated
    on.set_jet_rewards(False)
    with pytest.raises(AttributeError, match="set_jet_rewards"):
        on.rwd_jets
    on.close(), off.close()


def test_double_buffered_outputs_are_the_ones_the_jets_launch_reads():
    """with double_buffer() the launch reads the buffer the step just wrote: a blow-up flag planted in the other one (the one that
    was current before the step) must not reach the jets"""
    _need_gpu()
    D, S = make("default", "f32").double_buffer().set_jet_rewards(), make("default", "f32").set_jet_rewards()
    a, z = inputs(D, 3, 23)
    for env in (D, S):
        env.reset()
    for k in range(3):
        old = D.out_buf
        D.status.fill_(_lib.ST_BLOWUP)                                    # the buffer this step does NOT write
        D.step(a[k], z[k])
        S.step(a[k], z[k])
        assert D.out_buf is not old and int(D.status.max()) == 0
        assert torch.equal(D.rwd_jets, S.rwd_jets) and torch.equal(D.jet_episodes.ret, S.jet_episodes.ret), k
    D.close(), S.close()


# ---- 10. the single-env mirror ---------------------------------------------------------------------------------------------------
def test_separable_mirror_reads_rwd_jets_and_downloads_no_state(monkeypatch):
    _need_gpu()
    g = golden("shkadov_separable")
    e = E.shkadov_separable(n_jets=5)
    e.rand_init = False
    for k in range(5):
        e.reset()
    np.random.seed(6)

    def no_download(*args, **kw):
        raise AssertionError("shkadov_separable.step downloaded the state")
    monkeypatch.setattr(e.vec, "get_state", no_download)
    for j in range(5):
        obs, rwd, done, trunc, _ = e.step(g["actions"][0].tolist())
        assert abs(rwd - g["rwd"][j]) <= 1e-14 and np.max(np.abs(obs - g["obs"][j])) <= 1e-12
        assert [done, trunc] == g["done"][j].tolist()
    monkeypatch.undo()
    e.close()
