"""Host tests (no GPU) of what DESIGN.md section 15 states once: the launch sequence of a step (VecEnv._enqueue_step behind
step(), step_autoreset() and capture()), the mask frame (VecEnv._masked), and the base class of the device bookkeeping buffers
(vec._SegBuffer: EpisodeStats, JetStats, Normalizer)."""
import pytest
import torch

from beacon_amd import _lib, vec

S, J, T, R, RR, N = "shkadov_step", "shkadov_jet_rewards", "episode_track", "shkadov_reset", "shkadov_reset_random", "normalize"


class _Lib(object):
    """libbeacon_hip of an env without a handle: bcn_set_mask (the one function _reset_finished calls itself) succeeds."""

    @staticmethod
    def bcn_set_mask(h, ptr):
        return 0


def _env(jets, norm, rand_init=False):
    """A VecShkadov without a handle and without a device, whose _call and _apply_mask record instead of launching.  A record is
    (entry point, mask it receives[, kind, with episode buffer -- normalize only]); the mask is the argument of the entry points
    that take one (episode_track, normalize) and the mask in force in the library for the others, spelled None / "mask" (the
    caller's) / "finished" (the episode buffer's)."""
    env = vec.VecShkadov.__new__(vec.VecShkadov)
    env.h, env.lib, env._mask, env._rotate = None, _Lib(), None, 0
    env.batch, env.n_jets, env.ndt_act, env._init_dev = 4, 2, 5, None
    env._n_rand = env.n_rand = torch.zeros(4, dtype=torch.int32)
    env.out_buf = torch.zeros(16, dtype=torch.uint8)
    env.obs, env.rwd, env.done, env.trunc, env.status = (torch.zeros(4) for _ in range(5))
    ep = vec.EpisodeStats.__new__(vec.EpisodeStats)
    ep.buf, ep.finished = torch.zeros(16, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    env._episodes = ep
    env._jets = vec.JetStats.__new__(vec.JetStats)
    env._jets.buf = torch.zeros(16, dtype=torch.uint8)
    env._jets_on, env._jets_stats = jets, 1
    nz = env._norm = vec.Normalizer.__new__(vec.Normalizer)
    nz.buf, nz.norm_obs, nz.norm_rwd = torch.zeros(16, dtype=torch.uint8), torch.zeros(4), torch.zeros(4)
    nz.training, nz.gamma, nz.eps, nz.clip_obs, nz.clip_rwd = True, 0.99, 1e-8, 10.0, 10.0
    env._norm_on = norm
    if rand_init:
        env.set_random_init(3)
    env.user_mask = torch.ones(4, dtype=torch.uint8)
    env.log = []

    def label(m):
        return None if m is None else "mask" if m is env.user_mask else "finished" if m is ep.finished else "unknown"

    def call(name, *args):
        if name == T:
            assert args[0] is env.out_buf and args[1] is ep.buf
            env.log.append((name, label(args[2])))
        elif name == N:
            assert args[0] is env.out_buf and args[1] is nz.buf and args[2] in (None, ep.buf)
            assert args[5:] == (1, 0.99, 1e-8, 10.0, 10.0)
            env.log.append((name, label(args[3]), args[4], args[2] is not None))
        else:
            env.log.append((name, label(env._mask)))

    def apply_mask(mask):
        env._mask = mask

    env._call, env._apply_mask = call, apply_mask
    return env


# What the commit before _enqueue_step launched, read off its four written-out copies.  "M" stands for the mask the call was
# given, None or the caller's: every entry holds for both.
STEP = {
    (False, False): [(S, "M")],
    (True, False): [(S, "M"), (J, "M")],
    (False, True): [(S, "M"), (N, "M", 0, False)],
    (True, True): [(S, "M"), (J, "M"), (N, "M", 0, False)],
}
STEP_AUTORESET = {
    (False, False): [(S, "M"), (T, "M"), (R, "finished")],
    (True, False): [(S, "M"), (J, "M"), (T, "M"), (R, "finished")],
    (False, True): [(S, "M"), (T, "M"), (R, "finished"), (N, "M", 0, True)],
    (True, True): [(S, "M"), (J, "M"), (T, "M"), (R, "finished"), (N, "M", 0, True)],
}
RESET_NORMALIZE = [(R, "M"), (N, "M", 1, False)]


def _given(seq, m):
    return [tuple(m if x == "M" else x for x in rec) for rec in seq]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("jets,norm", sorted(STEP))
def test_step_enqueues_the_parents_sequence(jets, norm, masked):
    env = _env(jets, norm)
    out = env.step(None, None, env.user_mask if masked else None)
    assert env.log == _given(STEP[jets, norm], "mask" if masked else None)
    assert env._mask is None                                          # the frame cleared what it set
    assert out[0] is (env._norm.norm_obs if norm else env.obs) and out[1] is (env._norm.norm_rwd if norm else env.rwd)
    assert out[2] is env.done and out[3] is env.trunc and out[4] is None


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("jets,norm", sorted(STEP_AUTORESET))
def test_step_autoreset_enqueues_the_parents_sequence(jets, norm, masked):
    env = _env(jets, norm)
    out = env.step_autoreset(None, None, env.user_mask if masked else None)
    assert env.log == _given(STEP_AUTORESET[jets, norm], "mask" if masked else None)
    assert env._mask is None                                          # ... and what _reset_finished left
    assert out[0] is (env._norm.norm_obs if norm else env.obs) and out[1] is (env._norm.norm_rwd if norm else env.rwd)
    assert out[2] is env.done and out[3] is env.trunc and out[4] is env.episodes


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("jets,norm", sorted(STEP_AUTORESET))
def test_step_autoreset_with_random_init_resets_through_the_fused_kernel(jets, norm, masked):
    env = _env(jets, norm, rand_init=True)
    env.step_autoreset(None, None, env.user_mask if masked else None)
    want = [(RR, m) if name == R else (name, m) + tuple(rest) for name, m, *rest in STEP_AUTORESET[jets, norm]]
    assert env.log == _given(want, "mask" if masked else None) and env._mask is None


@pytest.mark.parametrize("masked", [False, True])
def test_reset_with_normalize(masked):
    env = _env(True, True)                                            # (a reset launches nothing for the jets)
    out = env.reset(env.user_mask if masked else None)
    assert env.log == _given(RESET_NORMALIZE, "mask" if masked else None) and env._mask is None
    assert out[0] is env._norm.norm_obs and out[1] is None


def test_the_mask_is_cleared_when_a_launch_raises():
    env = _env(False, False)

    def boom(name, *args):
        raise _lib.BeaconHipError("launch failed")

    env._call = boom
    for fn in (env.step, env.step_autoreset):
        with pytest.raises(_lib.BeaconHipError):
            fn(None, None, env.user_mask)
        assert env._mask is None
    with pytest.raises(_lib.BeaconHipError):
        env.reset(env.user_mask)
    assert env._mask is None


# ---- the base class of the bookkeeping buffers ------------------------------------------------------------------------------
def _layout(rows, n, esz):
    """A hand-made layout list: rows of (name, elem, planes, row_elems) one behind the other by the 16-byte rule of
    include/beacon_hip.h.  Returns (layout, bytes)."""
    el = {_lib.SNAP_REAL: esz, _lib.SNAP_U8: 1, _lib.SNAP_I32: 4, _lib.SNAP_U32: 4, _lib.SNAP_F64: 8, _lib.SNAP_I64: 8}
    off, lay = 0, []
    for name, elem, planes, row in rows:
        lay.append(dict(name=name, offset=off, elem=elem, planes=planes, row_elems=row))
        off = (off + (planes * n if planes else 1) * row * el[elem] + 15) // 16 * 16
    return lay, off


def _buffer(cls, rows, n, tdtype=torch.float32, **attrs):
    b = cls.__new__(cls)
    lay, nbytes = _layout(rows, n, torch.empty((), dtype=tdtype).element_size())
    b.batch, b.tdtype, b.buf = n, tdtype, torch.zeros(nbytes, dtype=torch.uint8)
    for k, v in attrs.items():
        setattr(b, k, v)
    b._bind(lay)
    return b


def _episode(n, obs_dim, tdtype=torch.float32):
    RL, I32, F64, I64, U8 = _lib.SNAP_REAL, _lib.SNAP_I32, _lib.SNAP_F64, _lib.SNAP_I64, _lib.SNAP_U8
    rows = [("ret", RL, 1, 1), ("len", I32, 1, 1), ("last_ret", RL, 1, 1), ("last_len", I32, 1, 1), ("count", I32, 1, 1),
            ("sum_ret", F64, 1, 1), ("sum_len", I64, 1, 1), ("finished", U8, 1, 1), ("final_obs", RL, 1, obs_dim)]
    return _buffer(vec.EpisodeStats, rows, n, tdtype, obs_dim=obs_dim)


def _jets(n, n_jets, tdtype=torch.float32):
    rows = [(name, _lib.SNAP_F64 if name == "sum_ret" else _lib.SNAP_REAL, 1, n_jets) for name in vec.JetStats.NAMES]
    return _buffer(vec.JetStats, rows, n, tdtype, n_jets=n_jets)


def _normalizer(n, obs_dim, tdtype=torch.float32):
    RL, F64 = _lib.SNAP_REAL, _lib.SNAP_F64
    rows = [("obs_mean", F64, 0, obs_dim), ("obs_var", F64, 0, obs_dim), ("obs_count", F64, 0, 1), ("ret_mean", F64, 0, 1),
            ("ret_var", F64, 0, 1), ("ret_count", F64, 0, 1), ("ret", F64, 1, 1), ("norm_obs", RL, 1, obs_dim),
            ("norm_rwd", RL, 1, 1), ("norm_final_obs", RL, 1, obs_dim), ("scratch", _lib.SNAP_U8, 0, 40)]
    return _buffer(vec.Normalizer, rows, n, tdtype, obs_dim=obs_dim, gamma=0.9, eps=1e-6, clip_obs=5.0, clip_rwd=4.0, training=True)


@pytest.mark.parametrize("tdtype", [torch.float32, torch.float64])
def test_view_shapes_follow_each_class_rule(tdtype):
    B = 3
    for obs_dim in (1, 5):
        ep = _episode(B, obs_dim, tdtype)
        for name in ep.NAMES[:-1]:
            assert tuple(getattr(ep, name).shape) == (B,), name
        assert tuple(ep.final_obs.shape) == (B, obs_dim)                # 2-D whatever obs_dim is
        assert (ep.ret.dtype, ep.len.dtype, ep.sum_ret.dtype, ep.sum_len.dtype, ep.finished.dtype) == \
            (tdtype, torch.int32, torch.float64, torch.int64, torch.uint8)
        nz = _normalizer(B, obs_dim, tdtype)
        assert tuple(nz.obs_mean.shape) == tuple(nz.obs_var.shape) == (obs_dim,)        # planes = 0: flat [row_elems]
        for name in ("obs_count", "ret_mean", "ret_var", "ret_count"):
            assert tuple(getattr(nz, name).shape) == (1,) and getattr(nz, name).dtype == torch.float64
        assert tuple(nz.ret.shape) == tuple(nz.norm_rwd.shape) == (B,)
        want = (B, obs_dim) if obs_dim > 1 else (B,)                    # per-replica segments: 2-D only when row_elems > 1
        assert tuple(nz.norm_obs.shape) == tuple(nz.norm_final_obs.shape) == want and nz.norm_obs.dtype == tdtype
        assert tuple(nz.scratch.shape) == (40,) and nz.scratch.dtype == torch.uint8
    for n_jets in (1, 4):
        js = _jets(B, n_jets, tdtype)
        for name in js.NAMES:
            assert tuple(getattr(js, name).shape) == (B, n_jets), name   # [B, n_jets] even for one jet
        assert js.sum_ret.dtype == torch.float64 and js.rwd_jets.dtype == tdtype
    for b in (_episode(B, 5, tdtype), _jets(B, 4, tdtype), _normalizer(B, 5, tdtype)):
        # no copies, no overlap: writing a distinct value through every view is seen through every view, and in buf
        for k, name in enumerate(b.NAMES):
            getattr(b, name).fill_(k + 1)
        for k, name in enumerate(b.NAMES):
            v = b.view(name)
            assert v.data_ptr() == getattr(b, name).data_ptr() and bool((v == k + 1).all()), name
        with pytest.raises(KeyError):
            b.view("nope")


def test_snapshot_view_keeps_its_own_name_list():
    RL, I32, U8 = _lib.SNAP_REAL, _lib.SNAP_I32, _lib.SNAP_U8
    rows = [("fields", RL, 4, 6), ("obs_hist", RL, 1, 1), ("a_last", RL, 1, 1), ("a_prev", RL, 1, 2), ("stp", I32, 1, 1),
            ("obs", RL, 1, 1), ("rwd", RL, 1, 1), ("status", I32, 1, 1), ("done", U8, 1, 1)]
    lay, nbytes = _layout(rows, 3, 4)
    snap = vec.Snapshot(torch.zeros(nbytes, dtype=torch.uint8), dict(batch=3, dtype="f32", layout=lay, field_shape=[2, 3]))
    assert tuple(snap.view("fields").shape) == (4, 3, 2, 3)
    for name, shape in (("obs_hist", (3, 1)), ("a_last", (3, 1)), ("a_prev", (3, 2)), ("obs", (3, 1)), ("stp", (3,)), ("rwd", (3,)),
                        ("status", (3,)), ("done", (3,))):
        assert tuple(snap.view(name).shape) == shape, name
    snap.meta["field_shape"] = []                                        # the ODE envs: planes columns of one element
    snap.meta["layout"], _ = _layout([("fields", RL, 3, 1)], 3, 4)
    assert tuple(snap.view("fields").shape) == (3, 3)


def test_clear_mask_zeroes_only_the_selected_rows():
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8)
    for b in (_episode(3, 5), _episode(3, 1), _jets(3, 4), _jets(3, 1)):
        for name in b.NAMES:
            getattr(b, name).fill_(7)
        assert b.clear(mask) is b
        for name in b.NAMES:
            v = getattr(b, name)
            assert not v[0].any() and not v[2].any() and bool((v[1] == 7).all()), (type(b).__name__, name)   # 1-D and 2-D views
        assert b.clear() is b and not b.buf.any()
    nz = _normalizer(3, 5)
    nz.norm_obs.fill_(7)
    nz.obs_mean.fill_(7)
    assert nz.clear() is nz                                              # its own: variances back to 1, the rest 0
    assert bool((nz.obs_var == 1).all()) and bool((nz.ret_var == 1).all()) and not nz.obs_mean.any() and not nz.norm_obs.any()
    with pytest.raises(TypeError):
        nz.clear(mask)


@pytest.mark.parametrize("make,key,noun", [(_episode, "obs_dim", "observations"), (_jets, "n_jets", "jets"),
                                           (_normalizer, "obs_dim", "observations")])
def test_load_state_dict_refuses_each_mismatching_key(make, key, noun):
    b = make(3, 5)
    for name in b.NAMES:
        getattr(b, name).fill_(3)
    good = b.state_dict()
    assert set(good) >= {"buf", "batch", key, "dtype"} and (good["batch"], good[key], good["dtype"]) == (3, 5, "f32")
    if isinstance(b, vec.Normalizer):
        assert set(good) == {"buf", "batch", key, "dtype", "gamma", "eps", "clip_obs", "clip_rwd"}
    else:
        assert set(good) == {"buf", "batch", key, "dtype"}
    other = make(3, 5)
    assert other.load_state_dict(good) is other and torch.equal(other.buf, b.buf)
    name = type(b).__name__
    for bad, said in ((dict(good, batch=4), "4 replicas x 5"), (dict(good, **{key: 6}), "3 replicas x 6"),
                      (dict(good, dtype="f64"), r"3 replicas x 5 %s \(f64\)" % noun),
                      (dict(good, buf=torch.zeros(good["buf"].numel() + 16, dtype=torch.uint8)), "3 replicas x 5")):
        with pytest.raises(ValueError, match=r"%s.load_state_dict: statistics of %s" % (name, said)) as e:
            other.load_state_dict(bad)
        assert str(e.value).endswith("replicas x %s %s (%s), this env has 3 x 5" % (bad[key], noun, bad["dtype"]))
