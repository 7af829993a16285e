"""Every instantiation of the general 1D step kernels -- burgers_step_k, shkadov_step_k, sloshing_step_k x float64 / float32 x
K = 1, 2, 4, 8 cells per thread x NT = 64 .. 1024 threads (csrc/env1d_impl.inc: BCN_DISPATCH_1D / BCN_LAUNCH_NT) -- against the
float64 oracle, at the smallest grids at which that shape can go wrong ("The 1D shape matrix"):

  full    n = K NT            every thread full, cell n-1 the last cell of the last thread
  ragged  n = K NT - K + 1    the last live thread holds ONE cell, its first: the outflow copy / far wall reaches into the
                              neighbouring thread (K = 1: n = NT - 3)
  half    n = K NT / 2 + 1    (NT >= 128) the fewest cells that still select this NT: half the threads, whole waves, idle

The shape is forced with the options one_wave = 0 and cells_per_thread = K, and every case asserts env.kernel_shape == (K, NT):
the launcher overrides a request that does not fit, and a case that ran another instantiation would prove nothing.

float64: fields and observations are BIT-IDENTICAL to the oracle (the property test_env1d_float64_bit_identical_to_oracle asserts
at the default shapes), rewards -- reductions whose order depends on NT -- within 1e-12.  float32: the bounds the project
already measured against the oracle (tests/test_gpu_parity.py); no number is new here."""
import numpy as np
import pytest
import torch

from beacon_amd import vec as V
from oracle import oracle as O
from test_gpu_parity import shkadov_tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
ENVS = ("burgers", "shkadov", "sloshing")
KS = (1, 2, 4, 8)
NTS = (64, 128, 256, 512, 1024)

# A shkadov grid holds the observation window upstream of the first jet (l_obs = 49 cells) and the reward window downstream of
# the last one (l_rwd = 49 cells): bcn_shkadov_create refuses nx < 98 (jet_pos - l_obs >= 0, jet_pos + l_rwd <= nx), and a
# kernel that ran there would read outside its arrays.
SHK_MIN_N = 98
# Shapes that no valid constructor reaches: (env, K, NT) -> reason.  Both precisions.
EXCLUDED = {
    ("shkadov", 1, 64): "n <= 64 < %d cells: the 49-cell observation and reward windows do not fit the grid" % SHK_MIN_N,
}
# Grid lengths that no valid constructor reaches, of shapes that are otherwise covered: (env, K, NT, grid) -> (n used, reason)
SUBSTITUTED = {
    ("shkadov", 1, 128, "half"): (SHK_MIN_N, "n = 65 is below the smallest shkadov grid; %d is the fewest cells that select NT = 128" % SHK_MIN_N),
}

# float32 bounds, all from tests/test_gpu_parity.py: burgers -- test_burgers_nx512_vs_oracle_and_mirror (2e-4 on observations and
# reward, valid up to 1920 timesteps) and test_burgers_vs_golden / test_burgers_shkadov_fullsize_properties (1e-3 on fields);
# sloshing -- test_sloshing_vs_golden (5e-5); shkadov -- shkadov_tol, and the packed-against-scalar bounds of
# test_shkadov_packed_step_variants_match_the_scalar_step_and_the_oracle (5e-6 on h, q and observations, 5e-4 on the rhs arrays;
# q -- driven by random full-amplitude jets -- at 5 x shkadov_tol, the factor that test gives the observations, which are q)
BURGERS_F32 = dict(obs=2e-4, rwd=2e-4, fields=1e-3)
SLOSHING_F32 = 5e-5
SHK_PK_VS_SCALAR = dict(hq=5e-6, rhs=5e-4, obs=5e-6)
F64_RWD = 1e-12


def grids(name, K, NT):
    g = [("full", K * NT), ("ragged", K * NT - K + 1 if K > 1 else NT - 3)]
    if NT >= 128:
        g.append(("half", K * NT // 2 + 1))
    return [(tag, SUBSTITUTED.get((name, K, NT, tag), (n,))[0]) for tag, n in g]


def expected_shape(n, K):
    """The documented rule (include/beacon_hip.h: bcn_kernel_shape; env1d_impl.inc): with one_wave = 0 and cells_per_thread = K
    the launcher keeps K unless n > 1024 K (then doubles it until the grid fits) and takes the smallest NT of 64 .. 1024 with
    K NT >= n."""
    k = K
    while n > k * 1024:
        k *= 2
    return k, next(nt for nt in NTS if n <= k * nt)


def ctor_kwargs(name, n):
    """Constructor arguments that give a grid of exactly n cells (the +0.5 keeps int(80 L) / int(5 L) away from truncation)."""
    if name == "burgers":
        return dict(nx=n)
    if name == "sloshing":
        return dict(L=(n - 2 + 0.5) / 80.0)
    # shkadov: two jets 10 apart near the end of a long grid; one jet in the middle of a short one (jet_space 4 -> 19 cells: the
    # smallest that holds a jet of half-width 9), its position chosen in cells so that both 49-cell windows fit from n = 98 on
    if n >= 400:
        n_jets, js = 2, 10.0
        L0 = (n + 0.5) / 5.0 - js * (n_jets + 2)
        return dict(L0=L0, n_jets=n_jets, jet_space=js, jet_pos=L0)
    n_jets, js = 1, 4.0
    L0 = (n + 0.5) / 5.0 - js * (n_jets + 2)
    dx = (L0 + js * (n_jets + 2)) / n
    return dict(L0=L0, n_jets=n_jets, jet_space=js, jet_pos=(49 + (n - SHK_MIN_N) // 2 + 0.5) * dx)


PARAMS = {  # per-replica physics of the set_params case (replica 0: the constructor's defaults)
    "burgers": dict(u_target=[0.5, 0.4, 0.6], amp=[10.0, 5.0, 12.0]),
    "shkadov": dict(delta=[0.1, 0.08, 0.15]),
    "sloshing": dict(amp=[5.0, 3.0, 6.0], alpha=[5.0e-4, 1.0e-3, 2.0e-4], g=[9.81, 9.0, 10.5]),
}


def sloshing_init(n):
    """the smooth synthetic free surface of test_sloshing_other_lengths_vs_oracle_f64"""
    nx = n - 2
    x = (np.arange(nx + 2) - 0.5) / nx
    init = np.zeros((2, nx + 2))
    init[0] = 1.0 + 0.05 * np.cos(np.pi * x)
    return init


def ripple(name, n):
    """A smooth non-uniform state [B, nfields, n], different per replica.  From reset a burgers / shkadov grid is FLAT wherever
    the inlet noise and the forcing have not arrived yet -- most of a long grid after two action steps -- and on a flat field a
    thread that reads the wrong halo cell reads the right value.  One more action step from this state makes every cell's
    neighbours differ (wavelength 256 cells or the whole grid, amplitude 2-3 %: far from a shock or a film wave)."""
    c = 2.0 * np.pi * max(1, n // 256) * np.arange(n) / n
    st = np.zeros((B, 3 if name == "burgers" else 4, n))
    for b in range(B):
        if name == "burgers":
            st[b, :3] = 0.5 + 0.02 * np.sin(c + b)
        else:
            st[b, 0] = 1.0 + 0.02 * np.cos(c + b)
            st[b, 1] = 1.0 + 0.03 * np.sin(c + 2.0 * b)
    return st


class _Ref(object):
    pass


_REFS = {}


def reference(name, n, variant="plain"):
    """The oracle's trajectory of the B replicas at this grid, computed once and shared by every shape and precision that runs it
    (many (K, NT) pairs meet at the same n).  variant: "plain" -- two action steps from the env's start (one for burgers beyond
    4096 cells: two would pass the 1920 timesteps the float32 bounds hold for), then for burgers / shkadov one step from
    ripple(); "mask" -- two steps, replica 1 switched off in the second; "params" -- two steps with PARAMS."""
    key = (name, n, variant)
    if key in _REFS:
        return _REFS[key]
    r = _Ref()
    r.name, r.n, r.variant, r.kw = name, n, variant, ctor_kwargs(name, n)
    rng = np.random.default_rng([ENVS.index(name), n, ("plain", "mask", "params").index(variant)])
    r.init = sloshing_init(n) if name == "sloshing" else None
    pk = [{k: v[b] for k, v in PARAMS[name].items()} if variant == "params" else {} for b in range(B)]
    if name == "burgers":
        ors = [O.burgers(**r.kw, **pk[b]) for b in range(B)]
    elif name == "shkadov":
        ors = [O.shkadov(init_fields=np.ones((2, n)), **r.kw, **pk[b]) for b in range(B)]   # the flat film
        for o in ors:
            o.rand_init = False
    else:
        ors = [O.sloshing(init_fields=r.init, **r.kw, **pk[b]) for b in range(B)]
    assert all((o.nx if name != "sloshing" else o.nx + 2) == n for o in ors), (name, n, r.kw)
    for o in ors:
        o.reset()
    r.n_jets = ors[0].n_jets if name == "shkadov" else 0
    ndt = ors[0].cfg.ndt_act
    plan = ["step"] if (name == "burgers" and n > 4096) else ["step", "step"]
    if variant == "plain" and name != "sloshing":
        plan.append("ripple")
    r.steps = []
    for i, what in enumerate(plan):
        s = _Ref()
        s.state0 = ripple(name, n) if what == "ripple" else None
        s.k = 1 if what == "ripple" else i + 1                  # action steps since the state was last given: shkadov_tol(k)
        s.mask = np.array([1, 0, 1], np.uint8) if (variant == "mask" and i == 1) else None
        s.acts = rng.uniform(-1, 1, (B, r.n_jets) if name == "shkadov" else (B,))
        s.noise = {"burgers": rng.uniform(-0.1, 0.1, B), "shkadov": rng.uniform(-5e-4, 5e-4, (B, ndt)), "sloshing": None}[name]
        s.out = []
        for b, o in enumerate(ors):
            if s.state0 is not None:
                o.w[:s.state0.shape[1]] = s.state0[b]
                o.w[s.state0.shape[1]:] = 0.0
            if s.mask is not None and not s.mask[b]:
                s.out.append(None)
                continue
            if name == "burgers":
                res = o.step([s.acts[b]], s.noise[b])
            elif name == "shkadov":
                res = o.step(s.acts[b].tolist(), s.noise[b])
            else:
                res = o.step([s.acts[b]])
            nf = 3 if name == "burgers" else 2
            s.out.append(dict(fields=o.w[:nf].copy(), obs=np.array(res[0], np.float64), rwd=float(res[1]), done=bool(res[2]),
                              trunc=bool(res[3])))
            assert np.isfinite(o.w).all() and np.abs(o.w[:nf]).max() < 3.0, (name, n, i, b)   # the oracle itself is far from blow-up
        r.steps.append(s)
    _REFS[key] = r
    return r


def make_env(ref, dtype, K, one_wave):
    cls = {"burgers": V.VecBurgers, "shkadov": V.VecShkadov, "sloshing": V.VecSloshing}[ref.name]
    env = cls(B, DEV, dtype, **ref.kw) if ref.name == "burgers" else cls(B, DEV, dtype, ref.init, **ref.kw)
    assert (env.nx + 2 if ref.name == "sloshing" else env.nx) == ref.n, (ref.name, ref.n, ref.kw)
    env.set_option("one_wave", one_wave)
    env.set_option("cells_per_thread", K)
    if ref.variant == "params":
        env.set_params(**PARAMS[ref.name])
    env.reset()
    return env


def run(ref, dtype, K, NT, one_wave=0):
    """Step the device env through the reference's plan; returns per step (state [B, nf, n] float64, obs, rwd, done, trunc, status).
    Asserts the shape after the first step and that a masked replica keeps its state and output rows bit for bit."""
    env = make_env(ref, dtype, K, one_wave)
    recs = []
    for i, s in enumerate(ref.steps):
        if s.state0 is not None:
            env.set_state(s.state0)
        if s.mask is not None:
            off = torch.as_tensor(s.mask == 0, device=DEV)
            env.obs[off] = -777.25                               # a sentinel: a masked row that was rewritten with its own value would pass
            before = [x.clone() for x in (env.get_state(), env.obs, env.rwd, env.done, env.trunc, env.status)]
        env.step(s.acts, s.noise, mask=None if s.mask is None else torch.as_tensor(s.mask, device=DEV))
        torch.cuda.synchronize()
        if i == 0:
            assert expected_shape(ref.n, K) == (K, NT), "the grid does not select this shape: a mistake in the test"
            assert env.kernel_shape == (K, NT), (ref.name, dtype, ref.n, env.kernel_shape)
            assert env.kernel_name == ref.name + "_step_k"
        if s.mask is not None:
            after = (env.get_state(), env.obs, env.rwd, env.done, env.trunc, env.status)
            for x, y in zip(before, after):
                assert torch.equal(x[off], y[off]), "a masked replica changed"
        recs.append([x.double().cpu().numpy() for x in (env.get_state(), env.obs, env.rwd)] +
                    [x.cpu().numpy() for x in (env.done, env.trunc, env.status)])
    env.close()
    return recs


def dist(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def compare(ref, dtype, recs, tag, exact=True):
    """Device records against the oracle.  float64: bit-identical fields and observations (exact=False, the set_params case:
    1e-12, the bound of test_every_replica_of_a_mixed_batch_matches_the_float64_oracle_of_its_arguments), rewards within 1e-12.
    float32: the inherited bounds (top of the file).  Prints the worst figures before it asserts."""
    name, worst, fails = ref.name, {}, []

    def check(what, d, tol, where):
        worst[what] = max(worst.get(what, 0.0), d)
        if not d <= tol:
            fails.append((what, d, tol) + where)

    for i, (s, (st, obs, rwd, done, trunc, status)) in enumerate(zip(ref.steps, recs)):
        for b, want in enumerate(s.out):
            if want is None:
                continue
            w = (i, b)
            nf = want["fields"].shape[0]
            if dtype == "f64":
                if exact:
                    check("fields_differ", float(not np.array_equal(st[b, :nf], want["fields"])), 0.0, w)
                    check("obs_differ", float(not np.array_equal(obs[b], want["obs"])), 0.0, w)
                check("fields", dist(st[b, :nf], want["fields"]), 0.0 if exact else 1e-12, w)
                check("obs", dist(obs[b], want["obs"]), 0.0 if exact else 1e-12, w)
                check("rwd", dist(rwd[b], want["rwd"]), F64_RWD, w)
            elif name == "burgers":
                check("fields", dist(st[b, :nf], want["fields"]), BURGERS_F32["fields"], w)
                check("obs", dist(obs[b], want["obs"]), BURGERS_F32["obs"], w)
                check("rwd", dist(rwd[b], want["rwd"]), BURGERS_F32["rwd"], w)
            elif name == "shkadov":
                check("h", dist(st[b, 0], want["fields"][0]), shkadov_tol("f32", s.k), w)
                check("q", dist(st[b, 1], want["fields"][1]), 5 * shkadov_tol("f32", s.k), w)
                check("obs", dist(obs[b], want["obs"]), shkadov_tol("f32", s.k), w)
                check("rwd", dist(rwd[b], want["rwd"]), shkadov_tol("f32", s.k, reward=True), w)
            else:
                check("fields", dist(st[b, :nf], want["fields"]), SLOSHING_F32, w)
                check("obs", dist(obs[b], want["obs"]), SLOSHING_F32, w)
                check("rwd", dist(rwd[b], want["rwd"]), SLOSHING_F32, w)
            check("done", float(bool(done[b]) != want["done"] or bool(trunc[b]) != want["trunc"]), 0.0, w)
            check("status", float(abs(int(status[b]))), 0.0, w)
    print("MEASURED %s %s n=%d %s: max |device - oracle| %s" % (name, dtype, ref.n, tag, {k: "%.2e" % v for k, v in worst.items()}))
    assert not fails, (name, dtype, ref.n, tag, fails[:6])


CASES = [(name, dtype, K, NT) for name in ENVS for dtype in ("f64", "f32") for K in KS for NT in NTS if (name, K, NT) not in EXCLUDED]


def test_the_exclusion_list_is_as_short_as_the_constructors_allow():
    """118 of the 120 instantiations run; what is excluded is exactly what bcn_shkadov_create cannot build."""
    assert len(CASES) == 120 - 2 * len(EXCLUDED) and len(EXCLUDED) <= 1
    for (name, K, NT) in EXCLUDED:
        assert name == "shkadov" and K * NT < SHK_MIN_N
        with pytest.raises(Exception):
            L0 = (K * NT + 0.5) / 5.0 - 3.0                      # n = K NT with one jet and the smallest spacing
            V.VecShkadov(B, DEV, "f64", None, L0=L0, n_jets=1, jet_space=1.0, jet_pos=L0)
    for (name, K, NT, tag), (n, _) in SUBSTITUTED.items():
        assert name == "shkadov" and dict(grids("", K, NT))[tag] < SHK_MIN_N and expected_shape(n, K) == (K, NT)


@pytest.mark.parametrize("name,dtype,K,NT", CASES, ids=["%s-%s-K%d-NT%d" % c for c in CASES])
def test_shape_vs_oracle(name, dtype, K, NT):
    for tag, n in grids(name, K, NT):
        ref = reference(name, n)
        if name == "shkadov" and dtype == "f32":
            # one_wave = 1: the packed timestep where the shape has one (K = 4, two LDS buffers) and n % 4 == 0, else the scalar
            # one; one_wave = 2: the scalar timestep always.  Both against the oracle, and against each other.
            pk, sc = run(ref, dtype, K, NT, one_wave=1), run(ref, dtype, K, NT, one_wave=2)
            compare(ref, dtype, pk, "%s one_wave=1" % tag)
            compare(ref, dtype, sc, "%s one_wave=2" % tag)
            for i, (p, s) in enumerate(zip(pk, sc)):
                d = (dist(p[0][:, :2], s[0][:, :2]), dist(p[0][:, 2:], s[0][:, 2:]), dist(p[1], s[1]))
                print("MEASURED shkadov f32 n=%d %s step %d: max |packed - scalar| h,q %.2e rhs %.2e obs %.2e" % ((n, tag, i) + d))
                assert d[0] <= SHK_PK_VS_SCALAR["hq"] and d[1] <= SHK_PK_VS_SCALAR["rhs"] and d[2] <= SHK_PK_VS_SCALAR["obs"], (n, tag, i, d)
        else:
            compare(ref, dtype, run(ref, dtype, K, NT), tag)


# the entry code shared by all shapes -- *_params, the mask return -- off the default shape: one multi-wave shape, ragged grid
ENTRY_K, ENTRY_NT = 2, 256


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ENVS)
def test_masked_step_at_a_forced_shape(name, dtype):
    """Replica 1 is switched off in the second step: its state and its output rows (a sentinel in the observations) stay bitwise
    untouched -- asserted in run() -- and the others still equal the oracle."""
    n = dict(grids(name, ENTRY_K, ENTRY_NT))["ragged"]
    ref = reference(name, n, "mask")
    compare(ref, dtype, run(ref, dtype, ENTRY_K, ENTRY_NT), "masked")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ENVS)
def test_per_replica_parameters_at_a_forced_shape(name, dtype):
    """set_params: each replica against the oracle of ITS arguments."""
    n = dict(grids(name, ENTRY_K, ENTRY_NT))["ragged"]
    ref = reference(name, n, "params")
    compare(ref, dtype, run(ref, dtype, ENTRY_K, ENTRY_NT), "set_params", exact=False)
