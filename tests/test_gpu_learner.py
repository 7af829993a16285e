"""The on-device learner (beacon_amd.Learner, libbeacon_learner.so) against tests/learner_ref.py -- torch autograd, torch.optim.Adam and
clip_grad_norm_ in float64 on the CPU -- on the MI355X.

How errors are measured (as in tests/test_gpu_actor.py): for a quantity q -- a gradient segment, a statistic, a parameter or moment
segment -- err(q) = max |device - reference| / max(1, max |reference|).  The reference gets the device's inputs (the weights and the
rows as the device holds them, cast to float64), so the error is the kernels' arithmetic alone.

The data of every case is made on the CPU from fixed seeds, and the tests assert on the REFERENCE that it exercises what it should:
clip_frac in [0.2, 0.8] (both branches of the surrogate), no ratio within 1e-4 of 1 +- clip and no relu pre-activation within 1e-5 of
0 (the gradient is discontinuous there: a float32 flip is no arithmetic error).

float64: f64_tol(m) = (m + 640) x 2^-53 x 500, the summation-order bound: a gradient entry is the W-weighted mean of m per-row terms,
each a chain of dot products of at most 384 + 128 + 128 terms, so another order of the same sums moves it by at most (m + 640) u
max |term|; the terms (|adv| <= 4.5, ratio <= e^0.5, |z| <= 10, |activation| <= 4) stay below 500.  5.5e-11 for m = 257, 9.5e-10 for
m = 16 385.
float32: the project's rule -- every tolerance in F32_TOL is at most 10 x the worst error measured on the MI355X over the cases; both
numbers stand next to each other there."""
import functools

import numpy as np
import pytest
import torch

import learner_ref as R
from test_gpu_actor import _Env, _weights

pytestmark = pytest.mark.gpu

CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01
U64 = 2.0 ** -53


def f64_tol(m):
    return (m + 640) * U64 * 500.0


# float32: quantity -> (tolerance, worst error measured on the MI355X)
F32_TOL = {"grad": (2.0e-6, 2.087e-7), "stats": (2.3e-6, 2.360e-7),                             # test_gradient_and_stats_match_reference, over CASES
           "adam_params": (8.7e-7, 8.765e-8), "adam_m": (1.3e-7, 1.331e-8), "adam_v": (2.2e-10, 2.242e-11),   # test_adam_matches_torch
           "e2e_params": (2.7e-7, 2.734e-8)}                                                    # test_end_to_end_update

# (m rows, obs_dim, hidden, activation, kind, act_dim, selection): selection "idx" = 130 of the rows in permuted order and uint8 weights
# with about a third zeros.  65 / 257: a partial tile behind one / several full ones; 33 x (17, 128, 3): the two-pass width and partial
# output groups; 384: several K-slabs; 16 385 rows: 257 tiles in float32, 513 in float64 -- more than the fixed grid of 256, so a
# workgroup walks up to three tiles.
CASES = [(1, 1, (5,), "tanh", "gaussian", 1, None),
         (65, 33, (17, 128, 3), "relu", "gaussian", 5, None),
         (257, 384, (64, 64), "tanh", "gaussian", 10, None),
         (65, 6, (64, 64), "relu", "categorical", 4, None),
         (257, 6, (64, 64), "tanh", "categorical", 3, "idx"),
         (16385, 3, (4,), "tanh", "gaussian", 1, None)]
IDS = ["%dx%d-%s-%s-%s%d%s" % (c[0], c[1], "_".join(map(str, c[2])), c[3], c[4][:3], c[5], "-idx" if c[6] else "") for c in CASES]
# the data seed of each case, chosen on the CPU so that the assertions on the reference hold in both dtypes
SEEDS = dict(zip(IDS, [11, 12, 11, 13, 11, 11]))


def weights_dict(obs_dim, hidden, kind, n, dtype, wseed=1):
    """{segment name: CPU tensor of `dtype`}: what Actor.load leaves on the device for the same seed"""
    pi, vf, ls = _weights(obs_dim, hidden, n, 1.0, wseed)
    w = {}
    for net, layers in (("pi", pi), ("vf", vf)):
        for l, (W, b) in enumerate(layers):
            w["%s_w%d" % (net, l)], w["%s_b%d" % (net, l)] = torch.as_tensor(W).to(dtype), torch.as_tensor(b).to(dtype)
    w["log_std"] = torch.as_tensor(ls).to(dtype) if kind == "gaussian" else torch.zeros(0, dtype=dtype)
    return w


@functools.lru_cache(maxsize=None)
def case_data(case, dtype, seed):
    """The rows of a case (CPU tensors of `dtype`, the idx / weight selection included) and the reference's answer: made once per
    case and dtype, shared by the tests, never modified."""
    m, obs_dim, hidden, activation, kind, n, sel = case
    rng = np.random.default_rng(seed)
    w = weights_dict(obs_dim, hidden, kind, n, dtype)
    ref = R.Ref(w, hidden, activation, 0 if kind == "gaussian" else 1)
    t = lambda x: torch.as_tensor(x).to(dtype)
    obs = t(rng.uniform(-1.0, 1.0, (m, obs_dim)))
    act = t(rng.normal(0.0, 0.7, (m, n))) if kind == "gaussian" else torch.as_tensor(rng.integers(0, n, m)).to(torch.int32)
    adv, ret = t(rng.normal(size=m)), t(rng.normal(size=m))
    with torch.no_grad():
        logp = ref.terms(obs, act, torch.zeros(m), adv, ret, None, CLIP, VF_COEF, ENT_COEF)["logp"]
    pert = rng.uniform(-0.5, 0.5, m)
    near = np.abs(np.abs(np.exp(-pert) - 1.0) - CLIP) < 2e-3           # (16 385 uniform draws always put some ratio on a clip boundary)
    logp_old = t(logp.numpy() + np.where(near, pert + 0.01, pert))
    idx = weight = None
    if sel == "idx":
        idx = torch.as_tensor(rng.permutation(m)[:130].copy()).to(torch.int32)
        weight = torch.as_tensor(rng.uniform(size=m) > 1.0 / 3.0).to(torch.uint8)
    rows = idx.long() if idx is not None else slice(None)
    grads, stats, terms = ref.grad(obs[rows], act[rows], logp_old[rows], adv[rows], ret[rows], None if weight is None else weight[rows],
                                   CLIP, VF_COEF, ENT_COEF)
    pre = ref.preactivations(obs[rows]) if activation == "relu" else []
    margin = dict(ratio=float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()),
                  relu=min([float(p.abs().min()) for p in pre] or [1.0]))
    return dict(w=w, obs=obs, act=act, adv=adv, ret=ret, logp_old=logp_old, idx=idx, weight=weight, grads=grads, stats=stats, margin=margin)


def check_reference(case, d):
    """what the data must exercise, asserted on the reference"""
    cf = d["stats"]["clip_frac"]
    assert (0.2 <= cf <= 0.8) if case[0] > 1 else cf in (0.0, 1.0), cf        # (one row: 0 or 1, there is nothing between)
    assert d["margin"]["ratio"] > 1e-4 and d["margin"]["relu"] > 1e-5, d["margin"]


def make_learner(case, dtype, d=None, batch=None, **hyper):
    from beacon_amd import Actor, Learner
    m, obs_dim, hidden, activation, kind, n, sel = case
    a = Actor(_Env(batch or m, obs_dim, kind, n, dtype), hidden=hidden, activation=activation, seed=7)
    w = d["w"] if d is not None else weights_dict(obs_dim, hidden, kind, n, dtype)
    L = len(hidden) + 1
    a.load([(w["pi_w%d" % l], w["pi_b%d" % l]) for l in range(L)], [(w["vf_w%d" % l], w["vf_b%d" % l]) for l in range(L)],
           w["log_std"] if kind == "gaussian" else None)
    hp = dict(clip_range=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)
    hp.update(hyper)
    return Learner(a, **hp)


def dev_batch(d):
    c = lambda x: None if x is None else x.cuda()
    return dict(obs_rows=c(d["obs"]), actions=c(d["act"]), logp_old=c(d["logp_old"]), adv=c(d["adv"]), ret=c(d["ret"]), weight=c(d["weight"]),
                idx=c(d["idx"]))


def err(dev, ref):
    ref = torch.as_tensor(ref).double().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    return float((dev.double().cpu().reshape(-1) - ref).abs().max() / max(1.0, float(ref.abs().max())))


def tol_of(dtype, key, m):
    return f64_tol(m) if dtype == torch.float64 else F32_TOL[key][0]


def tag(dtype):
    return "f64" if dtype == torch.float64 else "f32"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_and_stats_match_reference(case, dtype):
    d = case_data(case, dtype, SEEDS[IDS[CASES.index(case)]])
    check_reference(case, d)
    ln = make_learner(case, dtype, d)
    grads, stats = ln.grad(**dev_batch(d))
    assert grads is ln.grads and stats is ln.stats and {k for k in grads if grads[k].numel()} == set(d["grads"])
    ge = {k: err(grads[k], g) for k, g in d["grads"].items()}
    dev_stats = ln.stats_dict()
    se = {k: abs(dev_stats[k] - v) / max(1.0, abs(v)) for k, v in d["stats"].items()}
    print("learner errors %s %s: grad %.3e (%s) stats %.3e (%s)" % (IDS[CASES.index(case)], tag(dtype), max(ge.values()), max(ge, key=ge.get),
                                                                   max(se.values()), max(se, key=se.get)))
    n_rows = 130 if case[6] else case[0]
    for k, e in ge.items():
        assert e <= tol_of(dtype, "grad", n_rows), (k, e)
    for k, e in se.items():
        assert e <= tol_of(dtype, "stats", n_rows), (k, e)
    assert dev_stats["weight"] == d["stats"]["weight"]                        # W is a sum of small integers: exact
    assert int(ln.step_count[0]) == 0                                         # grad() alone takes no optimiser step


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_zero_weights_are_invisible(kind, dtype):
    """Rows of weight 0 with NaN in adv, ret, logp_old and in their observation rows, named by idx: bit for bit the minibatch in which
    those rows are absent (their idx entries name no row, so they are staged as zeros like the rows behind m), every surviving row in
    the same tile position."""
    case = (257, 6, (64, 64), "tanh", kind, 3, None)
    rng = np.random.default_rng(5)
    w = weights_dict(6, (64, 64), kind, 3, dtype)
    t = lambda x: torch.as_tensor(x).to(dtype).cuda()
    obs, adv, ret, logp_old = t(rng.uniform(-1, 1, (257, 6))), t(rng.normal(size=257)), t(rng.normal(size=257)), t(rng.uniform(-1.5, -0.5, 257))
    act = t(rng.normal(0, 0.7, (257, 3))) if kind == "gaussian" else torch.as_tensor(rng.integers(0, 3, 257)).to(torch.int32).cuda()
    idx = torch.as_tensor(rng.permutation(257)[:200].copy()).to(torch.int32).cuda()
    weight = torch.as_tensor(rng.uniform(size=257) > 1.0 / 3.0).to(torch.uint8).cuda()
    dead = weight == 0
    assert 40 < int(dead[idx.long()].sum()) < 100
    ln = make_learner(case, dtype, dict(w=w))
    # the clean minibatch: the dead rows are absent
    idx_clean = torch.where(dead[idx.long()], torch.full_like(idx, -1), idx)
    ln.grad(obs, act, logp_old, adv, ret, weight=None, idx=idx_clean)
    want = (ln.grad_buf.clone(), ln.stats.clone())
    assert bool(torch.isfinite(want[1]).all()) and float(want[1][6]) == float((~dead[idx.long()]).sum())
    # the same rows with garbage where the weight is 0
    nan = float("nan")
    obs, adv, ret, logp_old = obs.clone(), adv.clone(), ret.clone(), logp_old.clone()
    obs[dead], adv[dead], ret[dead], logp_old[dead] = nan, nan, nan, nan
    ln.grad_buf.fill_(255)
    ln.grad(obs, act, logp_old, adv, ret, weight=weight, idx=idx)
    assert torch.equal(ln.grad_buf, want[0]) and torch.equal(ln.stats, want[1])
    # ... and as real weights
    ln.grad(obs, act, logp_old, adv, ret, weight=weight.to(dtype), idx=idx)
    assert torch.equal(ln.grad_buf, want[0]) and torch.equal(ln.stats, want[1])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_reproducible(dtype):
    """two grad() calls on the same inputs: the same bits, with several tiles per workgroup and with the idx selection"""
    for case in (CASES[5], CASES[4], CASES[1]):
        d = case_data(case, dtype, SEEDS[IDS[CASES.index(case)]])
        ln = make_learner(case, dtype, d)
        b = dev_batch(d)
        ln.grad(**b)
        first = (ln.grad_buf.clone(), ln.stats.clone())
        ln.work.fill_(255)                                                    # the work buffer needs no initialisation
        ln.grad_buf.zero_()
        ln.grad(**b)
        assert torch.equal(ln.grad_buf, first[0]) and torch.equal(ln.stats, first[1])


ADAM_CASE = (65, 6, (64, 64), "tanh", "gaussian", 2, None)
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-5)


@functools.lru_cache(maxsize=None)
def adam_reference(dtype, steps=5):
    """five reference steps on ADAM_CASE with a max_grad_norm between the norms the unclipped trajectory has: some steps clip, some do not"""
    d = case_data(ADAM_CASE, dtype, 11)

    def run(max_norm):
        ref = R.Ref(d["w"], ADAM_CASE[2], ADAM_CASE[3], 0)
        opt = ref.adam(ADAM["lr"], ADAM["betas"], ADAM["eps"])
        norms, margins = [], []
        for _ in range(steps):
            _, _, terms = ref.grad(d["obs"], d["act"], d["logp_old"], d["adv"], d["ret"], None, CLIP, VF_COEF, ENT_COEF)
            margins.append(float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()))
            norms.append(ref.clip_and_step(opt, max_norm))
        return ref, opt, norms, margins

    free = run(0.0)[2]
    max_norm = float(np.sort(free)[steps // 2 - 1] + np.sort(free)[steps // 2]) / 2.0
    ref, opt, norms, margins = run(max_norm)
    return d, ref, opt, max_norm, norms, margins


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_adam_matches_torch(dtype):
    steps = 5
    d, ref, opt, max_norm, norms, margins = adam_reference(dtype)
    clipped = [n > max_norm for n in norms]
    assert any(clipped) and not all(clipped), (norms, max_norm)                 # the one max_grad_norm clips in some steps, not in others
    assert min(margins) > 1e-4 and min(abs(n - max_norm) for n in norms) > 1e-3 * max_norm
    ln = make_learner(ADAM_CASE, dtype, d, max_grad_norm=max_norm, **ADAM)
    b = dev_batch(d)
    dev_norms = []
    for _ in range(steps):
        ln.grad(**b)
        ln.step()
        dev_norms.append(float(ln.stats[7]))
    assert ln.step_count.cpu().tolist()[0] == steps                            # exactly
    m_ref, v_ref, step_ref = ref.moments(opt)
    assert step_ref == steps
    esz = 8 if dtype == torch.float64 else 4
    seg = lambda flat, s: flat[s["offset"] // esz:s["offset"] // esz + s["row_elems"]]
    worst = {"adam_params": 0.0, "adam_m": 0.0, "adam_v": 0.0}
    for s in ln.grad_layout:
        name = s["name"]
        if s["row_elems"] == 0:
            continue
        worst["adam_params"] = max(worst["adam_params"], err(ln.actor.weights[name], dict(ref.named)[name].detach()))
        worst["adam_m"] = max(worst["adam_m"], err(seg(ln.m, s), m_ref[name]))
        worst["adam_v"] = max(worst["adam_v"], err(seg(ln.v, s), v_ref[name]))
    print("learner adam errors %s: %s; norms device %s reference %s, max_grad_norm %.6g"
          % (tag(dtype), " ".join("%s=%.3e" % kv for kv in sorted(worst.items())), dev_norms, norms, max_norm))
    # float64: m and v are linear / quadratic in the gradient (|g| <= 10 here): f64_tol and 20 f64_tol; a parameter moves by
    # lr m^ / (sqrt(v^) + eps) per step, whose sensitivity to the gradient is at most 1 / eps: steps x lr x f64_tol / eps
    t64 = f64_tol(65)
    f64 = {"adam_params": steps * ADAM["lr"] * t64 / ADAM["eps"], "adam_m": t64, "adam_v": 20.0 * t64}
    for k, e in worst.items():
        assert e <= (f64[k] if dtype == torch.float64 else F32_TOL[k][0]), (k, e)
    # the gaps between the segments stay zero in every buffer
    gap = torch.ones(ln.m.numel(), dtype=torch.bool, device=ln.m.device)
    for s in ln.grad_layout:
        seg(gap, s).fill_(False)
    for flat in (ln.m, ln.v, ln.grad_buf.view(dtype), ln.actor.params.view(dtype)):
        assert not bool(flat[gap].any())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_eager_equals_graph(dtype):
    """one grad() + step() captured in the caller's graph and replayed three times: the bits of three eager pairs; the step counter
    advances on the device at every replay"""
    case = CASES[4]
    d = case_data(case, dtype, SEEDS[IDS[4]])
    ln = make_learner(case, dtype, d, lr=1e-3, max_grad_norm=0.5)
    b = dev_batch(d)
    start = ln.actor.params.clone()
    for _ in range(3):
        ln.grad(**b)
        ln.step()
    eager = (ln.actor.params.clone(), ln.opt.clone(), ln.stats.clone())
    assert int(ln.step_count[0]) == 3 and not torch.equal(eager[0], start)
    ln.actor.params.copy_(start)
    ln.opt.zero_()
    ln.work.zero_()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        ln.grad(**b)
        ln.step()
    assert torch.equal(ln.actor.params, start) and int(ln.step_count[0]) == 0      # the capture launched nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ln.actor.params, eager[0]) and torch.equal(ln.opt, eager[1]) and torch.equal(ln.stats, eager[2])
    assert int(ln.step_count[0]) == 3


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_end_to_end_update(dtype):
    """VecBurgers, 8 replicas, 8 steps through actor.act() / step_autoreset, compute_gae, learner.update with a seeded generator --
    against the reference doing the same minibatches from the downloaded buffers."""
    import beacon_amd
    from beacon_amd import Actor, Learner
    T, B, hidden, epochs, nmb, seed = 8, 8, (16, 16), 2, 2, 1234
    env = beacon_amd.VecBurgers(B, dtype=tag(dtype), seed=5)
    actor = Actor(env, hidden=hidden, seed=21)
    pi, vf, ls = _weights(env.obs_dim, hidden, actor.act_dim, 1.0, 9)
    actor.load(pi, vf, ls)
    w0 = {k: v.detach().clone().cpu() for k, v in actor.weights.items()}
    ro = env.rollout(T)
    actor.attach(ro)
    env.reset()
    ro.begin()
    for _ in range(T):
        env.step_autoreset(actor.act())
    last_value = actor.values(env.obs)
    final_values = actor.values(ro.final_obs.reshape(T * B, env.obs_dim)).view(T, B)
    adv, ret = ro.compute_gae(actor.value_seq, last_value, final_values, gamma=0.99, lam=0.95)
    hp = dict(lr=3e-4, clip_range=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5)
    ln = Learner(actor, **hp)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    assert ln.update(ro, adv, ret, epochs=epochs, minibatches=nmb, generator=gen) is ln
    assert ro.check() == (T, False)                                               # the one host read of the cursor, after the update
    assert int(ln.step_count[0]) == epochs * nmb

    N = T * B
    cpu = lambda x: x.detach().double().cpu()
    obs, raw, logp_old, valid = cpu(ro.obs[:-1]).reshape(N, -1), cpu(actor.raw_seq).reshape(N, -1), cpu(actor.logp_seq).reshape(N), cpu(ro.valid).reshape(N)
    a64, r64 = cpu(adv).reshape(N), cpu(ret).reshape(N)
    on = valid > 0
    assert int(on.sum()) == N
    a64 = (a64 - a64[on].mean()) / (a64[on].std() + 1e-8)
    ref = R.Ref(w0, hidden, "tanh", 0)
    opt = ref.adam(hp["lr"], hp["betas"], hp["eps"])
    gen2 = torch.Generator(device="cuda").manual_seed(seed)
    for _ in range(epochs):
        perm = torch.randperm(N, device="cuda", generator=gen2).cpu()
        for k in range(nmb):
            rows = perm[k * N // nmb:(k + 1) * N // nmb]
            _, _, terms = ref.grad(obs[rows], raw[rows], logp_old[rows], a64[rows], r64[rows], valid[rows], CLIP, VF_COEF, ENT_COEF)
            assert float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()) > 1e-4
            ref.clip_and_step(opt, hp["max_grad_norm"])
    worst = max(err(actor.weights[name], p.detach()) for name, p in ref.named)
    moved = max(float((p.detach() - w0[name].double().reshape(p.shape)).abs().max()) for name, p in ref.named)
    print("learner end-to-end %s: worst parameter error %.3e, the update moved a parameter by %.3e" % (tag(dtype), worst, moved))
    assert moved > 1e-4                                                             # the comparison is of an update that happened
    # float64: four steps of at most lr each, each with the gradient's bound over the Adam sensitivity 1 / eps
    assert worst <= (epochs * nmb * hp["lr"] * f64_tol(N // nmb) / hp["eps"] if dtype == torch.float64 else F32_TOL["e2e_params"][0]), worst
    env.close()
