"""The host-free PPO update on the MI355X: libbeacon_epochs.so (the shuffle, the standardisation), the KL stop rule and the
learning-rate schedule of bcn_learner_step, and Learner.plan over them -- against tests/epochs_ref.py (NumPy, written from
include/beacon_epochs.h) and tests/learner_ref.py (torch autograd and torch.optim.Adam in float64 on the CPU).

Integers and decisions are compared exactly: a permutation with torch.equal, the counters of the optimiser's step segment as lists,
"nothing moved" and "eager equals graph" bit for bit.  Tolerances, where there are any:
  standardisation, float64   2 (N - 1) u (M + max |out|) + 4 u max |out| with u = 2^-53 and M = max |adv - mean| / std of the case's
                             own active rows (std_tol below derives it); asserted to lie below 1e-9
  standardisation, float32   2^-23 max(1, |ref|): a float64 computation on exact float32 inputs, rounded once
  Adam under the schedule    the tolerances of test_gpu_learner.test_adam_matches_torch, taken from there
  end to end, float64        the bound of test_gpu_learner.test_end_to_end_update
  end to end, float32        F32_E2E = (tolerance, measured on the MI355X), tolerance <= 10 x measured, the project's rule; and at most
                             8 x the error of learner_ref.Ref(dtype=torch.float32) doing the same update on the same numbers"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import epochs_ref as E
import learner_ref as R
import test_gpu_learner as G
from test_gpu_actor import _weights

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
U64 = 2.0 ** -53
# float32, the end-to-end update through plan.run: (tolerance, worst parameter error measured on the MI355X)
F32_E2E = (4.5e-7, 4.562e-8)          # (the float32 reference's own error on the same update: 4.562e-8 as well)
F32_FACTOR = 8.0


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _epochs():
    from beacon_amd import epochs
    return epochs, epochs.load()


# ---- 1. the permutation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, 0xDEADBEEFCAFEF00D], ids=["seed7", "seed64"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 257, 4097, 65537, (1 << 20) + 1])
def test_permutation_equals_the_host_restatement(n, seed):
    """two draws in a row from a zeroed counter word: the host's epochs 0 and 1, the word reads 2 afterwards; nothing is written
    outside idx [n] and the one word"""
    epochs, L = _epochs()
    pad = 64
    buf = torch.full((n + 2 * pad,), -7, dtype=torch.int32, device="cuda")
    idx = buf[pad:pad + n]
    step = torch.zeros(4, dtype=torch.int32, device="cuda")
    for epoch in (0, 1):
        epochs._check(L.bcn_epochs_permute(n, seed, _ptr(step, 4), _ptr(idx), _stream()))
        want = torch.as_tensor(E.permutation(n, seed, epoch), dtype=torch.int32)
        assert torch.equal(idx.cpu(), want), (n, seed, epoch)
        assert step.cpu().tolist() == [0, epoch + 1, 0, 0]
    assert bool((buf[:pad] == -7).all()) and bool((buf[pad + n:] == -7).all())
    # a counter word with its top bit set is the epoch 2^31 (the word's bits as uint32), and the tick wraps it like one
    step[1] = -(1 << 31)
    epochs._check(L.bcn_epochs_permute(n, seed, _ptr(step, 4), _ptr(idx), _stream()))
    assert torch.equal(idx.cpu(), torch.as_tensor(E.permutation(n, seed, 1 << 31), dtype=torch.int32))
    assert step.cpu().tolist() == [0, -(1 << 31) + 1, 0, 0]


# ---- 2. the standardisation -------------------------------------------------------------------------------------------------------------
# name -> (n_rows, weights, rows_per_weight, (steps T, cursor) or None).  The grid is 64 workgroups over chunks of 1024 rows:
#   one, two              the two max(., 1) clamps: one active row of one, one active row of two
#   257                   a partial chunk, one workgroup, no weights
#   70001-real            69 chunks: the workgroups 0 .. 4 walk a second chunk (rows from 65 536 on); real weights, a third of them 0,
#                         some NaN (not > 0: inactive)
#   69993-u8-cursor-rpw3  21 steps of 1111 replicas of 3 jets, 69 chunks as well; uint8 weights per replica, a third of them 0; the
#                         cursor at 20 of 21 steps cuts 3333 rows off, inside workgroup 1's second chunk
STD_CASES = {"one": (1, None, 1, None), "two": (2, "u8-first", 1, None), "257": (257, None, 1, None),
             "70001-real": (70001, "real", 1, None), "69993-u8-cursor-rpw3": (69993, "u8", 3, (21, 20))}


@functools.lru_cache(maxsize=None)
def std_data(name, dtype):
    """the inputs of a case as the device will hold them (CPU tensors; NaN in every inactive row) and the float64 two-pass reference"""
    n, wkind, rpw, steps = STD_CASES[name]
    rng = np.random.default_rng(len(name) + n)
    adv = torch.as_tensor(rng.normal(0.3, 1.7, n)).to(dtype)
    weight = None
    if wkind == "u8-first":
        weight = torch.tensor([1, 0], dtype=torch.uint8)
    elif wkind == "u8":
        weight = torch.as_tensor(rng.uniform(size=n // rpw) > 1.0 / 3.0).to(torch.uint8)
    elif wkind == "real":
        w = rng.uniform(0.25, 2.0, n) * (rng.uniform(size=n) > 1.0 / 3.0)
        w[rng.integers(0, n, 50)] = np.nan
        weight = torch.as_tensor(w).to(dtype)
    cursor, rps = (None, 0) if steps is None else (steps[1], n // steps[0])
    on = E.active_rows(n, None if weight is None else weight.double().numpy(), rpw, cursor, rps)
    adv[torch.as_tensor(~on)] = float("nan")
    ref, mean, var, count = E.standardise(adv.double().numpy(), on)
    return dict(n=n, adv=adv, weight=weight, rpw=rpw, cursor=cursor, rps=rps, on=on, ref=ref, mean=mean, var=var, count=count)


def std_tol(d, dtype):
    """float32: 2^-23 max(1, |ref|) per element.  float64: the device and NumPy add the same c <= N numbers in different orders.  Each
    sum of c terms is off by at most (c - 1) u sum |term|: the mean by (N - 1) u max |adv - mean| once the common offset is taken out
    -- the shift of every output by that over std, (N - 1) u M -- and the variance, a sum of non-negative terms, by a relative
    (N - 1) u, which scales every output by at most that.  Both sides err, hence the 2; the last term is the roundings of the
    subtraction, the division and the square root.  One number for the whole case."""
    if dtype == torch.float32:
        return 2.0 ** -23 * np.maximum(1.0, np.abs(d["ref"]))
    a = d["adv"].double().numpy()[d["on"]]
    std = np.sqrt(d["var"]) + 1e-8
    M = float(np.abs(a - d["mean"]).max() / std) if a.size else 0.0
    top = float(np.abs(d["ref"]).max())
    tol = 2.0 * (d["n"] - 1) * U64 * (M + top) + 4.0 * U64 * top
    assert tol < 1e-9, tol
    return tol


def _begin(d, dtype, step=None, normalize=True):
    """bcn_epochs_begin on the case's data: (adv_out with guard elements around it stripped, moments, the guards intact)"""
    epochs, L = _epochs()
    n, pad = d["n"], 32
    adv = d["adv"].cuda()
    buf = torch.full((n + 2 * pad,), 123.0, dtype=dtype, device="cuda")
    out = buf[pad:pad + n]
    weight = None if d["weight"] is None else d["weight"].cuda()
    cursor = None if d["cursor"] is None else torch.tensor([d["cursor"], 0, 0, 0], dtype=torch.int32, device="cuda")
    segs, nbytes = epochs.work_layout()
    work = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")            # "it needs no initialisation"
    wk = epochs.W_NONE if weight is None else (epochs.W_U8 if weight.dtype == torch.uint8 else epochs.W_REAL)
    b = epochs.EpochsBatch(adv=_ptr(adv), adv_out=_ptr(out), weight=None if weight is None else _ptr(weight),
                           cursor=None if cursor is None else _ptr(cursor), step=None if step is None else _ptr(step), work=_ptr(work),
                           n_rows=n, dtype=1 if dtype == torch.float64 else 0, normalize=int(normalize), weight_kind=wk,
                           rows_per_step=d["rps"], rows_per_weight=d["rpw"])
    epochs._check(L.bcn_epochs_begin(C.byref(b), _stream()))
    torch.cuda.synchronize()
    moments = work[segs[0]["offset"]:segs[0]["offset"] + 32].view(torch.float64).cpu().tolist()
    guards = bool((buf[:pad] == 123.0).all()) and bool((buf[pad + n:] == 123.0).all())
    return out.clone(), moments, guards


@DTYPES
@pytest.mark.parametrize("name", list(STD_CASES))
def test_standardisation_matches_the_two_pass_reference(name, dtype):
    d = std_data(name, dtype)
    n, on = d["n"], d["on"]
    assert 0 < d["count"] and (name in ("one", "257") or d["count"] < n)             # every masked case has inactive rows
    if n > 65536:
        assert -(-n // 1024) > 64 and on[65536:].any() and (~on[65536:]).any()      # the second chunk holds rows of both sorts
    step = torch.tensor([5, 6, 1, 7], dtype=torch.int32, device="cuda")
    out, moments, guards = _begin(d, dtype, step)
    assert guards
    assert step.cpu().tolist() == [5, 6, 0, 7]                                       # the flag cleared, no other word touched
    o = out.double().cpu().numpy()
    err = np.abs(o - d["ref"])
    tol = std_tol(d, dtype)
    print("epochs standardisation %s %s: %d of %d rows active, worst error %.3e (tolerance %.3e), mean %.6g var %.6g"
          % (name, G.tag(dtype), d["count"], n, float(err.max()), float(np.max(tol)), d["mean"], d["var"]))
    assert np.isfinite(o).all() and (err <= tol).all(), float(err.max())
    # inactive rows: +0 in every bit
    bits = out.view(torch.int64 if dtype == torch.float64 else torch.int32).cpu().numpy()
    assert (bits[~on] == 0).all()
    if name == "one":
        assert bits[0] == 0                                                          # (x - x) / 1e-8
    if name == "two":
        assert o[0] == 0.0 and moments[2] == 1.0 and moments[1] == 0.0               # c - 1 = 0 is clamped to 1: var 0, no NaN
    assert moments[2] == float(d["count"])                                           # exactly
    # mean and var themselves: two orders of the same sums of c <= n terms (the variance: non-negative ones), and a division
    top = float(np.abs(d["adv"].double().numpy()[on]).max())
    assert abs(moments[0] - d["mean"]) <= 2.0 * (n - 1) * U64 * top + 2.0 * U64 * abs(d["mean"]), (moments[0], d["mean"])
    assert abs(moments[1] - d["var"]) <= (2.0 * (n - 1) + 8.0) * U64 * d["var"], (moments[1], d["var"])
    assert moments[3] == np.sqrt(moments[1]) + 1e-8
    # run to run: the same bits, whatever the work buffer held before
    again, moments2, _ = _begin(d, dtype, step)
    assert torch.equal(out.view(torch.uint8), again.view(torch.uint8)) and moments2 == moments


def test_begin_without_normalize_clears_the_flag_alone():
    d = std_data("257", torch.float32)
    step = torch.tensor([5, 6, 1, 7], dtype=torch.int32, device="cuda")
    out, _, guards = _begin(d, torch.float32, step, normalize=False)
    assert step.cpu().tolist() == [5, 6, 0, 7] and guards and bool((out == 123.0).all())      # adv_out is not written


# ---- 3. the KL stop rule ----------------------------------------------------------------------------------------------------------------
KL_PAIRS, KL_SHIFT, KL_LR = 6, 0.02, 1e-3


@functools.lru_cache(maxsize=None)
def kl_reference(dtype):
    """ADAM_CASE of test_gpu_learner (65 rows) with logp_old = the policy's own log-probabilities shifted by KL_SHIFT: approx_kl grows
    with every step.  The float64 reference takes KL_PAIRS grad + step pairs under the header's rule, restated here; target_kl puts the
    threshold half way between the second and the third pair's approx_kl.  Returns (data, logp_old, target_kl, the pairs' approx_kl,
    steps taken, steps skipped)."""
    d = G.case_data(G.ADAM_CASE, dtype, 11)
    hidden, act = G.ADAM_CASE[2], G.ADAM_CASE[3]
    args = lambda lo: (d["obs"], d["act"], lo, d["adv"], d["ret"], None, G.CLIP, G.VF_COEF, G.ENT_COEF)
    free = R.Ref(d["w"], hidden, act, 0)
    with torch.no_grad():
        logp = free.terms(*args(torch.zeros(65)))["logp"]
    logp_old = (logp + KL_SHIFT).to(dtype)
    opt = free.adam(KL_LR, G.ADAM["betas"], G.ADAM["eps"])
    first = []
    for _ in range(3):
        first.append(free.grad(*args(logp_old))[1]["approx_kl"])
        free.clip_and_step(opt, 0.5)
    assert first[2] > max(first[:2])
    target_kl = 0.5 * (max(first[:2]) + first[2]) / 1.5
    ref = R.Ref(d["w"], hidden, act, 0)
    opt = ref.adam(KL_LR, G.ADAM["betas"], G.ADAM["eps"])
    flag, steps, skipped, kls = False, 0, 0, []
    for _ in range(KL_PAIRS):
        kl = ref.grad(*args(logp_old))[1]["approx_kl"]
        kls.append(kl)
        flag = flag or kl > 1.5 * target_kl
        if flag:
            skipped += 1
        else:
            ref.clip_and_step(opt, 0.5)
            steps += 1
    return d, logp_old, target_kl, kls, steps, skipped


def check_kl_reference(dtype):
    """what the case must show, asserted on the reference (tests/test_epochs_host.py has no GPU and calls this too)"""
    _, _, target_kl, kls, steps, skipped = kl_reference(dtype)
    thr = 1.5 * target_kl
    assert (steps, skipped) == (2, 4) and kls[0] <= thr and kls[1] <= thr and kls[2] > thr
    assert all(abs(k - thr) >= 1e-3 * thr for k in kls), (kls, thr)                   # no pair's decision hangs on roundoff
    assert kls[3:] == [kls[2]] * 3                                                    # nothing moves behind the stop


@DTYPES
def test_kl_stop(dtype):
    epochs, L = _epochs()
    check_kl_reference(dtype)
    d, logp_old, target_kl, kls, _, _ = kl_reference(dtype)
    hp = dict(lr=KL_LR, max_grad_norm=0.5, betas=G.ADAM["betas"], eps=G.ADAM["eps"])
    ln = G.make_learner(G.ADAM_CASE, dtype, d, target_kl=target_kl, **hp)
    b = dict(G.dev_batch(d), logp_old=logp_old.cuda())
    ln.step_count[1] = 9                                                              # the permutation counter is not the stop rule's
    after, dev_kl = [], []
    for _ in range(KL_PAIRS):
        ln.grad(**b)
        ln.step()
        dev_kl.append(float(ln.stats[4]))
        after.append((ln.actor.params.clone(), ln.m.clone(), ln.v.clone()))
    print("epochs kl stop %s: target_kl %.6e, approx_kl device %s reference %s" % (G.tag(dtype), target_kl, dev_kl, kls))
    assert ln.step_count.cpu().tolist() == [2, 9, 1, 4] and ln.skipped == 4
    assert not torch.equal(after[1][0], after[0][0])                                  # two steps were taken ...
    for x, y in zip(after[5], after[1]):                                              # ... and nothing has moved since, bit for bit
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    # the flag holds whatever target_kl a later step is given, until begin clears it
    ln.set_hyper(target_kl=1.0)
    ln.grad(**b)
    ln.step()
    assert ln.step_count.cpu().tolist() == [2, 9, 1, 5] and torch.equal(ln.actor.params, after[1][0])
    bb = epochs.EpochsBatch(step=_ptr(ln.step_count), normalize=0)
    epochs._check(L.bcn_epochs_begin(C.byref(bb), _stream()))
    assert ln.step_count.cpu().tolist() == [2, 9, 0, 5]
    ln.grad(**b)
    ln.step()
    assert ln.step_count.cpu().tolist() == [3, 9, 0, 5] and not torch.equal(ln.actor.params, after[1][0])
    # a NaN approx_kl does not stop
    ln.stats[4] = float("nan")
    ln.step()
    assert ln.step_count.cpu().tolist() == [4, 9, 0, 5]


@DTYPES
def test_target_kl_zero_is_the_path_without_the_field(dtype):
    """the same six pairs with target_kl = 0 and on a learner built without the argument: the same bits everywhere, and the words 1 .. 3
    of the step segment are not touched"""
    d, logp_old, _, _, _, _ = kl_reference(dtype)
    hp = dict(lr=KL_LR, max_grad_norm=0.5, betas=G.ADAM["betas"], eps=G.ADAM["eps"])
    b = dict(G.dev_batch(d), logp_old=logp_old.cuda())
    runs = []
    for extra in (dict(), dict(target_kl=0.0), dict(target_kl=None, lr_end=1e-5, lr_steps=0)):
        ln = G.make_learner(G.ADAM_CASE, dtype, d, **hp, **extra)
        ln.step_count[1:] = torch.tensor([11, 12, 13], dtype=torch.int32)
        for _ in range(KL_PAIRS):
            ln.grad(**b)
            ln.step()
        assert ln.step_count.cpu().tolist() == [KL_PAIRS, 11, 12, 13]
        runs.append((ln.actor.params.clone(), ln.opt.clone(), ln.stats.clone(), ln.grad_buf.clone()))
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---- 4. the learning-rate schedule ------------------------------------------------------------------------------------------------------
LR_STEPS, LR_MAX_NORM = 4, 0.25


@functools.lru_cache(maxsize=None)
def lr_reference(dtype, steps=5):
    """five torch.optim.Adam steps on ADAM_CASE with lr_t = lr + (0 - lr) min(s, 4) / 4 set before step s (s steps taken so far)"""
    d = G.case_data(G.ADAM_CASE, dtype, 11)
    ref = R.Ref(d["w"], G.ADAM_CASE[2], G.ADAM_CASE[3], 0)
    opt = ref.adam(G.ADAM["lr"], G.ADAM["betas"], G.ADAM["eps"])
    norms, margins, lrs = [], [], []
    for s in range(steps):
        lr_t = G.ADAM["lr"] + (0.0 - G.ADAM["lr"]) * min(s, LR_STEPS) / LR_STEPS
        for group in opt.param_groups:
            group["lr"] = lr_t
        _, _, terms = ref.grad(d["obs"], d["act"], d["logp_old"], d["adv"], d["ret"], None, G.CLIP, G.VF_COEF, G.ENT_COEF)
        margins.append(float((terms["ratio"] - 1.0).abs().sub(G.CLIP).abs().min()))
        norms.append(ref.clip_and_step(opt, LR_MAX_NORM))
        lrs.append(lr_t)
    return d, ref, opt, norms, margins, lrs


def check_lr_reference(dtype):
    _, _, _, norms, margins, lrs = lr_reference(dtype)
    assert lrs == [1e-3, 7.5e-4, 5e-4, 2.5e-4, 0.0]
    assert min(margins) > 1e-4 and min(abs(n - LR_MAX_NORM) for n in norms) > 1e-3 * LR_MAX_NORM, (margins, norms)


@DTYPES
def test_lr_schedule_matches_torch(dtype):
    steps = 5
    check_lr_reference(dtype)
    d, ref, opt, norms, _, _ = lr_reference(dtype)
    ln = G.make_learner(G.ADAM_CASE, dtype, d, max_grad_norm=LR_MAX_NORM, lr_end=0.0, lr_steps=LR_STEPS, **G.ADAM)
    b = G.dev_batch(d)
    before_last = None
    for s in range(steps):
        if s == steps - 1:
            before_last = (ln.actor.params.clone(), ln.m.clone())
        ln.grad(**b)
        ln.step()
    assert ln.step_count.cpu().tolist() == [steps, 0, 0, 0]
    assert torch.equal(ln.actor.params.view(torch.uint8), before_last[0].view(torch.uint8))     # lr_t = 0: the fifth step moves no parameter
    assert not torch.equal(ln.m, before_last[1])                                                # ... while it is a step: the moments move
    m_ref, v_ref, step_ref = ref.moments(opt)
    assert step_ref == steps
    esz = 8 if dtype == torch.float64 else 4
    seg = lambda flat, s: flat[s["offset"] // esz:s["offset"] // esz + s["row_elems"]]
    worst = {"adam_params": 0.0, "adam_m": 0.0, "adam_v": 0.0}
    for s in ln.grad_layout:
        name = s["name"]
        if s["row_elems"] == 0:
            continue
        worst["adam_params"] = max(worst["adam_params"], G.err(ln.actor.weights[name], dict(ref.named)[name].detach()))
        worst["adam_m"] = max(worst["adam_m"], G.err(seg(ln.m, s), m_ref[name]))
        worst["adam_v"] = max(worst["adam_v"], G.err(seg(ln.v, s), v_ref[name]))
    print("epochs lr schedule %s: %s; reference norms %s" % (G.tag(dtype), " ".join("%s=%.3e" % kv for kv in sorted(worst.items())), norms))
    # the tolerances of test_adam_matches_torch: the same case, the same number of steps, no step larger than its lr
    t64 = G.f64_tol(65)
    f64 = {"adam_params": steps * G.ADAM["lr"] * t64 / G.ADAM["eps"], "adam_m": t64, "adam_v": 20.0 * t64}
    for k, e in worst.items():
        assert e <= (f64[k] if dtype == torch.float64 else G.F32_TOL[k][0]), (k, e)
    # behind lr_steps the rate stays lr_end: with lr_end > 0 a sixth step moves the parameters again
    ln.set_hyper(lr_end=1e-4)
    ln.grad(**b)
    ln.step()
    assert not torch.equal(ln.actor.params, before_last[0]) and int(ln.step_count[0]) == steps + 1


# ---- 5. the plan, end to end ------------------------------------------------------------------------------------------------------------
HP = dict(lr=3e-4, clip_range=G.CLIP, vf_coef=G.VF_COEF, ent_coef=G.ENT_COEF, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5)
_BURGERS = {}


def _burgers(dtype):
    """VecBurgers, 8 replicas, 8 steps through actor.act() / step_autoreset and compute_gae, as test_gpu_learner.test_end_to_end_update;
    built once per dtype and never modified behind `start`: {env, actor, ro, adv, ret, start (the parameters before any update)}"""
    if dtype in _BURGERS:
        return _BURGERS[dtype]
    import beacon_amd
    from beacon_amd import Actor
    T, B, hidden = 8, 8, (16, 16)
    env = beacon_amd.VecBurgers(B, dtype=G.tag(dtype), seed=5)
    actor = Actor(env, hidden=hidden, seed=21)
    pi, vf, ls = _weights(env.obs_dim, hidden, actor.act_dim, 1.0, 9)
    actor.load(pi, vf, ls)
    ro = env.rollout(T)
    actor.attach(ro)
    env.reset()
    ro.begin()
    for _ in range(T):
        env.step_autoreset(actor.act())
    last_value = actor.values(env.obs)
    final_values = actor.values(ro.final_obs.reshape(T * B, env.obs_dim)).view(T, B)
    adv, ret = ro.compute_gae(actor.value_seq, last_value, final_values, gamma=0.99, lam=0.95)
    _BURGERS[dtype] = dict(env=env, actor=actor, ro=ro, adv=adv, ret=ret, T=T, B=B, hidden=hidden, start=actor.params.clone())
    return _BURGERS[dtype]


def _reference_update(w0, hidden, rows, valid_rows, N, seed, epochs, nmb, dtype=torch.float64):
    """the update of plan.run by the reference: the minibatches of epochs_ref.permutation for the epochs 0, 1, ..., torch's Adam behind
    clip_grad_norm_, in `dtype`.  rows = (obs, raw, logp_old, the STANDARDISED adv, ret), float64 [N ...]; valid_rows: a weight per row"""
    obs, raw, logp_old, a, ret = rows
    ref = R.Ref(w0, hidden, "tanh", 0, dtype=dtype)
    opt = ref.adam(HP["lr"], HP["betas"], HP["eps"])
    for e in range(epochs):
        perm = torch.as_tensor(E.permutation(N, seed, e))
        for k in range(nmb):
            sel = perm[k * N // nmb:(k + 1) * N // nmb]
            _, _, terms = ref.grad(obs[sel], raw[sel], logp_old[sel], a[sel], ret[sel], valid_rows[sel], G.CLIP, G.VF_COEF, G.ENT_COEF)
            assert float((terms["ratio"].double() - 1.0).abs().sub(G.CLIP).abs().min()) > 1e-4
            ref.clip_and_step(opt, HP["max_grad_norm"])
    return ref


@DTYPES
def test_end_to_end_plan_run(dtype):
    from beacon_amd import Learner
    r = _burgers(dtype)
    actor, ro, adv, ret, T, B, hidden = r["actor"], r["ro"], r["adv"], r["ret"], r["T"], r["B"], r["hidden"]
    epochs, nmb, seed, N = 2, 2, 7, T * B
    actor.params.copy_(r["start"])
    w0 = {k: v.detach().clone().cpu() for k, v in actor.weights.items()}
    ln = Learner(actor, **HP)
    plan = ln.plan(ro, epochs=epochs, minibatches=nmb, seed=seed)
    assert plan.run(adv, ret) is plan
    assert ro.check() == (T, False)
    assert ln.step_count.cpu().tolist() == [epochs * nmb, epochs, 0, 0]
    assert torch.equal(plan.idx.cpu(), torch.as_tensor(E.permutation(N, seed, epochs - 1), dtype=torch.int32))   # the last epoch's shuffle
    assert ln.plan(ro).seed == actor.seed == 21                                       # the default seed is the actor's

    cpu = lambda x: x.detach().double().cpu()
    rows = (cpu(ro.obs[:-1]).reshape(N, -1), cpu(actor.raw_seq).reshape(N, -1), cpu(actor.logp_seq).reshape(N), cpu(adv).reshape(N), cpu(ret).reshape(N))
    valid = cpu(ro.valid).reshape(N)
    assert int((valid > 0).sum()) == N
    want_adv = E.standardise(rows[3].numpy(), valid.numpy() > 0)[0]
    tol_adv = 2.0 ** -23 * np.maximum(1.0, np.abs(want_adv)) if dtype == torch.float32 else 1e-12
    assert (np.abs(plan.adv_norm.double().cpu().numpy() - want_adv) <= tol_adv).all()
    # the references get the standardised advantages in the buffer's precision, as adv_norm holds them
    rows = rows[:3] + (torch.as_tensor(want_adv).to(dtype).double(), rows[4])
    ref = _reference_update(w0, hidden, rows, valid, N, seed, epochs, nmb)
    worst = max(G.err(actor.weights[name], p.detach()) for name, p in ref.named)
    moved = max(float((p.detach() - w0[name].double().reshape(p.shape)).abs().max()) for name, p in ref.named)
    assert moved > 1e-4                                                               # the comparison is of an update that happened
    if dtype == torch.float64:
        print("epochs end-to-end f64: worst parameter error %.3e, the update moved a parameter by %.3e" % (worst, moved))
        # test_end_to_end_update's bound: four steps of at most lr each, each with the gradient's bound over the Adam sensitivity 1 / eps
        assert worst <= epochs * nmb * HP["lr"] * G.f64_tol(N // nmb) / HP["eps"], worst
    else:
        threads = torch.get_num_threads()
        torch.set_num_threads(1)                      # the blocks of torch's float32 sums follow the thread count: fix it
        try:
            ref32 = _reference_update(w0, hidden, rows, valid, N, seed, epochs, nmb, torch.float32)
        finally:
            torch.set_num_threads(threads)
        worst32 = max(G.err(p32.detach(), p.detach()) for (_, p32), (_, p) in zip(ref32.named, ref.named))
        print("epochs end-to-end f32: worst parameter error %.3e (the float32 reference: %.3e, ratio %.2f), the update moved a parameter by %.3e"
              % (worst, worst32, worst / worst32 if worst32 else float("inf"), moved))
        assert F32_E2E[0] <= 10.0 * F32_E2E[1]
        assert worst <= F32_E2E[0], worst
        assert worst <= F32_FACTOR * worst32, (worst, worst32)


def test_end_to_end_plan_run_per_jet():
    """the same on VecShkadov(13, n_jets=5), the film of tests/test_gpu_actor_jets.py, with a per-jet actor: T B A rows, the rollout's
    per-replica valid bytes weighing the A rows of their replica, in float64"""
    import beacon_amd
    from beacon_amd import Actor, Learner
    from beacon_amd.envs import packaged_init
    dtype, T, B, A, hidden = torch.float64, 4, 13, 5, (16, 16)
    env = beacon_amd.VecShkadov(B, "cuda:0", "f64", init_fields=packaged_init("shkadov"), n_jets=A, t_act=0.15, seed=5)
    env.set_jet_rewards()
    actor = Actor(env, hidden=hidden, seed=21, per_jet=True)
    pi, vf, ls = _weights(env.n_obs, hidden, 1, 2.0, 9)
    actor.load(pi, vf, ls)
    ro = env.rollout(T)
    actor.attach(ro)
    env.reset()
    ro.begin()
    for _ in range(T):
        env.step_autoreset(actor.act())
    adv, ret = ro.compute_gae(actor.value_seq, actor.values(env.obs.view(-1, env.n_obs)), actor.values(ro.final_obs.view(-1, env.n_obs)), per_jet=True)
    w0 = {k: v.detach().clone().cpu() for k, v in actor.weights.items()}
    epochs, nmb, seed, N = 2, 3, 1234, T * B * A
    ln = Learner(actor, **HP)
    zeros = torch.zeros(T, B, dtype=dtype, device="cuda")
    plan = ln.plan(ro, epochs=epochs, minibatches=nmb, seed=seed)
    with pytest.raises(ValueError, match=r"compute_gae\(\.\.\., per_jet=True\)"):
        plan.run(zeros, zeros)
    assert (plan.N, plan.A) == (N, A) and plan.idx.numel() == N
    plan.run(adv, ret)
    assert ro.check() == (T, False) and ln.step_count.cpu().tolist() == [epochs * nmb, epochs, 0, 0]
    assert plan.moments_dict()["count"] == float(N)                                   # the pool: every valid step counts once per jet
    cpu = lambda x: x.detach().double().cpu()
    rows = (cpu(ro.obs[:-1]).reshape(N, env.n_obs), cpu(actor.raw_seq).reshape(N, 1), cpu(actor.logp_seq).reshape(N), cpu(adv).reshape(N), cpu(ret).reshape(N))
    valid = cpu(ro.valid).view(T, B).repeat_interleave(A, dim=1).reshape(N)
    rows = rows[:3] + (torch.as_tensor(E.standardise(rows[3].numpy(), valid.numpy() > 0)[0]), rows[4])
    ref = _reference_update(w0, hidden, rows, valid, N, seed, epochs, nmb)
    worst = max(G.err(actor.weights[name], p.detach()) for name, p in ref.named)
    moved = max(float((p.detach() - w0[name].double().reshape(p.shape)).abs().max()) for name, p in ref.named)
    print("epochs end-to-end per jet f64: worst parameter error %.3e, the update moved a parameter by %.3e" % (worst, moved))
    assert moved > 1e-4
    assert worst <= epochs * nmb * HP["lr"] * G.f64_tol(-(-N // nmb)) / HP["eps"], worst
    env.close()


# ---- 6. one graph -----------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_two_replays_equal_two_eager_runs(dtype):
    from beacon_amd import Learner
    r = _burgers(dtype)
    actor, ro, adv, ret = r["actor"], r["ro"], r["adv"], r["ret"]
    epochs, nmb = 2, 2
    snap = lambda ln, plan: [x.clone() for x in (actor.params, ln.opt, plan.idx, plan.adv_norm, ln.stats, plan.moments)]
    actor.params.copy_(r["start"])
    ln = Learner(actor, target_kl=0.5, lr_end=1e-5, lr_steps=6, **HP)                 # the rule and the schedule are in the graph too
    plan = ln.plan(ro, epochs=epochs, minibatches=nmb, seed=7)
    plan.run(adv, ret)
    first = snap(ln, plan)
    plan.run(adv, ret)
    eager = snap(ln, plan)
    assert ln.step_count.cpu().tolist() == [2 * epochs * nmb, 2 * epochs, 0, 0]
    assert not torch.equal(first[0], r["start"]) and not torch.equal(eager[0], first[0]) and not torch.equal(eager[2], first[2])

    actor.params.copy_(r["start"])
    ln2 = Learner(actor, target_kl=0.5, lr_end=1e-5, lr_steps=6, **HP)
    plan2 = ln2.plan(ro, epochs=epochs, minibatches=nmb, seed=7)
    g = plan2.capture(adv, ret)
    torch.cuda.synchronize()
    assert torch.equal(actor.params, r["start"]) and ln2.step_count.cpu().tolist() == [0, 0, 0, 0]      # the capture launched nothing
    assert not bool(plan2.idx.any()) and not bool(plan2.adv_norm.any())
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(snap(ln2, plan2), first):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(snap(ln2, plan2), eager):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert ln2.step_count.cpu().tolist() == [2 * epochs * nmb, 2 * epochs, 0, 0]
