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
m = 16 385.  A case whose own chain, obs_dim + sum(hidden), is longer takes that length for the 640 (896 at the limits), and
check_reference asserts the four bounds on the reference's numbers (the per-row term: learner_ref.Ref.row_term_max).
float32: the project's rule -- every tolerance in F32_TOL is at most 10 x the worst error measured on the MI355X over the cases; both
numbers stand next to each other there.  Under err() that is an ABSOLUTE 2e-6 for gradients whose segments have max |ref| of 2e-4 to
1, so beside it every float32 gradient is held to its own scale: per segment, rel(device) <= 8 x rel(cpu32), rel(x) = max |x - ref64|
/ max |ref64| and cpu32 the float32 reference (learner_ref.Ref(dtype=torch.float32)) on the same float32 data -- F32_FACTOR below."""
import functools

import numpy as np
import pytest
import torch

import learner_ref as R
from test_gpu_actor import _Env, _weights

pytestmark = pytest.mark.gpu

CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01
U64 = 2.0 ** -53


def f64_tol(m, chain=640):
    return (m + max(640, chain)) * U64 * 500.0


# float32: quantity -> (tolerance, worst error measured on the MI355X)
F32_TOL = {"grad": (2.0e-6, 2.087e-7), "stats": (2.3e-6, 2.360e-7),                             # test_gradient_and_stats_match_reference, over CASES
           "adam_params": (8.7e-7, 8.765e-8), "adam_m": (1.3e-7, 1.331e-8), "adam_v": (2.2e-10, 2.242e-11),   # test_adam_matches_torch
           "e2e_params": (2.7e-7, 2.734e-8),                                                    # test_end_to_end_update
           # test_adam_late_and_unclipped: unclipped gradients of norm 2.3 -- the moments exceed test_adam_matches_torch's entries and get
           # their own (the parameters, measured 5.195e-7, stay under adam_params)
           "late_adam_m": (1.3e-6, 1.360e-7), "late_adam_v": (1.6e-8, 1.652e-9)}
# float32, rel(device) <= F32_FACTOR x rel(cpu32) per gradient segment: both are float32 with unit roundoff 2^-24 and differ in the
# order of their sums alone -- the device adds a k-ascending fma chain of up to 512 terms and 64 rows one after the other per tile,
# the CPU adds in blocks; 8 covers a random-walk growth of sqrt(512 / 8)
F32_FACTOR = 8.0
# float32, a case that exceeds an entry of F32_TOL gets an entry of its own here, by the same rule: case id -> {quantity: (tolerance, measured)}
F32_CASE_TOL = {"257x6-64_64-tanh-gau2-x8": {"grad": (4.8e-5, 4.881e-6)}}   # weights x 8: gradients of size 1.7, a norm of 10 (CPU float32: 5.1e-6)
# (label, segment) -> a factor of its own in place of F32_FACTOR, each with its evidence.  On the MI355X every segment of more than one
# element stayed within 4.6 x rel(cpu32) over all cases and tests; three segments of ONE element exceeded 8.  There rel(cpu32) is a
# single rounding error, which can lie far below half an ulp of the number, and no other order of the same float32 sums is held to
# that.  The evidence is the float32 reference's own per-row terms of the segment added in NumPy in the device's order (64 rows of a
# tile one after the other in float32, a workgroup's tiles in float32, the workgroups in float64, / W, rounded to float32):
#   16385x3 log_std   device 6.23e-7, restated order 5.41e-7, cpu32 4.88e-8; sum |terms| / |sum| = 10     ratio 12.8
#   16385x3 pi_b1     device 7.99e-8 = 0.9 ulp of the float32 result, restated order and cpu32 9.12e-9 = 0.1 ulp; cancellation 40   ratio 8.8
#   65x33 (100, 65) vf_b2   device 5.05e-7 = 4.8 ulp, restated order 1.90e-7, cpu32 2.01e-8 = 0.2 ulp; cancellation 22   ratio 25.2
# Each is the summation order meeting a lucky single draw of the yardstick, so each gets the next power of two above its ratio.
F32_SEGMENT_FACTOR = {("16385x3-4-tanh-gau1 f32", "log_std"): 16.0, ("16385x3-4-tanh-gau1 f32", "pi_b1"): 16.0,
                      ("65x33-100_65-relu-gau15 f32", "vf_b2"): 32.0}

# (m rows, obs_dim, hidden, activation, kind, act_dim, selection).  selection: None, or pairs (key, value) of
#   idx      k: the minibatch is k of the rows in permuted order, with uint8 weights of which about a third are zero
#   idx_all  k: the minibatch is a permutation of ALL rows followed by k rows named a second time (m + k > n_rows), the same weights
#   wscale   s: the weights' scale (test_gpu_actor._weights): 8 saturates tanh, so that 1 - y^2 cancels
# 65 / 257: a partial tile behind one / several full ones; 33 x (17, 128, 3): the two-pass width and partial output groups; 384:
# several K-slabs; 16 385 rows: 257 tiles in float32, 513 in float64 -- more than the fixed grid of 256, so a workgroup walks up to
# three tiles.  The last five put what only the 4-wide net did so far -- a workgroup's second tile, `first == false` -- behind every
# other path, and the reduce launch behind other grids (REGIME below says which case is there for which):
#   6529 x 512, 3 x 128, 16 actions   every limit at once; a slab of 8e5 bytes, so a grid below 256 whose workgroups walk a second
#                                     tile through four K-slabs of observations (eight in float64), hidden-to-hidden dW, the
#                                     transposed layer and a 16-entry log_std
#   16 485 of 16 385 x 33, (17, 128, 3), categorical 4   the same walk through three layers, the two-pass width, partial output groups
#                                     and the categorical head, rows gathered by idx
#   2305 x 6                          37 / 73 slabs: the reduce launch's 8-wide loads with a full chunk before a partial one
#   65 x 33, (100, 65), 15 actions    widths above 64 that are no multiple of 4, an odd act_dim
#   257 x 6, weights x 8              saturated tanh
# The many-row cases are tanh: no relu net keeps millions of pre-activations 1e-5 away from 0, and the relu branch does not depend on
# the tile count.
CASES = [(1, 1, (5,), "tanh", "gaussian", 1, None),
         (65, 33, (17, 128, 3), "relu", "gaussian", 5, None),
         (257, 384, (64, 64), "tanh", "gaussian", 10, None),
         (65, 6, (64, 64), "relu", "categorical", 4, None),
         (257, 6, (64, 64), "tanh", "categorical", 3, (("idx", 130),)),
         (16385, 3, (4,), "tanh", "gaussian", 1, None),
         (6529, 512, (128, 128, 128), "tanh", "gaussian", 16, None),
         (16385, 33, (17, 128, 3), "tanh", "categorical", 4, (("idx_all", 100),)),
         (2305, 6, (64, 64), "tanh", "categorical", 16, None),
         (65, 33, (100, 65), "relu", "gaussian", 15, None),
         (257, 6, (64, 64), "tanh", "gaussian", 2, (("wscale", 8.0),))]
N_OLD = 6                                                                      # the cases before the five above


def selection(case):
    return dict(case[6] or ())


def case_id(c):
    s = selection(c)
    return "%dx%d-%s-%s-%s%d%s%s%s" % (c[0], c[1], "_".join(map(str, c[2])), c[3], c[4][:3], c[5], "-idx" if "idx" in s else "",
                                       "-idxall" if "idx_all" in s else "", "-x%g" % s["wscale"] if "wscale" in s else "")


IDS = [case_id(c) for c in CASES]
# the data seed of each case, chosen on the CPU so that the assertions on the reference hold in both dtypes
SEEDS = dict(zip(IDS, [11, 12, 11, 13, 11, 11, 11, 11, 11, 12, 11]))


def tile_rows(dtype):
    return 32 if dtype == torch.float64 else 64


def n_tiles(m, dtype):
    return -(-m // tile_rows(dtype))


# case -> what (grid, tiles, dtype) must satisfy for the case to be in the regime it is named for: a later change of the grid rule
# cannot quietly void it
REGIME = {IDS[6]: lambda grid, tiles, f64: (grid, tiles) == ((42, 205) if f64 else (84, 103)) and grid < 256 and tiles > grid,
          IDS[7]: lambda grid, tiles, f64: grid == 256 and tiles >= 257,
          IDS[8]: lambda grid, tiles, f64: min(grid, tiles) == (73 if f64 else 37)}      # used; per = ceil(used / 4) = 19 / 10


def weights_dict(obs_dim, hidden, kind, n, dtype, wseed=1, scale=1.0):
    """{segment name: CPU tensor of `dtype`}: what Actor.load leaves on the device for the same seed"""
    pi, vf, ls = _weights(obs_dim, hidden, n, scale, wseed)
    w = {}
    for net, layers in (("pi", pi), ("vf", vf)):
        for l, (W, b) in enumerate(layers):
            w["%s_w%d" % (net, l)], w["%s_b%d" % (net, l)] = torch.as_tensor(W).to(dtype), torch.as_tensor(b).to(dtype)
    w["log_std"] = torch.as_tensor(ls).to(dtype) if kind == "gaussian" else torch.zeros(0, dtype=dtype)
    return w


def reference(w, hidden, activation, kind, dtype, rows, weight=None):
    """The references' answer on `rows` = (obs, act, logp_old, adv, ret), already gathered: (grads, stats, terms) of the float64
    reference, and for float32 data also the gradient of the float32 reference on the same numbers (else None)."""
    k = 0 if kind == "gaussian" else 1
    out = R.Ref(w, hidden, activation, k).grad(*rows, weight, CLIP, VF_COEF, ENT_COEF)
    g32 = None
    if dtype == torch.float32:
        threads = torch.get_num_threads()
        torch.set_num_threads(1)          # the blocks of torch's float32 sums, and with them rel(cpu32), follow the thread count: fix it
        try:
            g32 = R.Ref(w, hidden, activation, k, dtype=torch.float32).grad(*rows, weight, CLIP, VF_COEF, ENT_COEF)[0]
        finally:
            torch.set_num_threads(threads)
    return out + (g32,)


@functools.lru_cache(maxsize=None)
def case_data(case, dtype, seed):
    """The rows of a case (CPU tensors of `dtype`, the idx / weight selection included) and the references' answers: made once per
    case and dtype, shared by the tests, never modified."""
    m, obs_dim, hidden, activation, kind, n, _ = case
    sel = selection(case)
    rng = np.random.default_rng(seed)
    w = weights_dict(obs_dim, hidden, kind, n, dtype, scale=sel.get("wscale", 1.0))
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
    if "idx" in sel or "idx_all" in sel:
        if "idx" in sel:
            idx = rng.permutation(m)[:sel["idx"]].copy()
        else:
            idx = rng.permutation(m)
        weight = torch.as_tensor(rng.uniform(size=m) > 1.0 / 3.0).to(torch.uint8)
        if "idx_all" in sel:
            idx = np.concatenate([idx, rng.integers(0, m, sel["idx_all"])])
        idx = torch.as_tensor(idx).to(torch.int32)
    rows = idx.long() if idx is not None else slice(None)
    batch = (obs[rows], act[rows], logp_old[rows], adv[rows], ret[rows])
    wb = None if weight is None else weight[rows]
    grads, stats, terms, grads32 = reference(w, hidden, activation, kind, dtype, batch, wb)
    pre = ref.preactivations(obs[rows]) if activation == "relu" else []
    margin = dict(ratio=float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()),
                  relu=min([float(p.abs().min()) for p in pre] or [1.0]))
    on = slice(None) if wb is None else wb > 0
    # what f64_tol's factor 500 rests on, over the rows that count
    bound = dict(adv=float(adv[rows][on].abs().max()), ratio=float(terms["ratio"].max()),
                 z=float(terms["z"].abs().max()) if kind == "gaussian" else 0.0,
                 term=ref.row_term_max(*batch, wb, CLIP, VF_COEF, ENT_COEF))
    return dict(w=w, obs=obs, act=act, adv=adv, ret=ret, logp_old=logp_old, idx=idx, weight=weight, grads=grads, stats=stats, margin=margin,
                grads32=grads32, bound=bound, m=int(batch[0].shape[0]), chain=obs_dim + sum(hidden))


def check_reference(case, d):
    """what the data must exercise, asserted on the reference"""
    cf = d["stats"]["clip_frac"]
    assert (0.2 <= cf <= 0.8) if case[0] > 1 else cf in (0.0, 1.0), cf        # (one row: 0 or 1, there is nothing between)
    assert d["margin"]["ratio"] > 1e-4 and d["margin"]["relu"] > 1e-5, d["margin"]
    b = d["bound"]                                                            # f64_tol's docstring: e^0.5 = 1.6487...
    assert b["adv"] <= 4.5 and b["ratio"] <= 1.65 and b["z"] <= 10.0 and b["term"] <= 500.0, b


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


def rel(x, ref):
    """max |x - ref| / max |ref| over a segment: the error at the segment's OWN scale (err() has a floor of 1 under it, and every
    gradient segment here has max |ref| of 2e-4 .. 3e-2)"""
    ref = torch.as_tensor(ref).double().reshape(-1)
    return float((torch.as_tensor(x).double().cpu().reshape(-1) - ref).abs().max() / ref.abs().max())


def tol_of(dtype, key, m, chain=640, cid=None):
    return f64_tol(m, chain) if dtype == torch.float64 else F32_CASE_TOL.get(cid, F32_TOL).get(key, F32_TOL[key])[0]


def tag(dtype):
    return "f64" if dtype == torch.float64 else "f32"


def check_scale_aware(label, grads, want, want32, factor=F32_FACTOR):
    """float32, per non-empty segment: rel(device) <= factor x rel(cpu32), cpu32 the float32 reference on the same float32 data; a
    segment whose reference is identically zero must be exact zeros on the device (any dtype: want32 None skips the rest)."""
    rels = {}
    for k, g in want.items():
        if g.numel() == 0:
            continue
        if not bool(g.any()):
            assert not bool(grads[k].any()), k
            continue
        if want32 is not None:
            rels[k] = (rel(grads[k], g), rel(want32[k], g), g.numel())
    if not rels:
        return
    ratio = lambda k: rels[k][0] / rels[k][1] if rels[k][1] else float("inf")
    k = max(rels, key=ratio)
    print("learner float32 at the gradient's scale %s: worst segment %s (%d) rel(device) %.3e rel(cpu32) %.3e ratio %.2f; over the segments rel(device) <= %.3e rel(cpu32) <= %.3e"
          % (label, k, rels[k][2], rels[k][0], rels[k][1], ratio(k), max(r[0] for r in rels.values()), max(r[1] for r in rels.values())))
    bad = {k: rels[k] for k in rels if rels[k][0] > F32_SEGMENT_FACTOR.get((label, k), factor) * rels[k][1]}
    assert not bad, bad


def check_against(label, ln, dtype, m, want, want_stats, want32, chain=640):
    """the gradient and the statistics of the last grad() against the references': err() under the tolerances of the module docstring
    (a mean over m rows), and the float32 check at the gradient's own scale"""
    grads = ln.grads
    assert {k for k in grads if grads[k].numel()} == set(want)
    ge = {k: err(grads[k], g) for k, g in want.items()}
    dev_stats = ln.stats_dict()
    se = {k: abs(dev_stats[k] - v) / max(1.0, abs(v)) for k, v in want_stats.items()}
    print("learner errors %s %s: grad %.3e (%s) stats %.3e (%s)" % (label, tag(dtype), max(ge.values()), max(ge, key=ge.get),
                                                                   max(se.values()), max(se, key=se.get)))
    for k, e in ge.items():
        assert e <= tol_of(dtype, "grad", m, chain), (k, e)
    for k, e in se.items():
        assert e <= tol_of(dtype, "stats", m, chain), (k, e)
    check_scale_aware(label, grads, want, want32)
    return dev_stats


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_and_stats_match_reference(case, dtype):
    cid = IDS[CASES.index(case)]
    d = case_data(case, dtype, SEEDS[cid])
    check_reference(case, d)
    ln = make_learner(case, dtype, d)
    n_rows = d["m"]
    if cid in REGIME:
        assert REGIME[cid](ln.grid, n_tiles(n_rows, dtype), dtype == torch.float64), (ln.grid, n_tiles(n_rows, dtype))
    grads, stats = ln.grad(**dev_batch(d))
    assert grads is ln.grads and stats is ln.stats and {k for k in grads if grads[k].numel()} == set(d["grads"])
    ge = {k: err(grads[k], g) for k, g in d["grads"].items()}
    dev_stats = ln.stats_dict()
    se = {k: abs(dev_stats[k] - v) / max(1.0, abs(v)) for k, v in d["stats"].items()}
    print("learner errors %s %s: grad %.3e (%s) stats %.3e (%s)" % (cid, tag(dtype), max(ge.values()), max(ge, key=ge.get),
                                                                   max(se.values()), max(se, key=se.get)))
    chain = d["chain"] if CASES.index(case) >= N_OLD else 640                   # (the six first cases keep their value)
    for k, e in ge.items():
        assert e <= tol_of(dtype, "grad", n_rows, chain, cid), (k, e)
    for k, e in se.items():
        assert e <= tol_of(dtype, "stats", n_rows, chain, cid), (k, e)
    assert dev_stats["weight"] == d["stats"]["weight"]                      # W is a sum of small integers: exact
    assert int(ln.step_count[0]) == 0                                         # grad() alone takes no optimiser step
    check_scale_aware("%s %s" % (cid, tag(dtype)), grads, d["grads"], d["grads32"])


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


def small_rows(rng, m, obs_dim, kind, n, dtype):
    """(obs, act, adv, ret) of m rows, CPU tensors as the device will hold them"""
    t = lambda x: torch.as_tensor(x).to(dtype)
    act = t(rng.normal(0.0, 0.7, (m, n))) if kind == "gaussian" else torch.as_tensor(rng.integers(0, n, m)).to(torch.int32)
    return t(rng.uniform(-1.0, 1.0, (m, obs_dim))), act, t(rng.normal(size=m)), t(rng.normal(size=m))


def logp_of(w, hidden, kind, obs, act):
    with torch.no_grad():
        z = torch.zeros(obs.shape[0])
        return R.Ref(w, hidden, "tanh", 0 if kind == "gaussian" else 1).terms(obs, act, z, z, z, None, CLIP, VF_COEF, ENT_COEF)["logp"]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_single_rows_are_placed_right(kind, dtype):
    """Five live rows, each the only one of its tile, among 260 tiles and one row of dead ones (weight 0): row 0, the last row of tile 0,
    the first of tile 1, a middle row of tile 259 -- which workgroup 3 walks second -- and the last row, alone in tile 260, which
    workgroup 4 walks second.  obs_dim 70 is two K-slabs of observations in float32 and three in float64.  The reference runs on the
    five rows alone, so the gradient is a mean of five terms of one row's size: a row taken from the wrong tile, a stale slab or a
    wrong `first` is an error of order 1 at that scale, which f64_tol(5), F32_TOL and the float32 check at the gradient's scale all see.
    Then the same with real weights and with NaN in every dead row: the same bits."""
    TB, obs_dim, hidden, n = tile_rows(dtype), 70, (64, 64), 3
    m = 260 * TB + 1
    live = torch.tensor([0, TB - 1, TB, 259 * TB + TB // 2 - 3, m - 1])
    rng = np.random.default_rng(21)
    w = weights_dict(obs_dim, hidden, kind, n, dtype)
    obs, act, adv, ret = small_rows(rng, m, obs_dim, kind, n, dtype)
    # every live row in the unclipped branch (all five reach the policy's gradient), three of them outside the clip range
    adv[live] = torch.tensor([1.0, -1.2, 0.8, -0.6, 1.5]).to(dtype)
    logp_old = torch.as_tensor(rng.uniform(-1.5, -0.5, m)).to(dtype)
    logp_old[live] = (logp_of(w, hidden, kind, obs[live], act[live]) + torch.tensor([0.4, -0.4, 0.05, -0.05, 0.3])).to(dtype)
    rows = (obs[live], act[live], logp_old[live], adv[live], ret[live])
    grads, stats, terms, grads32 = reference(w, hidden, "tanh", kind, dtype, rows)
    assert stats["clip_frac"] == 0.6 and float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()) > 1e-2
    assert min(float(g.abs().max()) for g in grads.values()) > 1e-4                 # every segment has a gradient to get wrong
    case = (m, obs_dim, hidden, "tanh", kind, n, None)
    ln = make_learner(case, dtype, dict(w=w), batch=64)
    assert ln.grid == 256 and n_tiles(m, dtype) == 261                              # tiles 259 and 260 are second tiles
    weight = torch.zeros(m, dtype=torch.uint8)
    weight[live] = 1
    dev = [x.cuda() for x in (obs, act, logp_old, adv, ret)]
    weight = weight.cuda()
    ln.grad(*dev, weight=weight)
    dev_stats = check_against("single rows %s" % kind, ln, dtype, 5, grads, stats, grads32, chain=obs_dim + sum(hidden))
    assert dev_stats["weight"] == 5.0
    want = (ln.grad_buf.clone(), ln.stats.clone())
    ln.grad_buf.fill_(255)
    ln.grad(*dev, weight=weight.to(dtype))
    assert torch.equal(ln.grad_buf, want[0]) and torch.equal(ln.stats, want[1])
    dead = weight == 0
    for x in (dev[0], dev[2], dev[3], dev[4]):
        x[dead] = float("nan")
    for wt in (weight, weight.to(dtype)):
        ln.grad_buf.fill_(255)
        ln.grad(*dev, weight=wt)
        assert torch.equal(ln.grad_buf, want[0]) and torch.equal(ln.stats, want[1])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["gaussian", "categorical"])
def test_inactive_rows_by_every_rule(kind, dtype):
    """The row rules of include/beacon_learner.h in one minibatch of 257 entries over 257 rows: an idx at or past n_rows or below 0, a
    real weight of -1 or NaN, a class of -1 or act_dim, a row at or behind the cursor (value 3, 64 rows per step: s >= 192).  Every row
    that a rule of its own makes inactive holds NaN.  Against the reference on the surviving rows, and bit for bit the clean minibatch
    in which the inactive entries are named -1 in idx.  Then a cursor of 0 and below (nothing is live), fractional real weights, and
    a sum of weights below 1."""
    m, obs_dim, hidden, n = 257, 6, (64, 64), 3
    rng = np.random.default_rng(31)
    w = weights_dict(obs_dim, hidden, kind, n, dtype)
    obs, act, adv, ret = small_rows(rng, m, obs_dim, kind, n, dtype)
    pert = rng.choice([-1.0, 1.0], m) * rng.uniform(0.02, 0.45, m)
    pert = np.where(np.abs(np.abs(np.exp(-pert) - 1.0) - CLIP) < 2e-3, pert + 0.01, pert)
    logp_old = (logp_of(w, hidden, kind, obs, act) + torch.as_tensor(pert)).to(dtype)
    idx = torch.as_tensor(rng.permutation(m).copy()).to(torch.int32)
    past, below = [3, 70, 131, 256], [9, 64, 200]                              # positions in idx, in several tiles
    idx[past] = torch.tensor([m, m + 1, 1000, 2 ** 31 - 1], dtype=torch.int32)
    idx[below] = torch.tensor([-1, -7, -2 ** 31], dtype=torch.int32)
    src = rng.permutation(192)                                                 # source rows in front of the cursor, disjoint sets
    weight = torch.ones(m, dtype=dtype)
    weight[src[:8]] = -1.0
    weight[src[8:16]] = float("nan")
    bad_act = act.clone()
    if kind == "categorical":
        bad_act[src[16:24]] = -1
        bad_act[src[24:32]] = n
    cursor = torch.tensor([3, 0, 0, 0], dtype=torch.int32)
    s = idx.long()
    named = (s >= 0) & (s < m)
    sc = s.clamp(0, m - 1)
    alive = named & (sc < 192) & (weight[sc] > 0)
    if kind == "categorical":
        alive &= (bad_act[sc] >= 0) & (bad_act[sc] < n)
    n_alive = int(alive.sum())
    assert 120 < n_alive < 190 and int((named & (sc >= 192)).sum()) > 50, n_alive
    rows = s[alive]
    grads, stats, terms, grads32 = reference(w, hidden, "tanh", kind, dtype, (obs[rows], act[rows], logp_old[rows], adv[rows], ret[rows]))
    assert 0.2 <= stats["clip_frac"] <= 0.8 and float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()) > 1e-4
    case = (m, obs_dim, hidden, "tanh", kind, n, None)
    ln = make_learner(case, dtype, dict(w=w), lr=1e-3, max_grad_norm=0.5)
    c = lambda x: x.cuda()
    # the clean minibatch
    ln.grad(c(obs), c(act), c(logp_old), c(adv), c(ret), weight=None, idx=c(torch.where(alive, idx, torch.full_like(idx, -1))))
    dev_stats = check_against("row rules %s" % kind, ln, dtype, n_alive, grads, stats, grads32)
    assert dev_stats["weight"] == float(n_alive)
    want = (ln.grad_buf.clone(), ln.stats.clone())
    # every rule at once, NaN in the rows that a rule of their own makes inactive
    gone = ~(weight > 0) | (torch.arange(m) >= 192)
    if kind == "categorical":
        gone |= (bad_act < 0) | (bad_act >= n)
    assert int(gone.sum()) > 80 and not bool(gone[rows].any())
    nobs, nlogp, nadv, nret = obs.clone(), logp_old.clone(), adv.clone(), ret.clone()
    for x in (nobs, nlogp, nadv, nret):
        x[gone] = float("nan")
    dirty = (c(nobs), c(bad_act), c(nlogp), c(nadv), c(nret))
    ln.grad_buf.fill_(255)
    ln.grad(*dirty, weight=c(weight), idx=c(idx), _cursor=c(cursor), _rows_per_step=64)
    assert torch.equal(ln.grad_buf, want[0]) and torch.equal(ln.stats, want[1])
    # a cursor of 0, and below: nothing is live -- W reads 1, the gradient is +0 in every bit, a step moves no parameter
    for k, cur in enumerate((0, -2)):
        ln.grad_buf.fill_(255)
        before = ln.actor.params.clone()
        ln.grad(*dirty, weight=c(weight), idx=c(idx), _cursor=c(torch.tensor([cur, 0, 0, 0], dtype=torch.int32)), _rows_per_step=64)
        assert not bool(ln.grad_buf.any()) and bool(torch.isfinite(ln.stats).all()) and float(ln.stats[6]) == 1.0
        ln.step()
        assert torch.equal(ln.actor.params, before) and int(ln.step_count[0]) == k + 1
    # fractional real weights
    frac = torch.as_tensor(rng.uniform(0.0, 2.0, m)).to(dtype)
    assert float(frac.min()) > 0.0
    grads, stats, terms, grads32 = reference(w, hidden, "tanh", kind, dtype, (obs, act, logp_old, adv, ret), frac)
    ln.grad(c(obs), c(act), c(logp_old), c(adv), c(ret), weight=c(frac))
    check_against("fractional weights %s" % kind, ln, dtype, m, grads, stats, grads32)
    # a sum of weights below 1: W clamps to 1, the gradient is the weighted sum and not the mean
    tiny = torch.tensor([0.2, 0.3, 0.1]).to(dtype)
    three = (obs[:3], act[:3], logp_old[:3], adv[:3], ret[:3])
    grads, stats, terms, grads32 = reference(w, hidden, "tanh", kind, dtype, three, tiny)
    assert stats["weight"] == 1.0
    ln.grad(*[c(x.contiguous()) for x in three], weight=c(tiny))
    dev_stats = check_against("weights below one %s" % kind, ln, dtype, 3, grads, stats, grads32)
    assert dev_stats["weight"] == 1.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_update_partial_masked_rollout(dtype):
    """test_end_to_end_update on a rollout that is neither full nor fully valid: 5 of 8 steps recorded, two of them with replicas that
    a mask skips, NaN in adv and ret wherever a row is invalid or unrecorded, three minibatches of 21, 21 and 22 rows.  The reference
    standardises the advantages over the valid, recorded rows and runs the same minibatches on them."""
    import beacon_amd
    from beacon_amd import Actor, Learner
    T, B, n_rec, hidden, epochs, nmb, seed = 8, 8, 5, (16, 16), 2, 3, 1234
    env = beacon_amd.VecBurgers(B, dtype=tag(dtype), seed=5)
    actor = Actor(env, hidden=hidden, seed=21)
    pi, vf, ls = _weights(env.obs_dim, hidden, actor.act_dim, 1.0, 9)
    actor.load(pi, vf, ls)
    w0 = {k: v.detach().clone().cpu() for k, v in actor.weights.items()}
    ro = env.rollout(T)
    actor.attach(ro)
    env.reset()
    ro.begin()
    for _ in range(T):                                       # a full rollout first: the unrecorded steps of the next keep its rows,
        env.step_autoreset(actor.act())                      # valid = 1 included, so only the cursor makes them inactive
    ro.begin()
    skip = {1: [2, 5, 7], 3: [0, 5]}
    for t in range(n_rec):
        mask = None
        if t in skip:
            mask = torch.ones(B, dtype=torch.uint8, device="cuda")
            mask[skip[t]] = 0
        env.step_autoreset(actor.act(mask=mask), mask=mask)
    assert bool(ro.valid[n_rec:].all()) and int((ro.valid[:n_rec] == 0).sum()) == 5
    last_value = actor.values(env.obs)
    final_values = actor.values(ro.final_obs.reshape(T * B, env.obs_dim)).view(T, B)
    adv, ret = ro.compute_gae(actor.value_seq, last_value, final_values, gamma=0.99, lam=0.95)
    N = T * B
    live = (ro.valid.view(T, B) > 0) & (torch.arange(T, device="cuda").view(T, 1) < n_rec)
    adv[~live] = float("nan")
    ret[~live] = float("nan")
    hp = dict(lr=3e-4, clip_range=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF, max_grad_norm=0.5, betas=(0.9, 0.999), eps=1e-5)
    ln = Learner(actor, **hp)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ln.update(ro, adv, ret, epochs=epochs, minibatches=nmb, generator=gen)
    assert ro.check() == (n_rec, False)
    assert int(ln.step_count[0]) == epochs * nmb == 6
    assert bool(torch.isfinite(actor.params.view(dtype)).all()) and bool(torch.isfinite(ln.stats).all())

    cpu = lambda x: x.detach().double().cpu()
    obs, raw, logp_old = cpu(ro.obs[:-1]).reshape(N, -1), cpu(actor.raw_seq).reshape(N, -1), cpu(actor.logp_seq).reshape(N)
    a64, r64, on = cpu(adv).reshape(N), cpu(ret).reshape(N), live.reshape(N).cpu()
    n_live = int(on.sum())
    assert n_live == n_rec * B - 5 and N // 4 <= n_live <= 3 * N // 4             # a condition of the test, not a measurement
    a64 = (a64 - a64[on].mean()) / (a64[on].std() + 1e-8)
    ref = R.Ref(w0, hidden, "tanh", 0)
    opt = ref.adam(hp["lr"], hp["betas"], hp["eps"])
    gen2 = torch.Generator(device="cuda").manual_seed(seed)
    for _ in range(epochs):
        perm = torch.randperm(N, device="cuda", generator=gen2).cpu()
        for k in range(nmb):
            rows = perm[k * N // nmb:(k + 1) * N // nmb]
            rows = rows[on[rows]]                                                     # (autograd cannot be handed the NaN rows)
            assert rows.numel() >= 2
            _, _, terms = ref.grad(obs[rows], raw[rows], logp_old[rows], a64[rows], r64[rows], None, CLIP, VF_COEF, ENT_COEF)
            assert float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()) > 1e-4
            ref.clip_and_step(opt, hp["max_grad_norm"])
    worst = max(err(actor.weights[name], p.detach()) for name, p in ref.named)
    moved = max(float((p.detach() - w0[name].double().reshape(p.shape)).abs().max()) for name, p in ref.named)
    print("learner partial masked rollout %s: worst parameter error %.3e, the update moved a parameter by %.3e" % (tag(dtype), worst, moved))
    assert moved > 1e-4
    assert worst <= (epochs * nmb * hp["lr"] * f64_tol(N // nmb) / hp["eps"] if dtype == torch.float64 else F32_TOL["e2e_params"][0]), worst
    env.close()


LATE_CASE = CASES[9]                                                               # relu, segment sizes that are no multiples of 256


@functools.lru_cache(maxsize=None)
def late_reference(dtype, max_norm, steps=3, start=999):
    d = case_data(LATE_CASE, dtype, SEEDS[IDS[9]])
    ref = R.Ref(d["w"], LATE_CASE[2], LATE_CASE[3], 0)
    opt = ref.adam(ADAM["lr"], ADAM["betas"], ADAM["eps"], start_step=start)
    norms, margins = [], []
    for _ in range(steps):
        _, _, terms = ref.grad(d["obs"], d["act"], d["logp_old"], d["adv"], d["ret"], None, CLIP, VF_COEF, ENT_COEF)
        margins.append((float((terms["ratio"] - 1.0).abs().sub(CLIP).abs().min()), min(float(p.abs().min()) for p in ref.preactivations(d["obs"]))))
        norms.append(ref.clip_and_step(opt, max_norm))
    return d, ref, opt, norms, margins


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_adam_late_and_unclipped(dtype):
    """Three steps from a step counter of 999 (bias corrections of 1 - 0.9^1000 and 1 - 0.999^1000, zero moments) with max_grad_norm=None:
    parameters and moments against torch.optim.Adam without clip_grad_norm_; stats[7] is the norm nevertheless; the reference that
    clips at 0.5 -- below every step's norm -- is somewhere else."""
    steps = 3
    d, ref, opt, norms, margins = late_reference(dtype, 0.0)
    assert min(r for r, _ in margins) > 1e-4 and min(p for _, p in margins) > 1e-5 and min(norms) > 1.2 * 0.5, (margins, norms)
    ln = make_learner(LATE_CASE, dtype, d, max_grad_norm=None, **ADAM)
    assert ln.max_grad_norm == 0.0
    ln.step_count[0] = 999
    b = dev_batch(d)
    dev_norms = []
    for _ in range(steps):
        ln.grad(**b)
        ln.step()
        dev_norms.append(float(ln.stats[7]))
    assert int(ln.step_count[0]) == 999 + steps
    esz = 8 if dtype == torch.float64 else 4
    seg = lambda flat, s: flat[s["offset"] // esz:s["offset"] // esz + s["row_elems"]]

    def errors(ref, opt):
        m_ref, v_ref, step_ref = ref.moments(opt)
        assert step_ref == 999 + steps
        worst = {"adam_params": 0.0, "adam_m": 0.0, "adam_v": 0.0}
        for s in ln.grad_layout:
            name = s["name"]
            if s["row_elems"] == 0:
                continue
            worst["adam_params"] = max(worst["adam_params"], err(ln.actor.weights[name], dict(ref.named)[name].detach()))
            worst["adam_m"] = max(worst["adam_m"], err(seg(ln.m, s), m_ref[name]))
            worst["adam_v"] = max(worst["adam_v"], err(seg(ln.v, s), v_ref[name]))
        return worst

    worst = errors(ref, opt)
    print("learner late adam errors %s: %s; norms device %s reference %s" % (tag(dtype), " ".join("%s=%.3e" % kv for kv in sorted(worst.items())), dev_norms, norms))
    # float64, as in test_adam_matches_torch: m and v are linear / quadratic in the gradient (|g| <= 10), a parameter's step has a
    # sensitivity to the gradient of at most 1 / eps (the bias corrections at t = 1000 only lower it: (1 - beta1) / (1 - beta1^t) <= 1)
    t64 = f64_tol(65)
    tol = {"adam_params": steps * ADAM["lr"] * t64 / ADAM["eps"], "adam_m": t64, "adam_v": 20.0 * t64}
    if dtype == torch.float32:
        tol = {"adam_params": F32_TOL["adam_params"][0], "adam_m": F32_TOL["late_adam_m"][0], "adam_v": F32_TOL["late_adam_v"][0]}
    for k, e in worst.items():
        assert e <= tol[k], (k, e)
    for dn, rn in zip(dev_norms, norms):                                            # the norm is reported although nothing is clipped
        assert abs(dn - rn) / max(1.0, rn) <= tol_of(dtype, "stats", 65)
    clipped = errors(*late_reference(dtype, 0.5)[1:3])
    assert clipped["adam_m"] > 1e3 * tol["adam_m"] and clipped["adam_v"] > 1e3 * tol["adam_v"], clipped
