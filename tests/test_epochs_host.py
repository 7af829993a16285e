"""CPU-side checks of the host-free PPO update (no GPU): the header, the binding and the library of libbeacon_epochs.so agree and the
other three libraries' symbol sets are untouched; tests/epochs_ref.py's permutation is a bijection whose walks end, and uniform where
a minibatch shuffle has to be; every refusal of the new entry points with its code and a message naming the field; the fields
appended to bcn_learner_adam; Learner's and Plan's argument errors on a bare env; the DPP wait-state scan of the new library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import epochs_ref as E
import isa_hazards as H
import noise_ref as P
from test_actor_host import NAMES as ACTOR_NAMES, _bare, _cfg
from test_learner_host import NAMES as LEARNER_NAMES

NAMES = {"bcn_epochs_work_layout", "bcn_epochs_work_bytes", "bcn_epochs_permute", "bcn_epochs_begin", "bcn_epochs_last_error"}
SEEDS = (0, 7, 0xDEADBEEFCAFEF00D)
EPOCHS = (0, 1, 1 << 31)


def _lib():
    from beacon_amd import build, epochs
    if build.hipcc() is None and not os.path.exists(epochs.LIB):
        pytest.skip("no hipcc and no prebuilt library")
    return epochs.load()


def _exported(lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("bcn_")}


def test_header_binding_and_library_agree():
    from beacon_amd import _lib as main, actor, build, epochs, learner
    hdr = open(os.path.join(ROOT, "include", "beacon_epochs.h")).read()
    declared = set(re.findall(r"BCN_EPOCHS_API\s+[\w\s\*]+?\b(bcn_epochs_\w+)\s*\(", hdr))
    assert declared == NAMES == set(epochs.SIGNATURES)
    assert int(re.search(r"#define BCN_EPOCHS_API_VERSION (\d+)", hdr).group(1)) == epochs.API_VERSION == 1
    for macro, value in (("GRID", epochs.GRID), ("CHUNK", epochs.CHUNK), ("ROUNDS", epochs.ROUNDS), ("MAX_SEGS", epochs.MAX_SEGS)):
        assert int(re.search(r"#define BCN_EPOCHS_%s (\d+)" % macro, hdr).group(1)) == value, macro
    assert epochs.ROUNDS == E.ROUNDS and len(epochs.MOMENTS) == 4
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name)
    assert _exported(epochs.LIB) == NAMES
    # the structs the binding passes are the header's, field for field
    for struct, cls in (("bcn_epochs_seg", epochs.EpochsSeg), ("bcn_epochs_batch", epochs.EpochsBatch)):
        body = re.search(r"typedef struct \{([^{}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
        fields = [re.sub(r"\[\d+\]$", "", f) for f in fields]
        assert [f[:-4] if f.endswith("_dev") else f for f in fields] == [f[0] for f in cls._fields_], struct
    # the other three libraries export what they exported: the new entry points are in none of their tables
    actor.load(), learner.load(), main.load()
    assert _exported(actor.LIB) == ACTOR_NAMES == set(actor.SIGNATURES)
    assert _exported(learner.LIB) == LEARNER_NAMES == set(learner.SIGNATURES)
    assert not any("epochs" in n for n in _exported(build.LIB)) and not any("epochs" in n for n in main.SIGNATURES)
    main_hdr = open(os.path.join(ROOT, "include", "beacon_hip.h")).read()
    assert len(re.findall(r"BCN_API\s+[\w\s\*]+?\b(bcn_\w+)\s*\(", main_hdr)) == 78
    for other in ("beacon_hip.h", "beacon_actor.h", "beacon_learner.h"):
        assert "BCN_EPOCHS_API" not in open(os.path.join(ROOT, "include", other)).read()
    # a unit of its own, on the one build machinery; the Philox definition it shares is among what its .sig hashes
    assert epochs._UNIT.__class__ is learner._UNIT.__class__
    assert [os.path.basename(s) for s in epochs.sources()] == sorted(epochs.FILE_FLAGS) == ["epochs.hip"]
    deps = {os.path.basename(f) for f in epochs._UNIT.deps()}
    assert {"epochs.hip", "beacon_epochs.h", "env1d.h"} <= deps and not deps & {"beacon_actor.h", "beacon_learner.h", "policy_net.h"}
    assert not any("epochs" in os.path.basename(s) for s in build.sources() + actor.sources() + learner.sources())
    import beacon_amd
    assert beacon_amd.Plan is epochs.Plan and "plan" in beacon_amd.__doc__
    segs, nbytes = epochs.work_layout()
    assert [(s["name"], s["elem"], s["planes"], s["row_elems"]) for s in segs] == [("moments", 3, 0, 4), ("part", 3, 0, 2 * epochs.GRID),
                                                                                  ("part2", 3, 0, epochs.GRID)]
    end = 0
    for s in segs:
        assert s["offset"] % 16 == 0 and s["offset"] >= end
        end = s["offset"] + 8 * s["row_elems"]
    assert nbytes >= end and nbytes % 16 == 0


def test_the_round_tables_are_the_headers_round_function():
    """epochs_ref evaluates F(r, h) once per value of the half it reads; here f is computed with Philox called per element, as the
    header writes it, over a whole domain with unequal halves"""
    n, seed, epoch = 257, 0xDEADBEEFCAFEF00D, 5
    k, hl, hr = E.geometry(n)
    assert (k, hl, hr) == (9, 4, 5) and E.geometry(1) == (2, 1, 1) and E.geometry(2) == (2, 1, 1) and E.geometry(5) == (3, 1, 2)
    assert E.geometry((1 << 31) - 1) == (31, 15, 16) and E.geometry(4097) == (13, 6, 7) and E.geometry(4096) == (12, 6, 6)
    x = np.arange(1 << k, dtype=np.uint64)
    k0, k1 = P._key(seed)
    L, R = x >> np.uint64(hr), x & np.uint64((1 << hr) - 1)
    for r in range(6):
        if r % 2 == 0:
            L = L ^ (P.philox4x32_10(R, epoch, r, 3, k0, k1)[0] & np.uint64((1 << hl) - 1))
        else:
            R = R ^ (P.philox4x32_10(L, epoch, r, 3, k0, k1)[0] & np.uint64((1 << hr) - 1))
    f = (L << np.uint64(hr)) | R
    assert np.array_equal(f, E.feistel(x, n, seed, epoch))
    assert np.array_equal(np.sort(f), x)                          # f is a bijection of the whole domain
    assert not np.array_equal(E.feistel(x, n, seed, epoch + 1), f) and not np.array_equal(E.feistel(x, n, seed + 1, epoch), f)


def test_permutation_is_a_bijection_and_every_walk_ends():
    """every n in 1 .. 1029 and the sizes around 2^12, 2^16 and 2^20, over three seeds and three epochs: a permutation of 0 .. n - 1,
    every walk within 2^k applications (permutation() asserts it; the longest is reported), the domain below 2 n from n = 3 on"""
    longest, at = 0, None
    for n in list(range(1, 1030)) + [4095, 4096, 4097, 65537, (1 << 20) + 1]:
        k = E.geometry(n)[0]
        assert (1 << k) >= n and (n < 3 or (1 << k) < 2 * n), n
        for seed in SEEDS:
            for epoch in EPOCHS:
                idx, walk = E.permutation(n, seed, epoch, walks=True)
                assert idx.shape == (n,) and np.array_equal(np.bincount(idx, minlength=n), np.ones(n, dtype=np.int64)), (n, seed, epoch)
                assert walk <= 1 << k
                if walk > longest:
                    longest, at = walk, (n, seed, epoch)
    print("epochs permutation: longest walk %d applications at (n, seed, epoch) = %s" % (longest, at))
    # a pure function of its three arguments, and each of them matters
    a = E.permutation(257, 7, 1)
    assert np.array_equal(a, E.permutation(257, 7, 1))
    assert not np.array_equal(a, E.permutation(257, 7, 2)) and not np.array_equal(a, E.permutation(257, 8, 1))
    assert not np.array_equal(a, E.permutation(257, 7 + (1 << 32), 1))                 # the seed's high word is in the key
    assert np.array_equal(E.permutation(257, 7, 1 << 32), E.permutation(257, 7, 0))    # the epoch is a 32-bit word


def test_minibatches_are_uniform():
    """n = 257 rows in 4 minibatches over the epochs 0 .. 2047 under seed 12345: which minibatch a row falls into, and how often
    neighbouring rows share one, against the uniform shuffle's expectation; both standardised statistics below 4 in absolute value"""
    n, nmb, epochs, seed = 257, 4, 2048, 12345
    bounds = [k * n // nmb for k in range(nmb + 1)]
    size = np.diff(bounds).astype(np.float64)
    mb_of_pos = np.repeat(np.arange(nmb), np.diff(bounds))
    counts = np.zeros((n, nmb))
    together = 0
    for e in range(epochs):
        idx = E.permutation(n, seed, e)
        mb = np.empty(n, dtype=np.int64)
        mb[idx] = mb_of_pos                                  # position p holds row idx[p]: row idx[p] is in minibatch mb_of_pos[p]
        counts[np.arange(n), mb] += 1
        together += int((mb[:-1] == mb[1:]).sum())
    want = epochs * size / n
    chi = float(((counts - want) ** 2 / want).sum())
    dof = (n - 1) * (nmb - 1)
    z_chi = (chi - dof) / np.sqrt(2.0 * dof)
    p = float((size * (size - 1)).sum() / (n * (n - 1)))
    trials = epochs * (n - 1)
    z_pair = (together - trials * p) / np.sqrt(trials * p * (1.0 - p))
    print("epochs minibatch uniformity: chi-square %.1f at %d dof, z %.2f; neighbours together %d of %d (p %.4f), z %.2f"
          % (chi, dof, z_chi, together, trials, p, z_pair))
    assert abs(z_chi) < 4.0 and abs(z_pair) < 4.0, (z_chi, z_pair)


def test_every_refusal_has_its_code_and_names_the_field():
    from beacon_amd import epochs
    L = _lib()
    err = lambda: L.bcn_epochs_last_error().decode()
    p = C.c_void_p(64)                 # non-NULL dummies, never dereferenced: every check comes before a device is touched
    q = C.c_void_p(128)
    for n, word in ((0, "n = 0"), (-5, "n = -5"), (1 << 31, "n = 2147483648")):
        assert L.bcn_epochs_permute(n, 7, p, p, None) == 1 and word in err(), err()
    assert L.bcn_epochs_permute(8, 7, None, p, None) == 1 and "epoch_dev is NULL" in err()
    assert L.bcn_epochs_permute(8, 7, p, None, None) == 1 and "idx_dev is NULL" in err()

    def batch(**kw):
        b = dict(adv=p, adv_out=q, weight=None, cursor=None, step=p, work=p, n_rows=8, dtype=0, normalize=1, weight_kind=0, rows_per_step=0,
                 rows_per_weight=0)
        b.update(kw)
        return epochs.EpochsBatch(**b)
    assert L.bcn_epochs_begin(None, None) == 1 and "batch is NULL" in err()
    for kw, word in ((dict(normalize=0, step=None), "step_dev"), (dict(dtype=2), "batch.dtype"), (dict(dtype=-1), "batch.dtype"),
                     (dict(adv=None), "batch.adv_dev"), (dict(adv_out=None), "batch.adv_out_dev"), (dict(adv_out=p), "aliases"),
                     (dict(work=None), "batch.work_dev"), (dict(n_rows=0), "batch.n_rows"), (dict(n_rows=1 << 31), "batch.n_rows"),
                     (dict(weight_kind=3), "batch.weight_kind"), (dict(weight_kind=-1), "batch.weight_kind"),
                     (dict(weight_kind=1), "batch.weight_dev"), (dict(weight_kind=2), "batch.weight_dev"),
                     (dict(cursor=p, rows_per_step=0), "batch.rows_per_step"), (dict(rows_per_weight=-1), "batch.rows_per_weight"),
                     (dict(rows_per_weight=3), "batch.rows_per_weight")):
        assert L.bcn_epochs_begin(C.byref(batch(**kw)), None) == 1 and word in err(), (kw, err())


def test_the_appended_adam_fields():
    """bcn_learner_adam's three appended doubles: zeros pass their checks (the refusal that follows is of a field behind them),
    a target_kl, lr_end or lr_steps that is not finite is refused by name.  No call here gets as far as a launch."""
    from beacon_amd import learner
    L = learner.load()
    err = lambda: L.bcn_learner_last_error().decode()
    p = C.c_void_p(64)
    cfg = _cfg()
    assert [f[0] for f in learner.LearnerAdam._fields_] == ["lr", "beta1", "beta2", "eps", "max_grad_norm", "target_kl", "lr_end", "lr_steps"]
    assert C.sizeof(learner.LearnerAdam) == 64
    step = lambda **kw: L.bcn_learner_step(C.byref(cfg), p, p, p, p, C.byref(learner.LearnerAdam(**dict(dict(lr=1e-3, beta1=1.0, beta2=0.999, eps=1e-8,
                                                                                                    max_grad_norm=0.5), **kw))), None)
    assert step() == 1 and "adam.beta1" in err()                                              # zeros (left out) are accepted
    assert step(target_kl=0.0, lr_end=0.0, lr_steps=0.0) == 1 and "adam.beta1" in err()
    assert step(target_kl=0.01, lr_end=1e-5, lr_steps=100.0) == 1 and "adam.beta1" in err()
    assert step(target_kl=-1.0, lr_steps=-1.0) == 1 and "adam.beta1" in err()                 # <= 0 means none, not an error
    for field in ("target_kl", "lr_end", "lr_steps"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert step(**{field: bad}) == 1 and "adam." + field in err(), (field, bad, err())


def test_argument_errors_need_no_gpu():
    from beacon_amd import Actor, Learner, Plan
    _lib()
    env = _bare("VecBurgers")
    a = Actor(env, hidden=(5, 7), seed=3)
    for kw, word in ((dict(target_kl=-0.01), "target_kl"), (dict(target_kl="low"), "target_kl"), (dict(target_kl=float("nan")), "target_kl"),
                     (dict(target_kl=float("inf")), "target_kl"), (dict(lr_end=-1e-4), "lr_end"), (dict(lr_end=float("inf")), "lr_end"),
                     (dict(lr_end=None), "lr_end"), (dict(lr_steps=-1), "lr_steps"), (dict(lr_steps="many"), "lr_steps")):
        with pytest.raises(ValueError, match=word):
            Learner(a, **kw)
        with pytest.raises(ValueError, match=word):
            Learner(a).set_hyper(**kw)
    ln = Learner(a)
    assert (ln.target_kl, ln.lr_end, ln.lr_steps) == (0.0, 0.0, 0.0)
    ln.set_hyper(target_kl=0.02, lr_end=1e-5, lr_steps=500)
    assert (ln.target_kl, ln.lr_end, ln.lr_steps) == (0.02, 1e-5, 500.0)
    assert ln.set_hyper(target_kl=None).target_kl == 0.0
    with pytest.raises(ValueError, match="lr_steps"):
        ln.set_hyper(target_kl=0.5, lr_steps=-2)
    assert ln.target_kl == 0.0                                   # nothing is set when one of them is refused
    ln.set_hyper(target_kl=0.03)
    d = ln.state_dict()
    assert (d["target_kl"], d["lr_end"], d["lr_steps"]) == (0.03, 1e-5, 500.0)
    other = Learner(a).load_state_dict(d)
    assert (other.target_kl, other.lr_end, other.lr_steps) == (0.03, 1e-5, 500.0)
    old = {k: v for k, v in d.items() if k not in ("target_kl", "lr_end", "lr_steps")}     # a state from before the fields
    other = Learner(a, target_kl=0.5).load_state_dict(old)
    assert (other.target_kl, other.lr_end, other.lr_steps) == (0.0, 0.0, 0.0) and other.lr == ln.lr
    assert ln.skipped == 0 and ln.step_count.tolist() == [0, 0, 0, 0]
    # the plan's arguments, before the rollout is looked at and before any launch
    for kw, word in ((dict(epochs=0), "epochs"), (dict(epochs=2.5), "epochs"), (dict(epochs=True), "epochs"), (dict(minibatches=0), "minibatches"),
                     (dict(minibatches="four"), "minibatches"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(seed=1.5), "seed"),
                     (dict(normalize_adv=1), "normalize_adv"), (dict(normalize_adv=None), "normalize_adv")):
        with pytest.raises(ValueError, match=word):
            ln.plan(object(), **kw)
    with pytest.raises(ValueError, match="attached"):
        ln.plan(object())
    with pytest.raises(ValueError, match="attached"):
        ln.plan(None)
    with pytest.raises(ValueError, match="Learner"):
        Plan(a, object())


def test_the_gpu_cases_have_data_that_exercises_them():
    """the references of tests/test_gpu_epochs.py, without a GPU: the KL case stops at the third of six pairs with every pair's
    approx_kl a relative 1e-3 or more from the threshold; the schedule's five steps keep their margins from the clip boundaries; the
    standardisation cases have the active and inactive rows they are named for and a float64 tolerance below 1e-9"""
    import test_gpu_epochs as T
    for dtype in (torch.float64, torch.float32):
        T.check_kl_reference(dtype)
        T.check_lr_reference(dtype)
        for name, (n, _, rpw, steps) in T.STD_CASES.items():
            d = T.std_data(name, dtype)
            assert d["on"].sum() == d["count"] > 0 and np.isnan(d["adv"].numpy()[~d["on"]]).all() and np.isfinite(d["ref"]).all()
            assert n % rpw == 0 and (steps is None or n % steps[0] == 0)
            T.std_tol(d, dtype)
    d = T.std_data("69993-u8-cursor-rpw3", torch.float32)
    assert d["rps"] == 3333 and d["cursor"] * d["rps"] == 66660 and not d["on"][66660:].any() and d["on"][65536:66660].any()
    assert 0.25 < float((d["weight"] == 0).double().mean()) < 0.42 and d["weight"].numel() == 69993 // 3
    d = T.std_data("70001-real", torch.float64)
    assert bool(torch.isnan(d["weight"]).any()) and not d["on"][torch.isnan(d["weight"]).numpy()].any()


def test_epochs_unit_compiles_for_gfx950_without_dpp_hazards():
    from beacon_amd import build, epochs
    tool = H.objdump()
    if tool is None or (build.hipcc() is None and not os.path.exists(epochs.LIB)):
        pytest.skip("no llvm-objdump / no hipcc and no prebuilt library")
    assert "-ffp-contract=off" in epochs.FILE_FLAGS["epochs.hip"]
    lib = epochs.build_epochs()
    assert not epochs.stale()
    rep = H.scan_file(lib, tool)
    H.summarise(rep)
    assert rep["code_objects"] >= 1 and not rep["findings"], rep["findings"]
    for f in os.listdir(epochs.SRC_DIR):                          # no inline assembly in the new unit
        assert "asm" not in re.sub(r"//.*", "", open(os.path.join(epochs.SRC_DIR, f)).read()), f
