// learner.hip -- the C ABI of libbeacon_learner.so (include/beacon_learner.h): argument checks, the three layouts, the two calls, and
// the float32 instantiation of the kernels (learner_impl.h).  The float64 instantiation is learner_f64.hip, built without FMA
// contraction.
//
// The library links nothing of libbeacon_actor.so.  The actor's cfg rules, its parameter layout (the gradient's) and the network's
// part of the argument block are the routines of ../actor/policy_net.h, which both libraries compile.
#include "learner_impl.h"

static thread_local PolicyErr g_learner_err;

extern "C" BCN_LEARNER_API const char* bcn_learner_last_error(void) { return g_learner_err.text; }

LEARNER_DEFINE_LAUNCH(float)

// ---- cfg and layouts ---------------------------------------------------------------------
static bool learner_cfg_ok(const bcn_actor_cfg* c) { return policy_cfg_ok(c, false, &g_learner_err); }

static size_t learner_n_elems(const bcn_actor_cfg* c) {
  size_t bytes;
  policy_params_lay(c, nullptr, 0, &bytes);
  return bytes / policy_esz(c);
}

static int learner_grid(const bcn_actor_cfg* c) {
  const size_t slab = learner_n_elems(c) * policy_esz(c);
  size_t g = ((size_t)64 << 20) / slab;
  g = g < 8 ? 8 : g;
  return (int)(g > BCN_LEARNER_MAX_GRID ? BCN_LEARNER_MAX_GRID : g);
}

static int learner_red_blocks(const bcn_actor_cfg* c) { return (int)((learner_n_elems(c) + LEARNER_RED_PARAMS - 1) / LEARNER_RED_PARAMS); }

static int learner_opt_lay(const bcn_actor_cfg* c, bcn_actor_seg* segs, int max_segs, size_t* bytes) {
  const size_t ne = learner_n_elems(c);
  const PolicySegDesc d[3] = {{"m", BCN_ACTOR_REAL, 0, ne}, {"v", BCN_ACTOR_REAL, 0, ne}, {"step", BCN_ACTOR_I32, 0, 4}};
  *bytes = policy_lay(d, 3, 1, policy_esz(c), segs, max_segs);
  return 3;
}

static int learner_work_lay(const bcn_actor_cfg* c, bcn_actor_seg* segs, int max_segs, size_t* bytes) {
  const size_t ne = learner_n_elems(c), grid = (size_t)learner_grid(c), nb = (size_t)learner_red_blocks(c);
  const PolicySegDesc d[4] = {{"stats", BCN_LEARNER_F64, 0, BCN_LEARNER_N_STATS}, {"wg_stats", BCN_LEARNER_F64, 0, grid * BCN_LEARNER_N_STATS},
                              {"norm2", BCN_LEARNER_F64, 0, nb}, {"slabs", BCN_ACTOR_REAL, 0, grid * ne}};
  *bytes = policy_lay(d, 4, 1, policy_esz(c), segs, max_segs);
  return 4;
}

extern "C" {

BCN_LEARNER_API int bcn_learner_grad_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  return policy_params_lay(cfg, segs, max_segs, &bytes);
}

BCN_LEARNER_API size_t bcn_learner_grad_bytes(const bcn_actor_cfg* cfg) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  policy_params_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}

BCN_LEARNER_API int bcn_learner_opt_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  return learner_opt_lay(cfg, segs, max_segs, &bytes);
}

BCN_LEARNER_API size_t bcn_learner_opt_bytes(const bcn_actor_cfg* cfg) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  learner_opt_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}

BCN_LEARNER_API int bcn_learner_work_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  return learner_work_lay(cfg, segs, max_segs, &bytes);
}

BCN_LEARNER_API size_t bcn_learner_work_bytes(const bcn_actor_cfg* cfg) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  learner_work_lay(cfg, nullptr, 0, &bytes);
  return bytes;
}

BCN_LEARNER_API int bcn_learner_grid(const bcn_actor_cfg* cfg) {
  if (!learner_cfg_ok(cfg)) return 0;
  return learner_grid(cfg);
}

}  // extern "C"

// ---- the calls ---------------------------------------------------------------------------
#define LEARNER_NEED(ptr, fn, name) \
  if (!(ptr)) { g_learner_err.set(fn ": " name " is NULL"); return BCN_LEARNER_ERR_ARG; }

template <typename real>
static int learner_grad_t(const bcn_actor_cfg* c, const void* params, const bcn_learner_batch* b, const bcn_learner_loss* loss, void* grad,
                          void* work, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  LearnerArgs<real> a;
  memset(&a, 0, sizeof(a));
  policy_fill_net<real>(c, params, &a);
  a.obs = static_cast<const real*>(b->obs_dev);
  a.act = b->act_dev;
  a.logp_old = static_cast<const real*>(b->logp_old_dev);
  a.adv = static_cast<const real*>(b->adv_dev);
  a.ret = static_cast<const real*>(b->ret_dev);
  a.weight = b->weight_dev; a.weight_kind = b->weight_kind;
  a.idx = b->idx_dev; a.cursor = b->cursor_dev; a.rows_per_step = b->rows_per_step;
  a.rows_per_weight = b->rows_per_weight > 1 ? b->rows_per_weight : 1;
  a.n_rows = (long long)b->n_rows; a.m = (long long)b->m;
  a.tiles = (a.m + TB - 1) / TB;
  bcn_actor_seg s[BCN_ACTOR_MAX_SEGS];
  size_t bytes;
  const int ns = policy_params_lay(c, s, BCN_ACTOR_MAX_SEGS, &bytes);
  a.clip = (real)loss->clip; a.vf_coef = (real)loss->vf_coef; a.ent_coef = (real)loss->ent_coef;

  bcn_actor_seg ws[4];
  learner_work_lay(c, ws, 4, &bytes);
  char* wk = static_cast<char*>(work);
  const size_t ne = learner_n_elems(c);
  a.slabs = reinterpret_cast<real*>(wk + ws[3].offset);
  a.slab_elems = ne;
  a.wg_stats = reinterpret_cast<double*>(wk + ws[1].offset);
  const int grid_max = learner_grid(c);
  const int grid = a.tiles < grid_max ? (int)a.tiles : grid_max;

  LearnerReduceArgs<real> r;
  memset(&r, 0, sizeof(r));
  r.slabs = a.slabs; r.slab_elems = ne; r.used = grid; r.wg_stats = a.wg_stats;
  r.grad = static_cast<real*>(grad);
  r.n_elems = (int)ne;
  r.n_segs = ns;
  for (int k = 0; k < ns; k++) {
    r.seg_begin[k] = (int)(s[k].offset / sizeof(real));
    r.seg_end[k] = r.seg_begin[k] + (int)s[k].row_elems;
  }
  r.norm2 = reinterpret_cast<double*>(wk + ws[2].offset);
  r.stats = reinterpret_cast<double*>(wk + ws[0].offset);
  r.vf_coef = (double)a.vf_coef; r.ent_coef = (double)a.ent_coef;
  const int e = learner_launch_grad<real>(a, r, grid, learner_red_blocks(c), stream);
  if (e) { g_learner_err.set("bcn_learner_grad: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_LEARNER_ERR_HIP; }
  return BCN_LEARNER_OK;
}

template <typename real>
static int learner_step_t(const bcn_actor_cfg* c, void* params, const void* grad, void* opt, const void* work, const bcn_learner_adam* h,
                          void* stream) {
  bcn_actor_seg s[4];
  size_t bytes;
  learner_opt_lay(c, s, 4, &bytes);
  char* ob = static_cast<char*>(opt);
  LearnerAdamArgs<real> a;
  memset(&a, 0, sizeof(a));
  a.params = static_cast<real*>(params);
  a.grad = static_cast<const real*>(grad);
  a.m = reinterpret_cast<real*>(ob + s[0].offset);
  a.v = reinterpret_cast<real*>(ob + s[1].offset);
  int32_t* step = reinterpret_cast<int32_t*>(ob + s[2].offset);
  a.step = step;
  learner_work_lay(c, s, 4, &bytes);
  a.stats = reinterpret_cast<const double*>(static_cast<const char*>(work) + s[0].offset);
  a.n_elems = (int)learner_n_elems(c);
  a.lr = h->lr; a.beta1 = h->beta1; a.beta2 = h->beta2; a.eps = h->eps; a.max_grad_norm = h->max_grad_norm;
  a.target_kl = h->target_kl; a.lr_end = h->lr_end; a.lr_steps = h->lr_steps;
  const int e = learner_launch_step<real>(a, step, stream);
  if (e) { g_learner_err.set("bcn_learner_step: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_LEARNER_ERR_HIP; }
  return BCN_LEARNER_OK;
}

extern "C" {

BCN_LEARNER_API int bcn_learner_grad(const bcn_actor_cfg* cfg, const void* params_dev, const bcn_learner_batch* b, const bcn_learner_loss* loss,
                                     void* grad_dev, void* work_dev, void* stream) {
  if (!learner_cfg_ok(cfg)) return BCN_LEARNER_ERR_ARG;
  LEARNER_NEED(params_dev, "bcn_learner_grad", "params_dev")
  LEARNER_NEED(b, "bcn_learner_grad", "batch")
  LEARNER_NEED(loss, "bcn_learner_grad", "loss")
  LEARNER_NEED(grad_dev, "bcn_learner_grad", "grad_dev")
  LEARNER_NEED(work_dev, "bcn_learner_grad", "work_dev")
  LEARNER_NEED(b->obs_dev, "bcn_learner_grad", "batch.obs_dev")
  LEARNER_NEED(b->act_dev, "bcn_learner_grad", "batch.act_dev")
  LEARNER_NEED(b->logp_old_dev, "bcn_learner_grad", "batch.logp_old_dev")
  LEARNER_NEED(b->adv_dev, "bcn_learner_grad", "batch.adv_dev")
  LEARNER_NEED(b->ret_dev, "bcn_learner_grad", "batch.ret_dev")
  if (b->weight_kind < BCN_LEARNER_W_NONE || b->weight_kind > BCN_LEARNER_W_REAL) {
    g_learner_err.set("bcn_learner_grad: batch.weight_kind = %d: must be 0 (none), 1 (uint8) or 2 (real)", b->weight_kind);
    return BCN_LEARNER_ERR_ARG;
  }
  if (b->weight_kind != BCN_LEARNER_W_NONE && !b->weight_dev) {
    g_learner_err.set("bcn_learner_grad: batch.weight_dev is NULL with weight_kind = %d", b->weight_kind);
    return BCN_LEARNER_ERR_ARG;
  }
  if (b->m < 1 || b->m > 0x7fffffffll) { g_learner_err.set("bcn_learner_grad: batch.m = %lld: must lie in 1 .. 2^31 - 1", (long long)b->m); return BCN_LEARNER_ERR_ARG; }
  if (b->n_rows < 1 || b->n_rows > 0x7fffffffll) { g_learner_err.set("bcn_learner_grad: batch.n_rows = %lld: must lie in 1 .. 2^31 - 1", (long long)b->n_rows); return BCN_LEARNER_ERR_ARG; }
  if (!b->idx_dev && b->m > b->n_rows) {
    g_learner_err.set("bcn_learner_grad: batch.m = %lld exceeds batch.n_rows = %lld without idx_dev", (long long)b->m, (long long)b->n_rows);
    return BCN_LEARNER_ERR_ARG;
  }
  if (b->cursor_dev && b->rows_per_step < 1) { g_learner_err.set("bcn_learner_grad: batch.rows_per_step = %d: a cursor needs >= 1", b->rows_per_step); return BCN_LEARNER_ERR_ARG; }
  if (b->rows_per_weight < 0) { g_learner_err.set("bcn_learner_grad: batch.rows_per_weight = %d: must be >= 0 (0 means 1)", b->rows_per_weight); return BCN_LEARNER_ERR_ARG; }
  if (b->rows_per_weight > 1 && b->n_rows % b->rows_per_weight != 0) {
    g_learner_err.set("bcn_learner_grad: batch.rows_per_weight = %d does not divide batch.n_rows = %lld", b->rows_per_weight, (long long)b->n_rows);
    return BCN_LEARNER_ERR_ARG;
  }
  if (!(loss->clip >= 0.0)) { g_learner_err.set("bcn_learner_grad: loss.clip = %g: must be >= 0", loss->clip); return BCN_LEARNER_ERR_ARG; }
  return cfg->dtype ? learner_grad_t<double>(cfg, params_dev, b, loss, grad_dev, work_dev, stream)
                    : learner_grad_t<float>(cfg, params_dev, b, loss, grad_dev, work_dev, stream);
}

BCN_LEARNER_API int bcn_learner_step(const bcn_actor_cfg* cfg, void* params_dev, const void* grad_dev, void* opt_dev, const void* work_dev,
                                     const bcn_learner_adam* adam, void* stream) {
  if (!learner_cfg_ok(cfg)) return BCN_LEARNER_ERR_ARG;
  LEARNER_NEED(params_dev, "bcn_learner_step", "params_dev")
  LEARNER_NEED(grad_dev, "bcn_learner_step", "grad_dev")
  LEARNER_NEED(opt_dev, "bcn_learner_step", "opt_dev")
  LEARNER_NEED(work_dev, "bcn_learner_step", "work_dev")
  LEARNER_NEED(adam, "bcn_learner_step", "adam")
  if (!(adam->target_kl - adam->target_kl == 0.0)) { g_learner_err.set("bcn_learner_step: adam.target_kl = %g: must be finite (<= 0: no stop rule)", adam->target_kl); return BCN_LEARNER_ERR_ARG; }
  if (!(adam->lr_end - adam->lr_end == 0.0)) { g_learner_err.set("bcn_learner_step: adam.lr_end = %g: must be finite", adam->lr_end); return BCN_LEARNER_ERR_ARG; }
  if (!(adam->lr_steps - adam->lr_steps == 0.0)) { g_learner_err.set("bcn_learner_step: adam.lr_steps = %g: must be finite (<= 0: no schedule)", adam->lr_steps); return BCN_LEARNER_ERR_ARG; }
  if (!(adam->beta1 >= 0.0 && adam->beta1 < 1.0)) { g_learner_err.set("bcn_learner_step: adam.beta1 = %g: must lie in [0, 1)", adam->beta1); return BCN_LEARNER_ERR_ARG; }
  if (!(adam->beta2 >= 0.0 && adam->beta2 < 1.0)) { g_learner_err.set("bcn_learner_step: adam.beta2 = %g: must lie in [0, 1)", adam->beta2); return BCN_LEARNER_ERR_ARG; }
  return cfg->dtype ? learner_step_t<double>(cfg, params_dev, grad_dev, opt_dev, work_dev, adam, stream)
                    : learner_step_t<float>(cfg, params_dev, grad_dev, opt_dev, work_dev, adam, stream);
}

}  // extern "C"
