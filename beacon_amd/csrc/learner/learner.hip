// learner.hip -- the C ABI of libbeacon_learner.so (include/beacon_learner.h): argument checks, the three layouts, the two calls, and
// the float32 instantiation of the kernels (learner_impl.h).  The float64 instantiation is learner_f64.hip, built without FMA
// contraction.
//
// The library links nothing of libbeacon_actor.so: the actor's cfg rules and its parameter layout (include/beacon_actor.h states
// both) are restated here, and tests/test_learner_host.py holds the two libraries against each other, refusal for refusal and
// segment for segment.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "learner_impl.h"

static thread_local char g_learner_err[512] = "";

static void learner_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_learner_err, sizeof(g_learner_err), fmt, ap);
  va_end(ap);
}

extern "C" BCN_LEARNER_API const char* bcn_learner_last_error(void) { return g_learner_err; }

LEARNER_DEFINE_LAUNCH(float)

// ---- cfg and layouts ---------------------------------------------------------------------
static bool learner_cfg_ok(const bcn_actor_cfg* c) {
  if (!c) { learner_set_error("cfg is NULL"); return false; }
  if (c->obs_dim < 1 || c->obs_dim > BCN_ACTOR_MAX_OBS) { learner_set_error("cfg.obs_dim = %d: must lie in 1 .. %d", c->obs_dim, BCN_ACTOR_MAX_OBS); return false; }
  if (c->dtype != 0 && c->dtype != 1) { learner_set_error("cfg.dtype = %d: must be 0 (float32) or 1 (float64)", c->dtype); return false; }
  if (c->n_hidden < 1 || c->n_hidden > BCN_ACTOR_MAX_LAYERS) { learner_set_error("cfg.n_hidden = %d: must lie in 1 .. %d", c->n_hidden, BCN_ACTOR_MAX_LAYERS); return false; }
  for (int l = 0; l < c->n_hidden; l++)
    if (c->hidden[l] < 1 || c->hidden[l] > BCN_ACTOR_MAX_HIDDEN) {
      learner_set_error("cfg.hidden[%d] = %d: must lie in 1 .. %d", l, c->hidden[l], BCN_ACTOR_MAX_HIDDEN);
      return false;
    }
  if (c->activation != BCN_ACTOR_TANH && c->activation != BCN_ACTOR_RELU) { learner_set_error("cfg.activation = %d: must be 0 (tanh) or 1 (relu)", c->activation); return false; }
  if (c->kind != BCN_ACTOR_GAUSSIAN && c->kind != BCN_ACTOR_CATEGORICAL) { learner_set_error("cfg.kind = %d: must be 0 (Gaussian) or 1 (categorical)", c->kind); return false; }
  const int lo = c->kind == BCN_ACTOR_GAUSSIAN ? 1 : 2;
  if (c->act_dim < lo || c->act_dim > BCN_ACTOR_MAX_ACT) { learner_set_error("cfg.act_dim = %d: must lie in %d .. %d for this kind", c->act_dim, lo, BCN_ACTOR_MAX_ACT); return false; }
  if (c->kind == BCN_ACTOR_GAUSSIAN && !(c->low <= c->high)) { learner_set_error("cfg.low = %g, cfg.high = %g: need low <= high", c->low, c->high); return false; }
  return true;
}

static size_t learner_up16(size_t x) { return (x + 15) & ~(size_t)15; }
static size_t learner_esz(const bcn_actor_cfg* c) { return c->dtype ? 8 : 4; }

static void learner_seg(bcn_actor_seg* segs, int max_segs, int k, const char* name, size_t off, int elem, size_t row_elems) {
  if (!segs || k >= max_segs) return;
  memset(&segs[k], 0, sizeof(segs[k]));
  strncpy(segs[k].name, name, sizeof(segs[k].name) - 1);
  segs[k].offset = off; segs[k].elem = elem; segs[k].planes = 0; segs[k].row_elems = (int64_t)row_elems;
}

// the parameter layout of include/beacon_actor.h; returns the segment count, the bytes in *bytes
static int learner_params_lay(const bcn_actor_cfg* c, bcn_actor_seg* segs, int max_segs, size_t* bytes) {
  const size_t esz = learner_esz(c);
  size_t off = 0;
  int k = 0;
  char name[16];
  for (int net = 0; net < 2; net++) {
    size_t in = (size_t)c->obs_dim;
    for (int l = 0; l <= c->n_hidden; l++) {
      const size_t out = l < c->n_hidden ? (size_t)c->hidden[l] : (net == 0 ? (size_t)c->act_dim : 1);
      snprintf(name, sizeof(name), "%s_w%d", net ? "vf" : "pi", l);
      off = learner_up16(off); learner_seg(segs, max_segs, k++, name, off, BCN_ACTOR_REAL, out * in); off += out * in * esz;
      snprintf(name, sizeof(name), "%s_b%d", net ? "vf" : "pi", l);
      off = learner_up16(off); learner_seg(segs, max_segs, k++, name, off, BCN_ACTOR_REAL, out); off += out * esz;
      in = out;
    }
  }
  const size_t nls = c->kind == BCN_ACTOR_GAUSSIAN ? (size_t)c->act_dim : 0;
  off = learner_up16(off); learner_seg(segs, max_segs, k++, "log_std", off, BCN_ACTOR_REAL, nls); off += nls * esz;
  *bytes = learner_up16(off);
  return k;
}

static size_t learner_n_elems(const bcn_actor_cfg* c) {
  size_t bytes;
  learner_params_lay(c, nullptr, 0, &bytes);
  return bytes / learner_esz(c);
}

static int learner_grid(const bcn_actor_cfg* c) {
  const size_t slab = learner_n_elems(c) * learner_esz(c);
  size_t g = ((size_t)64 << 20) / slab;
  g = g < 8 ? 8 : g;
  return (int)(g > BCN_LEARNER_MAX_GRID ? BCN_LEARNER_MAX_GRID : g);
}

static int learner_red_blocks(const bcn_actor_cfg* c) { return (int)((learner_n_elems(c) + LEARNER_RED_PARAMS - 1) / LEARNER_RED_PARAMS); }

static int learner_opt_lay(const bcn_actor_cfg* c, bcn_actor_seg* segs, int max_segs, size_t* bytes) {
  const size_t ne = learner_n_elems(c), esz = learner_esz(c);
  size_t off = 0;
  learner_seg(segs, max_segs, 0, "m", off, BCN_ACTOR_REAL, ne); off = learner_up16(off + ne * esz);
  learner_seg(segs, max_segs, 1, "v", off, BCN_ACTOR_REAL, ne); off = learner_up16(off + ne * esz);
  learner_seg(segs, max_segs, 2, "step", off, BCN_ACTOR_I32, 4); off = learner_up16(off + 16);
  *bytes = off;
  return 3;
}

static int learner_work_lay(const bcn_actor_cfg* c, bcn_actor_seg* segs, int max_segs, size_t* bytes) {
  const size_t ne = learner_n_elems(c), esz = learner_esz(c), grid = (size_t)learner_grid(c), nb = (size_t)learner_red_blocks(c);
  size_t off = 0;
  learner_seg(segs, max_segs, 0, "stats", off, BCN_LEARNER_F64, BCN_LEARNER_N_STATS); off = learner_up16(off + 8 * BCN_LEARNER_N_STATS);
  learner_seg(segs, max_segs, 1, "wg_stats", off, BCN_LEARNER_F64, grid * BCN_LEARNER_N_STATS); off = learner_up16(off + 8 * grid * BCN_LEARNER_N_STATS);
  learner_seg(segs, max_segs, 2, "norm2", off, BCN_LEARNER_F64, nb); off = learner_up16(off + 8 * nb);
  learner_seg(segs, max_segs, 3, "slabs", off, BCN_ACTOR_REAL, grid * ne); off = learner_up16(off + grid * ne * esz);
  *bytes = off;
  return 4;
}

extern "C" {

BCN_LEARNER_API int bcn_learner_grad_layout(const bcn_actor_cfg* cfg, bcn_actor_seg* segs, int max_segs) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  return learner_params_lay(cfg, segs, max_segs, &bytes);
}

BCN_LEARNER_API size_t bcn_learner_grad_bytes(const bcn_actor_cfg* cfg) {
  if (!learner_cfg_ok(cfg)) return 0;
  size_t bytes;
  learner_params_lay(cfg, nullptr, 0, &bytes);
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
  if (!(ptr)) { learner_set_error(fn ": " name " is NULL"); return BCN_LEARNER_ERR_ARG; }

template <typename real>
static int learner_grad_t(const bcn_actor_cfg* c, const void* params, const bcn_learner_batch* b, const bcn_learner_loss* loss, void* grad,
                          void* work, void* stream) {
  constexpr int TB = ActorGeom<real>::TB;
  LearnerArgs<real> a;
  memset(&a, 0, sizeof(a));
  a.params = static_cast<const real*>(params);
  a.obs = static_cast<const real*>(b->obs_dev);
  a.act = b->act_dev;
  a.logp_old = static_cast<const real*>(b->logp_old_dev);
  a.adv = static_cast<const real*>(b->adv_dev);
  a.ret = static_cast<const real*>(b->ret_dev);
  a.weight = b->weight_dev; a.weight_kind = b->weight_kind;
  a.idx = b->idx_dev; a.cursor = b->cursor_dev; a.rows_per_step = b->rows_per_step;
  a.n_rows = (long long)b->n_rows; a.m = (long long)b->m;
  a.tiles = (a.m + TB - 1) / TB;
  a.obs_dim = c->obs_dim; a.n_hidden = c->n_hidden; a.activation = c->activation; a.kind = c->kind; a.act_dim = c->act_dim;
  int hmax = 0;
  for (int l = 0; l < c->n_hidden; l++) { a.hidden[l] = c->hidden[l]; hmax = c->hidden[l] > hmax ? c->hidden[l] : hmax; }
  a.hmax_pad = hmax;
  const int omax = hmax > c->act_dim ? hmax : c->act_dim;
  a.wcols = ((omax + 3) & ~3) + 4;
  bcn_actor_seg s[BCN_ACTOR_MAX_SEGS];
  size_t bytes;
  const int ns = learner_params_lay(c, s, BCN_ACTOR_MAX_SEGS, &bytes);
  const int per = 2 * (c->n_hidden + 1);
  for (int l = 0; l <= c->n_hidden; l++) {
    a.pi.w[l] = (unsigned)(s[2 * l].offset / sizeof(real));       a.pi.b[l] = (unsigned)(s[2 * l + 1].offset / sizeof(real));
    a.vf.w[l] = (unsigned)(s[per + 2 * l].offset / sizeof(real)); a.vf.b[l] = (unsigned)(s[per + 2 * l + 1].offset / sizeof(real));
  }
  a.log_std = (unsigned)(s[ns - 1].offset / sizeof(real));
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
  if (e) { learner_set_error("bcn_learner_grad: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_LEARNER_ERR_HIP; }
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
  const int e = learner_launch_step<real>(a, step, stream);
  if (e) { learner_set_error("bcn_learner_step: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_LEARNER_ERR_HIP; }
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
    learner_set_error("bcn_learner_grad: batch.weight_kind = %d: must be 0 (none), 1 (uint8) or 2 (real)", b->weight_kind);
    return BCN_LEARNER_ERR_ARG;
  }
  if (b->weight_kind != BCN_LEARNER_W_NONE && !b->weight_dev) {
    learner_set_error("bcn_learner_grad: batch.weight_dev is NULL with weight_kind = %d", b->weight_kind);
    return BCN_LEARNER_ERR_ARG;
  }
  if (b->m < 1 || b->m > 0x7fffffffll) { learner_set_error("bcn_learner_grad: batch.m = %lld: must lie in 1 .. 2^31 - 1", (long long)b->m); return BCN_LEARNER_ERR_ARG; }
  if (b->n_rows < 1 || b->n_rows > 0x7fffffffll) { learner_set_error("bcn_learner_grad: batch.n_rows = %lld: must lie in 1 .. 2^31 - 1", (long long)b->n_rows); return BCN_LEARNER_ERR_ARG; }
  if (!b->idx_dev && b->m > b->n_rows) {
    learner_set_error("bcn_learner_grad: batch.m = %lld exceeds batch.n_rows = %lld without idx_dev", (long long)b->m, (long long)b->n_rows);
    return BCN_LEARNER_ERR_ARG;
  }
  if (b->cursor_dev && b->rows_per_step < 1) { learner_set_error("bcn_learner_grad: batch.rows_per_step = %d: a cursor needs >= 1", b->rows_per_step); return BCN_LEARNER_ERR_ARG; }
  if (!(loss->clip >= 0.0)) { learner_set_error("bcn_learner_grad: loss.clip = %g: must be >= 0", loss->clip); return BCN_LEARNER_ERR_ARG; }
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
  if (!(adam->beta1 >= 0.0 && adam->beta1 < 1.0)) { learner_set_error("bcn_learner_step: adam.beta1 = %g: must lie in [0, 1)", adam->beta1); return BCN_LEARNER_ERR_ARG; }
  if (!(adam->beta2 >= 0.0 && adam->beta2 < 1.0)) { learner_set_error("bcn_learner_step: adam.beta2 = %g: must lie in [0, 1)", adam->beta2); return BCN_LEARNER_ERR_ARG; }
  return cfg->dtype ? learner_step_t<double>(cfg, params_dev, grad_dev, opt_dev, work_dev, adam, stream)
                    : learner_step_t<float>(cfg, params_dev, grad_dev, opt_dev, work_dev, adam, stream);
}

}  // extern "C"
