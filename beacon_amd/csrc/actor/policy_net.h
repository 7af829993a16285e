// policy_net.h -- the policy / value network of include/beacon_actor.h, stated once for the two libraries that run it:
// libbeacon_actor.so (actor_impl.h, actor.hip) and libbeacon_learner.so (../learner/learner_impl.h, learner.hip).  Both include this
// file; neither links anything of the other.  Device side: the tile geometry, staging into LDS, one layer on a tile, the walk over
// an MLP's layers, the head's log-density terms.  Host side, at the end: the cfg rules, the segment and parameter layouts, the
// network's part of a kernel's argument block, the dynamic-LDS limit.  The log-probability the actor stores and the one the learner
// recomputes for the same row are the same routines here, so the first epoch's PPO ratio is exp(0).
//
// A site uses a routine of this file only if the device code of all four units stays what it was with the text written out in place
// (scripts/params_fast_kernels.py --compare; the rules of ns2d_cells.h; DESIGN.md 26 has the table of piece x site).
//
// A workgroup of 256 lanes owns a tile of TB rows (64 in float32, 32 in float64) and runs the MLPs on it one after the other, layer by
// layer.  Activations live in LDS k-major, h[k][row] with TBP = TB + 4 columns, so that the four consecutive rows of a lane are one
// 16-byte read (float32) and the outputs of a layer are written as such rows.  A layer's weights are staged per slab of KS reduction
// steps, transposed to w[k][out]: the largest matrix, 128 x 512 float32, is 256 KB and never fits the 160 KB LDS as a whole, a slab
// of it is 33 KB.  The first layer's input is staged the same way from the observation rows in HBM.
//
// Each lane keeps a register tile of (4 NPASS) rows x 4 outputs: lane = og * nrg + rg with nog = the power of two >= ceil(out / 4)
// output groups and nrg = 256 / nog row groups (NPASS = 2 when nog = 32, i.e. out > 64: the tile's rows in two halves).  Per k a lane
// reads one 16-byte weight chunk (shared by the nrg lanes of its output group: a broadcast) and one row chunk per pass (consecutive
// lanes read consecutive chunks: conflict-free), 2 reads for 16 fma.  Plain fma, not the float32 MFMA: the matrix rate equals the
// vector rate on gfx950 and both are exact fma chains, so MFMA would only save LDS reads -- and its 32x32 / 16x16 output blocks would
// leave 3/4 of the lanes' work on padding at the widths an RL policy has (a head of 1 .. 16 outputs, obs_dim 6) while the k-ordered
// chain per output that the header promises (and bcn_actor_values repeats bit for bit) falls out of the plain form for every shape.
//
// Rows of a partial tile are staged as zeros and never stored; columns of a partial slab are not looped over: nothing is read
// past a row or past the batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../../include/beacon_actor.h"

#define ACTOR_NT 256

template <typename real> struct ActorGeom;
template <> struct ActorGeom<float> { static constexpr int TB = 64, KS = 64; };
template <> struct ActorGeom<double> { static constexpr int TB = 32, KS = 32; };

// four consecutive reals of an LDS row, 16-byte aligned: one ds_read_b128 (float32) or two (float64)
template <typename real> struct alignas(16) ActorV4 { real v[4]; };

struct ActorNet {
  // element offsets into the parameter buffer: layers 0 .. n_hidden - 1 and the head (index n_hidden)
  unsigned w[BCN_ACTOR_MAX_LAYERS + 1], b[BCN_ACTOR_MAX_LAYERS + 1];
};

__device__ __forceinline__ float actor_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double actor_tanh(double x) { return tanh(x); }
__device__ __forceinline__ float actor_exp(float x) { return expf(x); }
__device__ __forceinline__ double actor_exp(double x) { return exp(x); }
__device__ __forceinline__ float actor_log(float x) { return logf(x); }
__device__ __forceinline__ double actor_log(double x) { return log(x); }
__device__ __forceinline__ float actor_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double actor_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float actor_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double actor_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float actor_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double actor_abs(double x) { return fabs(x); }

// ---- staging ---------------------------------------------------------------------------------------------------------------
// Stage ks columns (from k0 on) of `rows` rows of the row-major matrix src[.][K] into LDS transposed, dst[k * ld + row].
//   GATHER = false  the first `rows` rows of src, zeros for the rows from `valid` up to `rows`
//   GATHER = true   row r is row rowsrc[r] of src, or zeros for rowsrc[r] < 0 (the learner: behind m, weight 0)
// The global loads of ACTOR_STAGE_U elements per lane are issued before the first LDS store, so one round trip to memory covers all
// of them (issued one by one, the round trips of a slab added up to most of a launch).
#define ACTOR_STAGE_U 8
template <typename real, bool GATHER>
__device__ __forceinline__ void actor_stage(const real* __restrict__ src, int K, int k0, int ks, int rows, int valid, const int* rowsrc,
                                            real* dst, int ld) {
  const int total = rows * ks;
  for (int e0 = threadIdx.x; e0 < total; e0 += ACTOR_NT * ACTOR_STAGE_U) {
    real v[ACTOR_STAGE_U];
    int at[ACTOR_STAGE_U];
#pragma unroll
    for (int u = 0; u < ACTOR_STAGE_U; u++) {
      const int e = e0 + u * ACTOR_NT;
      const int r = e / ks, k = e - r * ks;
      if constexpr (GATHER) {
        const int s = e < total ? rowsrc[r] : -1;
        at[u] = e < total ? k * ld + r : -1;
        v[u] = s >= 0 ? src[(size_t)s * K + k0 + k] : real(0);
      } else {
        at[u] = e < total ? k * ld + r : -1;
        v[u] = (e < total && r < valid) ? src[(size_t)r * K + k0 + k] : real(0);
      }
    }
#pragma unroll
    for (int u = 0; u < ACTOR_STAGE_U; u++)
      if (at[u] >= 0) dst[at[u]] = v[u];
  }
}

// qs rows (from q0 on) of the row-major matrix W[.][N] into LDS as they are, dst[q * ld + n], n < n4 (zeros behind N)
template <typename real>
__device__ __forceinline__ void actor_stage_rows(const real* __restrict__ W, int N, int n4, int q0, int qs, real* dst, int ld) {
  const int total = qs * n4;
  for (int e = threadIdx.x; e < total; e += ACTOR_NT) {
    const int q = e / n4, n = e - q * n4;
    dst[q * ld + n] = n < N ? W[(size_t)(q0 + q) * N + n] : real(0);
  }
}

// ---- one layer ---------------------------------------------------------------------------------------------------------------
// One layer on the workgroup's tile, out[n][r] for n < N, r < TB, a sum over R steps q in ascending order:
//   TR = false  out[n][r] = f(bias[n] + sum_q W[n][q] in[q][r]), W [N][R]: the forward pass
//   TR = true   out[n][r] = (sum_q W[q][n] in[q][r]) f'(out[n][r]), W [R][N], no bias (nullptr): the gradient at the layer's input, in
//               place over its output -- the same product with the weight rows copied straight instead of transposed
//   xin         the input k-major in LDS (row stride TBP; must not alias out), or nullptr: rows of `obs`, staged per slab into xs --
//               GATHER = false: the rows from `row0` on, up to n_rows; GATHER = true: the rows rowsrc[0 .. TB) names
//   f           0 tanh, 1 relu, 2 identity; with TR the derivative of 0 / 1 from the layer's output: 1 - y^2, [y > 0]
template <typename real, bool TR, bool GATHER>
__device__ __forceinline__ void policy_layer(const real* __restrict__ W, const real* __restrict__ bias, int R, int N, int f, const real* xin,
                                             const real* __restrict__ obs, long long row0, long long n_rows, const int* rowsrc, real* xs,
                                             real* ws, int wcols, real* out) {
  constexpr int TB = ActorGeom<real>::TB, KS = ActorGeom<real>::KS, TBP = TB + 4;
  constexpr int NPASS = 2;
  const int lane = threadIdx.x;
  const int n4 = (N + 3) & ~3;
  int nog = 1;
  while (nog * 4 < n4) nog <<= 1;                   // <= 32: N <= 128
  const int nrg = ACTOR_NT / nog;
  const int og = lane / nrg, rg = lane - og * nrg;
  const int o0 = og * 4;
  const bool has_out = o0 < n4;

  real acc[NPASS][4][4];                            // [pass][row][output]
#pragma unroll
  for (int j = 0; j < 4; j++) {
    // the gathered forms test the pointer at run time: deriving the test from TR changed both learner units
    const real bj = ((!GATHER || bias != nullptr) && has_out && o0 + j < N) ? bias[o0 + j] : real(0);
#pragma unroll
    for (int p = 0; p < NPASS; p++)
#pragma unroll
      for (int i = 0; i < 4; i++) acc[p][i][j] = bj;
  }
  const int r_a = rg * 4, r_b = (nrg + rg) * 4;     // first row of pass 0 / pass 1
  const bool act_a = has_out && r_a < TB, act_b = has_out && r_b < TB;

  for (int q0 = 0; q0 < R; q0 += KS) {
    const int qs = min(KS, R - q0);
    __syncthreads();                                // the previous slab's (or layer's, or phase's) readers of ws / xs are done, its writers too
    // weights: W[o][q0 + q] -> ws[q][o], o < n4 (zeros behind N); consecutive lanes read consecutive q of one row
    if constexpr (TR) actor_stage_rows<real>(W, N, n4, q0, qs, ws, wcols);
    else actor_stage<real, false>(W, R, q0, qs, n4, N, nullptr, ws, wcols);
    if (xin == nullptr) {
      if constexpr (GATHER) actor_stage<real, true>(obs, R, q0, qs, TB, 0, rowsrc, xs, TBP);
      else actor_stage<real, false>(obs + (size_t)row0 * R, R, q0, qs, TB, (int)min((long long)TB, n_rows - row0), nullptr, xs, TBP);
    }
    __syncthreads();
    const real* x = xin ? xin + (size_t)q0 * TBP : xs;
    if (act_a) {
#pragma unroll 4
      for (int q = 0; q < qs; q++) {               // four steps' LDS reads are in flight before the first fma needs one
        const ActorV4<real> wq = *reinterpret_cast<const ActorV4<real>*>(ws + q * wcols + o0);
        const ActorV4<real> xq = *reinterpret_cast<const ActorV4<real>*>(x + q * TBP + r_a);
        const real* wv = wq.v;
        const real* xa = xq.v;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) acc[0][i][j] = actor_fma(wv[j], xa[i], acc[0][i][j]);
        if (act_b) {
          const ActorV4<real> xr = *reinterpret_cast<const ActorV4<real>*>(x + q * TBP + r_b);
          const real* xb = xr.v;
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[1][i][j] = actor_fma(wv[j], xb[i], acc[1][i][j]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < NPASS; p++) {
    const int r0 = p ? r_b : r_a;
    if (!(p ? act_b : act_a)) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (o0 + j >= N) continue;
      ActorV4<real>* at = reinterpret_cast<ActorV4<real>*>(out + (o0 + j) * TBP + r0);
      ActorV4<real> q, y;
      if constexpr (TR) y = *at;                    // this lane's own entries: nobody else reads or writes them in this phase
#pragma unroll
      for (int i = 0; i < 4; i++) {
        real v = acc[p][i][j];
        if constexpr (TR) {
          if (f == 0) v = v * (real(1) - y.v[i] * y.v[i]);
          else if (f == 1) v = y.v[i] > real(0) ? v : real(0);
        } else {
          if (f == 0) v = actor_tanh(v);
          else if (f == 1) v = v > real(0) ? v : real(0);
        }
        q.v[i] = v;
      }
      *at = q;
    }
  }
}

// One MLP on the tile: the forward pass over A's layers (A: the kernel's argument block, policy_fill_net's fields and obs, n_rows).
// Layer l's output goes to out_of(l) (LDS, [hidden[l]][TBP]; not layer l - 1's), the head's outputs land in `head` ([n_head][TBP]).
template <typename real, bool GATHER, typename Args, typename OutOf>
__device__ __forceinline__ void policy_mlp(const Args& A, const ActorNet& net, int n_head, long long row0, const int* rowsrc, OutOf out_of,
                                           real* xs, real* ws, real* head) {
  const real* in = nullptr;
  int K = A.obs_dim;
  for (int l = 0; l < A.n_hidden; l++) {
    real* o = out_of(l);
    policy_layer<real, false, GATHER>(A.params + net.w[l], A.params + net.b[l], K, A.hidden[l], A.activation, in, A.obs, row0, A.n_rows, rowsrc,
                                      xs, ws, A.wcols, o);
    in = o;
    K = A.hidden[l];
  }
  policy_layer<real, false, GATHER>(A.params + net.w[A.n_hidden], A.params + net.b[A.n_hidden], K, n_head, 2, in, A.obs, row0, A.n_rows, rowsrc,
                                    xs, ws, A.wcols, head);
}

// ---- the head's distribution (include/beacon_actor.h) ---------------------------------------------------------------------------
// Gaussian: one dimension's term of log p at the standardised draw z, log_std ls
template <typename real>
__device__ __forceinline__ real policy_gauss_logp(real z, real ls) {
  return (real(-0.5) * z * z - ls) - real(0.91893853320467274178);
}

// Categorical: mx, the largest of the n logits h[0 .. n), and lse, the log of the sum of exp(h - mx) over them; log p_i is the
// caller's (h[i] - mx) - lse.  A macro that leaves mx, se and lse in the caller's scope: as a routine that returns the pair, and as
// two routines that return a value each, it changed both actor kernels.
#define POLICY_LOG_SUM_EXP(h, n)                                  \
  real mx = h[0];                                                 \
  _Pragma("unroll") for (int i = 1; i < BCN_ACTOR_MAX_ACT; i++)   \
    if (i < n && h[i] > mx) mx = h[i];                            \
  real se = real(0);                                              \
  _Pragma("unroll") for (int i = 0; i < BCN_ACTOR_MAX_ACT; i++)   \
    if (i < n) se += actor_exp(h[i] - mx);                        \
  const real lse = actor_log(se);

// ---- host: cfg rules, layouts, the argument block, the LDS limit -------------------------------------------------------------------
// a library's last error: each library has ONE thread-local object of this type behind its bcn_*_last_error
struct PolicyErr {
  char text[512] = "";
  __attribute__((format(printf, 2, 3))) void set(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
  }
};

// the rules of bcn_actor_cfg; need_batch: with cfg.batch (the calls that size or touch per-replica buffers)
inline bool policy_cfg_ok(const bcn_actor_cfg* c, bool need_batch, PolicyErr* err) {
  if (!c) { err->set("cfg is NULL"); return false; }
  if (need_batch && c->batch < 1) { err->set("cfg.batch = %d: must be >= 1", c->batch); return false; }
  if (c->obs_dim < 1 || c->obs_dim > BCN_ACTOR_MAX_OBS) { err->set("cfg.obs_dim = %d: must lie in 1 .. %d", c->obs_dim, BCN_ACTOR_MAX_OBS); return false; }
  if (c->dtype != 0 && c->dtype != 1) { err->set("cfg.dtype = %d: must be 0 (float32) or 1 (float64)", c->dtype); return false; }
  if (c->n_hidden < 1 || c->n_hidden > BCN_ACTOR_MAX_LAYERS) { err->set("cfg.n_hidden = %d: must lie in 1 .. %d", c->n_hidden, BCN_ACTOR_MAX_LAYERS); return false; }
  for (int l = 0; l < c->n_hidden; l++)
    if (c->hidden[l] < 1 || c->hidden[l] > BCN_ACTOR_MAX_HIDDEN) {
      err->set("cfg.hidden[%d] = %d: must lie in 1 .. %d", l, c->hidden[l], BCN_ACTOR_MAX_HIDDEN);
      return false;
    }
  if (c->activation != BCN_ACTOR_TANH && c->activation != BCN_ACTOR_RELU) { err->set("cfg.activation = %d: must be 0 (tanh) or 1 (relu)", c->activation); return false; }
  if (c->kind != BCN_ACTOR_GAUSSIAN && c->kind != BCN_ACTOR_CATEGORICAL) { err->set("cfg.kind = %d: must be 0 (Gaussian) or 1 (categorical)", c->kind); return false; }
  const int lo = c->kind == BCN_ACTOR_GAUSSIAN ? 1 : 2;
  if (c->act_dim < lo || c->act_dim > BCN_ACTOR_MAX_ACT) { err->set("cfg.act_dim = %d: must lie in %d .. %d for this kind", c->act_dim, lo, BCN_ACTOR_MAX_ACT); return false; }
  if (c->kind == BCN_ACTOR_GAUSSIAN && !(c->low <= c->high)) { err->set("cfg.low = %g, cfg.high = %g: need low <= high", c->low, c->high); return false; }
  if (c->agents < 0) { err->set("cfg.agents = %d: must be >= 0 (0 means 1)", c->agents); return false; }
  if (need_batch && c->agents > 1 && c->batch % c->agents != 0) {
    err->set("cfg.batch = %d is no multiple of cfg.agents = %d: batch counts rows, agents per replica", c->batch, c->agents);
    return false;
  }
  return true;
}

// rows per replica of a cfg: cfg.agents, 0 meaning 1
inline int policy_agents(const bcn_actor_cfg* c) { return c->agents > 1 ? c->agents : 1; }

inline size_t policy_esz(const bcn_actor_cfg* c) { return c->dtype ? 8 : 4; }

// one segment of a packed buffer: planes x rows x row_elems elements (planes = 0: row_elems elements)
struct PolicySegDesc { char name[16]; int elem; int planes; size_t row_elems; };

// lays nd segments out, each 16-byte aligned, for `rows` rows per plane; returns the bytes.  An element is esz bytes (BCN_ACTOR_REAL),
// 8 (elem 3: BCN_LEARNER_F64 of beacon_learner.h) or 4.
inline size_t policy_lay(const PolicySegDesc* d, int nd, size_t rows, size_t esz, bcn_actor_seg* segs, int max_segs) {
  size_t off = 0;
  for (int k = 0; k < nd; k++) {
    off = (off + 15) & ~(size_t)15;
    if (segs && k < max_segs) {
      memset(&segs[k], 0, sizeof(segs[k]));
      strncpy(segs[k].name, d[k].name, sizeof(segs[k].name) - 1);
      segs[k].offset = off; segs[k].elem = d[k].elem; segs[k].planes = d[k].planes; segs[k].row_elems = (int64_t)d[k].row_elems;
    }
    off += (d[k].planes == 0 ? 1 : (size_t)d[k].planes * rows) * d[k].row_elems * (d[k].elem == BCN_ACTOR_REAL ? esz : d[k].elem == 3 ? 8 : 4);
  }
  return (off + 15) & ~(size_t)15;
}

// the parameter layout of include/beacon_actor.h (the gradient's too): pi_w0, pi_b0 ... vf_w0 ... log_std; returns the segment count
inline int policy_params_lay(const bcn_actor_cfg* c, bcn_actor_seg* segs, int max_segs, size_t* bytes) {
  PolicySegDesc d[BCN_ACTOR_MAX_SEGS];
  int nd = 0;
  for (int net = 0; net < 2; net++) {
    size_t in = (size_t)c->obs_dim;
    for (int l = 0; l <= c->n_hidden; l++) {
      const size_t out = l < c->n_hidden ? (size_t)c->hidden[l] : (net == 0 ? (size_t)c->act_dim : 1);
      snprintf(d[nd].name, sizeof(d[nd].name), "%s_w%d", net ? "vf" : "pi", l);
      d[nd].elem = BCN_ACTOR_REAL; d[nd].planes = 0; d[nd].row_elems = out * in; nd++;
      snprintf(d[nd].name, sizeof(d[nd].name), "%s_b%d", net ? "vf" : "pi", l);
      d[nd].elem = BCN_ACTOR_REAL; d[nd].planes = 0; d[nd].row_elems = out; nd++;
      in = out;
    }
  }
  snprintf(d[nd].name, sizeof(d[nd].name), "log_std");
  d[nd].elem = BCN_ACTOR_REAL; d[nd].planes = 0; d[nd].row_elems = c->kind == BCN_ACTOR_GAUSSIAN ? (size_t)c->act_dim : 0; nd++;
  *bytes = policy_lay(d, nd, 1, policy_esz(c), segs, max_segs);
  return nd;
}

// the network's part of a kernel's argument block (ActorArgs, LearnerArgs): what the cfg and the parameter layout decide
template <typename real, typename Args>
inline void policy_fill_net(const bcn_actor_cfg* c, const void* params, Args* a) {
  a->params = static_cast<const real*>(params);
  a->obs_dim = c->obs_dim; a->n_hidden = c->n_hidden; a->activation = c->activation; a->kind = c->kind; a->act_dim = c->act_dim;
  int hmax = 0;
  for (int l = 0; l < c->n_hidden; l++) { a->hidden[l] = c->hidden[l]; hmax = c->hidden[l] > hmax ? c->hidden[l] : hmax; }
  a->hmax_pad = hmax;
  const int omax = hmax > c->act_dim ? hmax : c->act_dim;
  a->wcols = ((omax + 3) & ~3) + 4;
  bcn_actor_seg s[BCN_ACTOR_MAX_SEGS];
  size_t bytes;
  const int ns = policy_params_lay(c, s, BCN_ACTOR_MAX_SEGS, &bytes);
  const int per = 2 * (c->n_hidden + 1);
  for (int l = 0; l <= c->n_hidden; l++) {
    a->pi.w[l] = (unsigned)(s[2 * l].offset / sizeof(real));       a->pi.b[l] = (unsigned)(s[2 * l + 1].offset / sizeof(real));
    a->vf.w[l] = (unsigned)(s[per + 2 * l].offset / sizeof(real)); a->vf.b[l] = (unsigned)(s[per + 2 * l + 1].offset / sizeof(real));
  }
  a->log_std = (unsigned)(s[ns - 1].offset / sizeof(real));
}

// Before a launch with `lds` bytes of dynamic LDS: raise the kernel's limit once per device.  `allowed`: the launch's own static table.
inline hipError_t policy_allow_lds(const void* kernel, size_t lds, size_t (&allowed)[64]) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (lds > 48 * 1024 && (dev < 0 || dev >= 64 || allowed[dev] < lds)) {
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) allowed[dev] = 160 * 1024;
  }
  return hipSuccess;
}
