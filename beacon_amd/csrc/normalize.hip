// normalize.hip -- the kernels behind bcn_normalize (normalize.h, include/beacon_hip.h): running mean / variance of every
// observation column and of the discounted return over the batch, and the normalised observations, rewards and terminal
// observations, TWO launches behind a step (or a reset); ONE in evaluation mode.
//
// Both kernels cut the batch into G slabs of S replicas and a row into chunks of w = min(n_obs, 64) columns; workgroup
// (slab g, chunk j) = blockIdx.x takes one tile, and the workgroup behind the last chunk of a slab takes the slab's returns and rewards
// (one "column" of its own, a lane per replica).  In a tile lane t sits on column t % w and replica t / w of every trip of
// R = 256 / w replicas, so its column never changes and consecutive lanes touch consecutive addresses of the row-major [B][n_obs]
// arrays: lorenz's 6-real rows go 42 replicas (252 lanes) per trip, rayleigh's 384-real rows as six chunks of 64 columns by 4 replicas.
//  * normalize_stats_k (training only): every lane takes the mean of its own elements, then the sum of squared deviations from
//    it (a second read of the same addresses: no sum of squares is ever formed), and the R lanes of a column merge their
//    (count, mean, M2) pairwise (Chan) through LDS in a fixed tree.  The result goes to the slab's row of the partials.  The
//    return workgroups first advance ret = gamma ret + rwd.  The workgroups of slab 0 also copy the running statistics to the
//    scratch, so that the second kernel reads nothing it writes.
//  * normalize_apply_k: every workgroup merges the G partials of its columns (the R lanes of a column take every R-th, then the
//    same tree), folds the batch moments into the copied running statistics, and normalises its tile with the result; slab 0
//    stores the new statistics.  In evaluation mode it reads the statistics in place and stores none.
// Whatever passes between workgroups passes from the first launch to the second.  No atomics, no scratch memory, every summation
// order fixed by the shape alone: two runs agree bit for bit.  All arithmetic is float64; the env's dtype is a uniform branch
// at the loads and stores.
#include "normalize.h"

namespace {

struct Moments { double n, mean, m2; };

// b into a (Chan et al.); an empty side changes nothing
__device__ __forceinline__ void moments_merge(Moments& a, const Moments& b) {
  if (b.n == 0.0) return;
  if (a.n == 0.0) { a = b; return; }
  const double tot = a.n + b.n, d = b.mean - a.mean, f = b.n / tot;
  a.mean += d * f;
  a.m2 += b.m2 + d * d * a.n * f;
  a.n = tot;
}

// The moments of the R lanes that share a column (lanes t, t + w, t + 2 w, ...), merged in a fixed tree through LDS; every lane
// gets its column's.  Lanes behind R w carry empty moments.  Called once per kernel by all threads.
__device__ __forceinline__ Moments moments_over_rows(Moments m, unsigned t, unsigned r, unsigned ci, unsigned w, unsigned R,
                                                     double (*lds)[BCN_NRM_NT]) {
  lds[0][t] = m.n; lds[1][t] = m.mean; lds[2][t] = m.m2;
  for (unsigned s = BCN_NRM_NT / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (r < s && r + s < R) {                    // t + s w < R w <= BCN_NRM_NT
      const unsigned o = t + s * w;
      const Moments other = {lds[0][o], lds[1][o], lds[2][o]};
      moments_merge(m, other);
      lds[0][t] = m.n; lds[1][t] = m.mean; lds[2][t] = m.m2;
    }
  }
  __syncthreads();
  const Moments out = {lds[0][ci], lds[1][ci], lds[2][ci]};
  return out;
}

__device__ __forceinline__ double nrm_load(const void* p, size_t i, int f64) {
  return f64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}
__device__ __forceinline__ void nrm_store(void* p, size_t i, int f64, double v) {
  if (f64) static_cast<double*>(p)[i] = v;
  else static_cast<float*>(p)[i] = (float)v;
}
__device__ __forceinline__ double nrm_clip(double y, double c) { return y < -c ? -c : (y > c ? c : y); }   // (a NaN stays one)

// the tile of this workgroup and the place of this lane in it
struct Tile {
  unsigned g, j, w, R, r, ci, col, b0, b1;
  bool ret, live;
};
__device__ __forceinline__ Tile nrm_tile(const NormalizeArgs& A) {
  Tile T;
  const unsigned t = threadIdx.x;
  T.g = blockIdx.x / (A.chunks + 1);
  T.j = blockIdx.x - T.g * (A.chunks + 1);
  T.ret = T.j == A.chunks;
  T.w = T.ret ? 1u : A.w;
  T.R = T.ret ? (unsigned)BCN_NRM_NT : A.R;
  T.r = t / T.w;
  T.ci = t - T.r * T.w;
  T.col = T.ret ? A.n_obs : T.j * A.w + T.ci;    // (the return is column n_obs of the scratch arrays)
  T.live = T.r < T.R && T.col <= A.n_obs && (T.ret || T.col < A.n_obs);
  T.b0 = T.g * A.S;
  T.b1 = T.b0 + A.S < A.batch ? T.b0 + A.S : A.batch;
  return T;
}

__device__ __forceinline__ bool nrm_on(const NormalizeArgs& A, unsigned b) { return !A.mask || A.mask[b] != 0; }
__device__ __forceinline__ bool nrm_counts(const NormalizeArgs& A, unsigned b) {
  return nrm_on(A, b) && (A.kind == BCN_NRM_RESET || !(A.status[b] & (BCN_ST_ITMAX | BCN_ST_BLOWUP)));
}

__global__ __launch_bounds__(BCN_NRM_NT) void normalize_stats_k(NormalizeArgs A) {
  __shared__ double lds[3][BCN_NRM_NT];
  const Tile T = nrm_tile(A);
  const unsigned nc = A.n_obs + 1;
  if (T.g == 0 && T.r == 0 && T.live) {          // the statistics in front of the update, for the second launch
    A.prev[T.col] = T.ret ? A.ret_mean[0] : A.obs_mean[T.col];
    A.prev[nc + T.col] = T.ret ? A.ret_var[0] : A.obs_var[T.col];
    if (T.ret || T.col == 0) A.prev[2 * nc + (T.ret ? 1 : 0)] = T.ret ? A.ret_count[0] : A.obs_count[0];
  }
  if (T.ret && A.kind != BCN_NRM_STEP) return;   // a reset leaves the return statistics alone (uniform over the workgroup)
  double* __restrict__ ret = A.ret;
  double sum = 0.0, cnt = 0.0;
  if (T.live) {
#pragma unroll 4
    for (unsigned b = T.b0 + T.r; b < T.b1; b += T.R) {
      double x;
      if (T.ret) {
        x = A.gamma * ret[b] + nrm_load(A.rwd, b, A.f64);
        if (nrm_on(A, b)) ret[b] = x;
      } else {
        x = nrm_load(A.obs, (size_t)b * A.n_obs + T.col, A.f64);
      }
      const bool c = nrm_counts(A, b);
      sum += c ? x : 0.0;
      cnt += c ? 1.0 : 0.0;
    }
  }
  Moments m = {cnt, cnt > 0.0 ? sum / cnt : 0.0, 0.0};
  if (T.live) {
#pragma unroll 4
    for (unsigned b = T.b0 + T.r; b < T.b1; b += T.R) {
      const double x = T.ret ? ret[b] : nrm_load(A.obs, (size_t)b * A.n_obs + T.col, A.f64);
      const double d = x - m.mean;
      m.m2 += nrm_counts(A, b) ? d * d : 0.0;
    }
  }
  m = moments_over_rows(m, threadIdx.x, T.r, T.ci, T.w, T.R, lds);
  if (T.r == 0 && T.live) {
    double* p = A.part + ((size_t)T.g * nc + T.col) * 3;
    p[0] = m.n; p[1] = m.mean; p[2] = m.m2;
  }
}

__global__ __launch_bounds__(BCN_NRM_NT) void normalize_apply_k(NormalizeArgs A) {
  __shared__ double lds[3][BCN_NRM_NT];
  const Tile T = nrm_tile(A);
  const unsigned nc = A.n_obs + 1;
  const bool step = A.kind == BCN_NRM_STEP;
  if (T.ret && !step) {                          // a reset: the return of the replicas it touches starts over
    if (A.training && T.live)
      for (unsigned b = T.b0 + T.r; b < T.b1; b += T.R)
        if (nrm_on(A, b)) A.ret[b] = 0.0;
    return;
  }
  double mean = 0.0, var = 1.0;
  if (A.training) {
    Moments m = {0.0, 0.0, 0.0};
    if (T.live)
      for (unsigned g = T.r; g < A.G; g += T.R) {
        const double* p = A.part + ((size_t)g * nc + T.col) * 3;
        const Moments other = {p[0], p[1], p[2]};
        moments_merge(m, other);
      }
    m = moments_over_rows(m, threadIdx.x, T.r, T.ci, T.w, T.R, lds);
    if (T.live) {
      double count = A.prev[2 * nc + (T.ret ? 1 : 0)];
      mean = A.prev[T.col];
      var = A.prev[nc + T.col];
      if (m.n > 0.0) {
        const double tot = count + m.n, d = m.mean - mean;
        mean += d * m.n / tot;
        var = (var * count + m.m2 + d * d * count * m.n / tot) / tot;
        count = tot;
      }
      if (T.g == 0 && T.r == 0) {
        (T.ret ? A.ret_mean : A.obs_mean + T.col)[0] = mean;
        (T.ret ? A.ret_var : A.obs_var + T.col)[0] = var;
        if (T.ret || T.col == 0) (T.ret ? A.ret_count : A.obs_count)[0] = count;
      }
    }
  } else if (T.live) {
    mean = T.ret ? A.ret_mean[0] : A.obs_mean[T.col];
    var = T.ret ? A.ret_var[0] : A.obs_var[T.col];
  }
  if (!T.live) return;
  const double inv = 1.0 / sqrt(var + A.eps);
  if (T.ret) {
#pragma unroll 4
    for (unsigned b = T.b0 + T.r; b < T.b1; b += T.R) {
      const double x = nrm_load(A.rwd, b, A.f64);
      const bool fin = (A.done[b] | A.trunc[b]) != 0;
      if (!nrm_on(A, b)) continue;
      nrm_store(A.norm_rwd, b, A.f64, nrm_clip(x * inv, A.clip_rwd));
      if (A.training && fin) A.ret[b] = 0.0;
    }
    return;
  }
#pragma unroll 4
  for (unsigned b = T.b0 + T.r; b < T.b1; b += T.R) {
    const size_t e = (size_t)b * A.n_obs + T.col;
    const double x = nrm_load(A.obs, e, A.f64);
    if (!nrm_on(A, b)) continue;
    nrm_store(A.norm_obs, e, A.f64, nrm_clip((x - mean) * inv, A.clip_obs));
    if (step && A.finished && A.finished[b])     // the terminal observation: normalised with the same statistics, never counted
      nrm_store(A.norm_final_obs, e, A.f64, nrm_clip((nrm_load(A.final_obs, e, A.f64) - mean) * inv, A.clip_obs));
  }
}

}  // namespace

int normalize_launch(const NormalizeArgs& a, hipStream_t s) {
  const dim3 grid(a.G * (a.chunks + 1));
  if (a.training) {
    hipLaunchKernelGGL(normalize_stats_k, grid, dim3(BCN_NRM_NT), 0, s, a);
    BCN_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(normalize_apply_k, grid, dim3(BCN_NRM_NT), 0, s, a);
  BCN_HIP(hipGetLastError());
  return BCN_OK;
}
