// epochs.hip -- libbeacon_epochs.so (include/beacon_epochs.h): the shuffle of a PPO epoch and the head of an update.  ONE unit:
// the kernels are templates on the real type, both instantiated here and chosen by the batch's dtype.
//
//   epochs_permute_kernel   idx[i] = the cycle walk of the header's Feistel map from i, one lane per i; the round function is word 0
//                           of the project's one Philox definition (../env1d.h: bcn_philox4x32) at the counter (half, epoch, r, 3)
//   epochs_tick_kernel      epoch[0] += 1, a launch of its own behind the permutation (the learner's adam / tick pattern)
//   epochs_sum_kernel, epochs_dev_kernel, epochs_write_kernel   the three launches of the standardisation: float64 accumulators, the
//                           fixed order the header states, the partials of a launch read by the next
//   epochs_clear_kernel     the stop flag alone
// No atomics, no communication between workgroups inside a launch, no allocation.  Built without FMA contraction: one rounding per
// written operation, so the float64 sums are the sequence the header states.
#include <stdarg.h>

#include "../env1d.h"                     // bcn_philox4x32
#include "../../../include/beacon_epochs.h"

#define EPOCHS_NT 256
#define EPOCHS_PER_LANE (BCN_EPOCHS_CHUNK / EPOCHS_NT)

struct EpochsErr {
  char text[512] = "";
  __attribute__((format(printf, 2, 3))) void set(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
  }
};
static thread_local EpochsErr g_epochs_err;

// ---- the permutation -------------------------------------------------------------------------------------------------------------
// f of the header: six rounds over (L: hl bits, R: hr bits)
__device__ __forceinline__ uint32_t epochs_feistel(uint32_t x, int hl, int hr, uint32_t epoch, uint32_t k0, uint32_t k1) {
  const uint32_t ml = (1u << hl) - 1u, mr = (1u << hr) - 1u;
  uint32_t L = x >> hr, R = x & mr;
#pragma unroll
  for (int r = 0; r < BCN_EPOCHS_ROUNDS; r++) {
    uint32_t o[4];
    if ((r & 1) == 0) {
      bcn_philox4x32(R, epoch, (uint32_t)r, 3u, k0, k1, o);
      L ^= o[0] & ml;
    } else {
      bcn_philox4x32(L, epoch, (uint32_t)r, 3u, k0, k1, o);
      R ^= o[0] & mr;
    }
  }
  return (L << hr) | R;
}

__global__ __launch_bounds__(EPOCHS_NT) void epochs_permute_kernel(long long n, int k, uint32_t k0, uint32_t k1, const int32_t* epoch_dev,
                                                                   int32_t* idx) {
  const long long i = (long long)blockIdx.x * EPOCHS_NT + threadIdx.x;
  if (i >= n) return;
  const uint32_t epoch = (uint32_t)epoch_dev[0];
  const int hl = k / 2, hr = k - hl;
  const uint32_t domain = 1u << k;            // k <= 31
  uint32_t x = (uint32_t)i;
  int32_t out = (int32_t)i;                   // never kept: the walk ends within `domain` applications (header)
  for (uint32_t t = 0; t < domain; t++) {     // bounded: a mistake in the map is a wrong answer, not a hang
    x = epochs_feistel(x, hl, hr, epoch, k0, k1);
    if ((long long)x < n) { out = (int32_t)x; break; }
  }
  idx[i] = out;
}

__global__ void epochs_tick_kernel(int32_t* epoch_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) epoch_dev[0] = (int32_t)((uint32_t)epoch_dev[0] + 1u);
}

// ---- the standardisation ---------------------------------------------------------------------------------------------------------
template <typename real>
struct EpochsArgs {
  const real* adv;
  real* out;
  const void* weight;
  const int32_t* cursor;
  int32_t* step;
  double *moments, *part, *part2;
  long long n_rows, chunks;
  int weight_kind, rows_per_step, rows_per_weight;
};

// the rows below `lim` can be active: n_rows, or what the rollout's cursor has recorded
template <typename real>
__device__ __forceinline__ long long epochs_limit(const EpochsArgs<real>& A) {
  long long lim = A.n_rows;
  if (A.cursor) {
    const long long c = A.cursor[0] > 0 ? A.cursor[0] : 0;
    lim = min(lim, c * (long long)A.rows_per_step);
  }
  return lim;
}

template <typename real>
__device__ __forceinline__ bool epochs_active(const EpochsArgs<real>& A, long long s, long long lim) {
  if (s >= lim) return false;
  const long long ws = A.rows_per_weight > 1 ? (long long)((uint32_t)s / (uint32_t)A.rows_per_weight) : s;
  if (A.weight_kind == BCN_EPOCHS_W_U8) return static_cast<const uint8_t*>(A.weight)[ws] > 0;
  if (A.weight_kind == BCN_EPOCHS_W_REAL) return static_cast<const real*>(A.weight)[ws] > real(0);
  return true;
}

// the 256 lanes' accumulators by the tree 128, 64, ... 1; the sum is in sh[0] for every lane behind the last barrier
__device__ __forceinline__ double epochs_tree(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();                            // the previous use of sh is read
  sh[t] = v;
  __syncthreads();
  for (int d = EPOCHS_NT / 2; d > 0; d >>= 1) {
    if (t < d) sh[t] += sh[t + d];
    __syncthreads();
  }
  return sh[0];
}

// (sum, count) of the G partials for g ascending
__device__ __forceinline__ void epochs_totals(const double* part, int G, double* sum, double* cnt) {
  double s = 0.0, c = 0.0;
  for (int g = 0; g < G; g++) { s += part[2 * g]; c += part[2 * g + 1]; }
  *sum = s; *cnt = c;
}

template <typename real>
__global__ __launch_bounds__(EPOCHS_NT) void epochs_sum_kernel(const EpochsArgs<real> A) {
  __shared__ double sh[EPOCHS_NT];
  const long long lim = epochs_limit(A);
  double s = 0.0, c = 0.0;
  for (long long ch = blockIdx.x; ch < A.chunks; ch += gridDim.x)
#pragma unroll
    for (int j = 0; j < EPOCHS_PER_LANE; j++) {
      const long long row = ch * BCN_EPOCHS_CHUNK + j * EPOCHS_NT + threadIdx.x;
      if (row < A.n_rows && epochs_active(A, row, lim)) { s += (double)A.adv[row]; c += 1.0; }
    }
  const double ts = epochs_tree(s, sh);
  const double tc = epochs_tree(c, sh);
  if (threadIdx.x == 0) {
    A.part[2 * blockIdx.x] = ts;
    A.part[2 * blockIdx.x + 1] = tc;
    if (blockIdx.x == 0 && A.step) A.step[2] = 0;
  }
}

template <typename real>
__global__ __launch_bounds__(EPOCHS_NT) void epochs_dev_kernel(const EpochsArgs<real> A) {
  __shared__ double sh[EPOCHS_NT];
  const long long lim = epochs_limit(A);
  double sum, cnt;
  epochs_totals(A.part, (int)gridDim.x, &sum, &cnt);          // every lane: the same loads in the same order, the same bits
  const double mean = sum / (cnt > 1.0 ? cnt : 1.0);
  double q = 0.0;
  for (long long ch = blockIdx.x; ch < A.chunks; ch += gridDim.x)
#pragma unroll
    for (int j = 0; j < EPOCHS_PER_LANE; j++) {
      const long long row = ch * BCN_EPOCHS_CHUNK + j * EPOCHS_NT + threadIdx.x;
      if (row < A.n_rows && epochs_active(A, row, lim)) {
        const double d = (double)A.adv[row] - mean;
        q += d * d;
      }
    }
  const double tq = epochs_tree(q, sh);
  if (threadIdx.x == 0) {
    A.part2[blockIdx.x] = tq;
    if (blockIdx.x == 0) {
      A.moments[BCN_EPOCHS_MOM_MEAN] = mean;
      A.moments[BCN_EPOCHS_MOM_COUNT] = cnt;
    }
  }
}

template <typename real>
__global__ __launch_bounds__(EPOCHS_NT) void epochs_write_kernel(const EpochsArgs<real> A) {
  const long long lim = epochs_limit(A);
  const double mean = A.moments[BCN_EPOCHS_MOM_MEAN], cnt = A.moments[BCN_EPOCHS_MOM_COUNT];
  double q = 0.0;
  for (int g = 0; g < (int)gridDim.x; g++) q += A.part2[g];
  const double var = q / (cnt - 1.0 > 1.0 ? cnt - 1.0 : 1.0);
  const double den = sqrt(var) + 1e-8;
  for (long long ch = blockIdx.x; ch < A.chunks; ch += gridDim.x)
#pragma unroll
    for (int j = 0; j < EPOCHS_PER_LANE; j++) {
      const long long row = ch * BCN_EPOCHS_CHUNK + j * EPOCHS_NT + threadIdx.x;
      if (row < A.n_rows) A.out[row] = epochs_active(A, row, lim) ? (real)(((double)A.adv[row] - mean) / den) : real(0);
    }
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    A.moments[BCN_EPOCHS_MOM_VAR] = var;
    A.moments[BCN_EPOCHS_MOM_DENOM] = den;
  }
}

__global__ void epochs_clear_kernel(int32_t* step) {
  if (threadIdx.x == 0 && blockIdx.x == 0) step[2] = 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static int epochs_work_lay(bcn_epochs_seg* segs, int max_segs, size_t* bytes) {
  const struct { const char* name; size_t n; } d[3] = {{"moments", BCN_EPOCHS_N_MOMENTS}, {"part", 2 * BCN_EPOCHS_GRID}, {"part2", BCN_EPOCHS_GRID}};
  size_t off = 0;
  for (int k = 0; k < 3; k++) {
    off = (off + 15) & ~(size_t)15;
    if (segs && k < max_segs) {
      memset(&segs[k], 0, sizeof(segs[k]));
      strncpy(segs[k].name, d[k].name, sizeof(segs[k].name) - 1);
      segs[k].offset = off; segs[k].elem = BCN_EPOCHS_F64; segs[k].planes = 0; segs[k].row_elems = (int64_t)d[k].n;
    }
    off += d[k].n * sizeof(double);
  }
  *bytes = (off + 15) & ~(size_t)15;
  return 3;
}

template <typename real>
static int epochs_begin_t(const bcn_epochs_batch* b, void* stream) {
  EpochsArgs<real> a;
  memset(&a, 0, sizeof(a));
  a.adv = static_cast<const real*>(b->adv_dev);
  a.out = static_cast<real*>(b->adv_out_dev);
  a.weight = b->weight_dev; a.weight_kind = b->weight_kind;
  a.cursor = b->cursor_dev; a.rows_per_step = b->rows_per_step;
  a.rows_per_weight = b->rows_per_weight > 1 ? b->rows_per_weight : 1;
  a.step = b->step_dev;
  a.n_rows = (long long)b->n_rows;
  a.chunks = (a.n_rows + BCN_EPOCHS_CHUNK - 1) / BCN_EPOCHS_CHUNK;
  bcn_epochs_seg s[3];
  size_t bytes;
  epochs_work_lay(s, 3, &bytes);
  char* wk = static_cast<char*>(b->work_dev);
  a.moments = reinterpret_cast<double*>(wk + s[0].offset);
  a.part = reinterpret_cast<double*>(wk + s[1].offset);
  a.part2 = reinterpret_cast<double*>(wk + s[2].offset);
  const int grid = a.chunks < BCN_EPOCHS_GRID ? (int)a.chunks : BCN_EPOCHS_GRID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(epochs_sum_kernel<real>, dim3(grid), dim3(EPOCHS_NT), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(epochs_dev_kernel<real>, dim3(grid), dim3(EPOCHS_NT), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(epochs_write_kernel<real>, dim3(grid), dim3(EPOCHS_NT), 0, st, a);
  return (int)hipGetLastError();
}

extern "C" {

BCN_EPOCHS_API const char* bcn_epochs_last_error(void) { return g_epochs_err.text; }

BCN_EPOCHS_API int bcn_epochs_work_layout(bcn_epochs_seg* segs, int max_segs) {
  size_t bytes;
  return epochs_work_lay(segs, max_segs, &bytes);
}

BCN_EPOCHS_API size_t bcn_epochs_work_bytes(void) {
  size_t bytes;
  epochs_work_lay(nullptr, 0, &bytes);
  return bytes;
}

BCN_EPOCHS_API int bcn_epochs_permute(int64_t n, uint64_t seed, int32_t* epoch_dev, int32_t* idx_dev, void* stream) {
  if (n < 1 || n > 0x7fffffffll) { g_epochs_err.set("bcn_epochs_permute: n = %lld: must lie in 1 .. 2^31 - 1", (long long)n); return BCN_EPOCHS_ERR_ARG; }
  if (!epoch_dev) { g_epochs_err.set("bcn_epochs_permute: epoch_dev is NULL"); return BCN_EPOCHS_ERR_ARG; }
  if (!idx_dev) { g_epochs_err.set("bcn_epochs_permute: idx_dev is NULL"); return BCN_EPOCHS_ERR_ARG; }
  int k = 0;                                 // bit_length(n - 1)
  for (uint64_t v = (uint64_t)(n - 1); v; v >>= 1) k++;
  k = k < 2 ? 2 : k;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)((n + EPOCHS_NT - 1) / EPOCHS_NT);
  hipLaunchKernelGGL(epochs_permute_kernel, dim3(blocks), dim3(EPOCHS_NT), 0, st, (long long)n, k, (uint32_t)(seed & 0xffffffffull),
                     (uint32_t)(seed >> 32), (const int32_t*)epoch_dev, idx_dev);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(epochs_tick_kernel, dim3(1), dim3(64), 0, st, epoch_dev);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { g_epochs_err.set("bcn_epochs_permute: launch -> %s", hipGetErrorString(e)); return BCN_EPOCHS_ERR_HIP; }
  return BCN_EPOCHS_OK;
}

BCN_EPOCHS_API int bcn_epochs_begin(const bcn_epochs_batch* b, void* stream) {
  if (!b) { g_epochs_err.set("bcn_epochs_begin: batch is NULL"); return BCN_EPOCHS_ERR_ARG; }
  if (!b->normalize) {
    if (!b->step_dev) { g_epochs_err.set("bcn_epochs_begin: batch.step_dev is NULL without batch.normalize: nothing to do"); return BCN_EPOCHS_ERR_ARG; }
    hipLaunchKernelGGL(epochs_clear_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), b->step_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_epochs_err.set("bcn_epochs_begin: launch -> %s", hipGetErrorString(e)); return BCN_EPOCHS_ERR_HIP; }
    return BCN_EPOCHS_OK;
  }
  if (b->dtype != 0 && b->dtype != 1) { g_epochs_err.set("bcn_epochs_begin: batch.dtype = %d: must be 0 (float32) or 1 (float64)", b->dtype); return BCN_EPOCHS_ERR_ARG; }
  if (!b->adv_dev) { g_epochs_err.set("bcn_epochs_begin: batch.adv_dev is NULL"); return BCN_EPOCHS_ERR_ARG; }
  if (!b->adv_out_dev) { g_epochs_err.set("bcn_epochs_begin: batch.adv_out_dev is NULL"); return BCN_EPOCHS_ERR_ARG; }
  if (b->adv_out_dev == b->adv_dev) { g_epochs_err.set("bcn_epochs_begin: batch.adv_out_dev aliases batch.adv_dev: the third launch reads what it would overwrite"); return BCN_EPOCHS_ERR_ARG; }
  if (!b->work_dev) { g_epochs_err.set("bcn_epochs_begin: batch.work_dev is NULL"); return BCN_EPOCHS_ERR_ARG; }
  if (b->n_rows < 1 || b->n_rows > 0x7fffffffll) { g_epochs_err.set("bcn_epochs_begin: batch.n_rows = %lld: must lie in 1 .. 2^31 - 1", (long long)b->n_rows); return BCN_EPOCHS_ERR_ARG; }
  if (b->weight_kind < BCN_EPOCHS_W_NONE || b->weight_kind > BCN_EPOCHS_W_REAL) {
    g_epochs_err.set("bcn_epochs_begin: batch.weight_kind = %d: must be 0 (none), 1 (uint8) or 2 (real)", b->weight_kind);
    return BCN_EPOCHS_ERR_ARG;
  }
  if (b->weight_kind != BCN_EPOCHS_W_NONE && !b->weight_dev) {
    g_epochs_err.set("bcn_epochs_begin: batch.weight_dev is NULL with weight_kind = %d", b->weight_kind);
    return BCN_EPOCHS_ERR_ARG;
  }
  if (b->cursor_dev && b->rows_per_step < 1) { g_epochs_err.set("bcn_epochs_begin: batch.rows_per_step = %d: a cursor needs >= 1", b->rows_per_step); return BCN_EPOCHS_ERR_ARG; }
  if (b->rows_per_weight < 0) { g_epochs_err.set("bcn_epochs_begin: batch.rows_per_weight = %d: must be >= 0 (0 means 1)", b->rows_per_weight); return BCN_EPOCHS_ERR_ARG; }
  if (b->rows_per_weight > 1 && b->n_rows % b->rows_per_weight != 0) {
    g_epochs_err.set("bcn_epochs_begin: batch.rows_per_weight = %d does not divide batch.n_rows = %lld", b->rows_per_weight, (long long)b->n_rows);
    return BCN_EPOCHS_ERR_ARG;
  }
  const int e = b->dtype ? epochs_begin_t<double>(b, stream) : epochs_begin_t<float>(b, stream);
  if (e) { g_epochs_err.set("bcn_epochs_begin: launch -> %s", hipGetErrorString((hipError_t)e)); return BCN_EPOCHS_ERR_HIP; }
  return BCN_EPOCHS_OK;
}

}  // extern "C"
