// ns2d_sched.h -- what the three register-resident kernel families (ns2d_fast_impl.h, ns2d_fast2_impl.h, ns2d_fast4_impl.h)
// share around their units of work: the ticketed chunk scheduler (device), the layout of its control block and the ONE host
// launcher (ns2d_sched_launch), which a family parameterises by its two kernels and a SchedPolicy.
#pragma once
#include <stdlib.h>

#include "ns2d.h"
#include "ns2d_prm.h"   // the launcher passes the per-replica table on where a unit is built with BCN_PRM_KERNELS

// With more replicas than CUs a replica is no longer tied to one workgroup: the step is cut into
// chunks of A.sched_q timesteps and persistent workgroups (one per CU) draw (chunk, replica) units
// from a global ticket counter in chunk-major order, so every CU stays busy until the slowest
// replica's chain of chunks ends (makespan ~ max(critical path, mean) instead of the sum of whichever
// two replicas a CU happened to get).  A replica's state moves between CUs through HBM; the hand-off
// follows the agent-scope release/acquire recipe of the CDNA programming guide (Guideline 16):
//   producer: stores -> workgroup barrier -> lane 0: fence(release, agent); s_waitcnt vmcnt(0);
//             relaxed agent store progress[r] = c+1
//   consumer: lane 0 polls progress[r] (relaxed, agent, s_sleep) -> fence(acquire, agent);
//             s_waitcnt vmcnt(0) -> workgroup barrier -> plain loads.
// Tickets are drawn in order, so when unit (c, r) is drawn unit (c-1, r) has already been drawn by
// a workgroup that never waits on a later ticket: every wait is finite whatever the residency.
// Spins are bounded anyway: on timeout the abort word is set, every workgroup drains, and the
// affected replicas report BCN_ST_ITMAX.
struct SchedCtl {
  unsigned int ticket;
  unsigned int abort;
  unsigned int pad[14];
  unsigned int progress[1];   // [B]
};

// The handle's scheduler block: [ SchedCtl with progress[B] | cyc[B][4] ] (NS2DArgs::sched_ctl, cyc, sched_bytes), zeroed by one
// memset in front of every step launch.  The control part is 128 + 4 B bytes rounded up to 16 -- SchedCtl's 64-byte header and
// progress[B] need 64 + 4 B; the other 64 are spare --, so cyc (unsigned long long) starts aligned.
struct SchedLayout {
  size_t ctl_bytes, cyc_offset, total;
};
inline SchedLayout ns2d_sched_layout(int batch) {
  const size_t ctl = (128 + (size_t)batch * sizeof(unsigned int) + 15) / 16 * 16;
  return {ctl, ctl, ctl + (size_t)batch * 4 * sizeof(unsigned long long)};
}

// The persistent workgroup's loop.  `s_words`: two LDS words the unit does not touch (SCHED_WORDS of the family's geometry struct);
// `unit(b, it0, it1, first_chunk, last_chunk)` runs timesteps [it0, it1) of replica b (state HBM ->
// chip -> HBM) and is called by every thread of the workgroup.
template <typename real, typename Unit>
__device__ __forceinline__ void ns2d_sched_loop(const NS2DArgs<real>& A, SchedCtl* ctl, int batch, int nchunk,
                                                unsigned int* s_words, Unit unit) {
  unsigned int& s_ticket = s_words[0];
  unsigned int& s_ok = s_words[1];
  const unsigned int total = (unsigned int)batch * (unsigned int)nchunk;
  for (;;) {
    if (threadIdx.x == 0) s_ticket = atomicAdd(&ctl->ticket, 1u);
    __syncthreads();
    const unsigned int t = s_ticket;
    if (t >= total) break;
    const int c = (int)(t / (unsigned int)batch), b = (int)(t % (unsigned int)batch);
    const bool skip = A.mask && !A.mask[b];
    if (threadIdx.x == 0) {
      unsigned int ok = 1;
      if (!skip && c > 0) {
        unsigned int spins = 0;
        while (__hip_atomic_load(&ctl->progress[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned int)c) {
          __builtin_amdgcn_s_sleep(32);
          if (++spins > (1u << 24) || __hip_atomic_load(&ctl->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            __hip_atomic_store(&ctl->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = 0;
            break;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      s_ok = ok;
    }
    __syncthreads();
    if (!skip) {
      if (s_ok) {
        // chunk c: the first sched_nbig chunks are twice as long (half the hand-offs through HBM where the order of the
        // units cannot matter yet), the last ones short (the step ends when the slowest replica's last chunk does)
        const int it0 = c < A.sched_nbig ? c * 2 * A.sched_q : (c + A.sched_nbig) * A.sched_q;
        const int it1 = (c == nchunk - 1) ? A.ndt_act : it0 + (c < A.sched_nbig ? 2 : 1) * A.sched_q;
        unit(b, it0, it1, c == 0, c == nchunk - 1);
      } else if (threadIdx.x == 0) {
        A.status[b] = BCN_ST_ITMAX;   // handle-owned when the caller passed none: never NULL here
      }
      __syncthreads();   // every wave's stores are issued and waited for (barrier implies vmcnt(0))
      if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&ctl->progress[b], (unsigned int)(c + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();     // s_ticket / s_ok are rewritten next trip
  }
}

// "first launch of this kernel on the current device": the dynamic-LDS attribute is per device, and a process may
// hold handles on several devices (one process per GPU is the deployment, not a requirement of the ABI)
inline bool ns2d_first_on_device(unsigned long long& seen) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (seen & bit) return false;
  seen |= bit;
  return true;
}

// host side, per handle (bcn_set_sched -> NS2DArgs::sched_mode / sched_grid / sched_q_user / lpt_min_batch; -1 / 0 = default):
// mode 0 plain launch, 1 two-launch LPT split (families with SchedPolicy::rank), 2 ticketed chunks (default); grid = persistent
// workgroups (default: one per CU of the handle's device); q = timesteps per chunk (0: the family's SchedPolicy::q_default).
// No environment variable changes any of it.
struct SchedParams {
  int mode, grid, q, lpt_min_batch;
};
inline int ns2d_cu_count() {   // of the current device (one handle per device; a process may hold several)
  static int ncu[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  int& n = ncu[dev & 63];
  if (n <= 0) {
    n = 256;
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
  }
  return n;
}
template <typename real>
inline SchedParams ns2d_sched_params(const NS2DArgs<real>& a) {
  SchedParams p;
  p.mode = a.sched_mode >= 0 ? a.sched_mode : 2;
  const int ncu = ns2d_cu_count();
  p.grid = a.sched_grid > 0 ? a.sched_grid : ncu;
  p.q = a.sched_q_user > 0 ? a.sched_q_user : 0;
  p.lpt_min_batch = a.lpt_min_batch > 0 ? a.lpt_min_batch : ncu + 1;
  return p;
}

// chunks of one step, long ones first: nbig long ones (2 q timesteps) followed by short ones (q; the last takes the remainder),
// the short tail covering at least the last `tail` * q timesteps (bcn_set_option "sched_tail", default 6; a tail >= ndt / q gives
// uniform chunks).
inline void ns2d_sched_chunks(int ndt, int q, int tail_user, int* nbig, int* nchunk) {
  const int tail = tail_user > 0 ? tail_user : 6;
  int nb = (ndt - tail * q) / (2 * q);
  if (nb < 0) nb = 0;
  int rem = ndt - nb * 2 * q;
  int ns = rem / q;
  if (ns < 1) { ns = 1; }
  *nbig = nb;
  *nchunk = nb + ns;
}

// What a kernel family states about itself; everything else of a launch is ns2d_sched_launch.  Each value was measured on
// that family's flagship grid.
struct SchedPolicy {
  const char* step_name;    // NS2DHost::launched after a plain (or split) launch
  const char* sched_name;   //   ... after a ticketed one
  int q_default;            // timesteps per chunk unless bcn_set_sched gave a q
  bool long_first;          // chunk list: ns2d_sched_chunks (long chunks first, "sched_tail") / uniform, ndt_act / q chunks
  // the LPT split (mode >= 1 where the ticketed launch does not apply): ranks the replicas by the sweeps of their first q
  // timesteps into `order`.  NULL: the family has no split.  A pointer, so that the rank kernel lives in its family's header
  // and no other unit gains it.
  void (*rank)(const int32_t* sweeps, int ndt, int q, int batch, int32_t* order, const uint8_t* mask, hipStream_t s);
};

// The launch of one action step by the step kernel K / the ticketed kernel KS of a family (nt threads, lds bytes of dynamic
// LDS): the ticketed persistent launch when replicas outnumber the workgroups, else one workgroup per replica -- in two
// launches around pol.rank where the LPT split applies.  Templated on the kernels THEMSELVES: the first-use masks below are one
// per kernel instantiation (all step kernels of a precision share one pointer type).
template <auto K, auto KS, typename real>
int ns2d_sched_launch(const SchedPolicy& pol, const NS2DArgs<real>& a, int batch, hipStream_t s, int nt, size_t lds BCN_PRM_PARAM) {
  NS2DArgs<real> c = a;
  if (!c.sweeps) c.sweeps = c.sweeps_int;
  c.order = nullptr; c.first_chunk = 1; c.last_chunk = 1; c.it_begin = 0; c.it_end = a.ndt_act;
  const SchedParams sp = ns2d_sched_params(a);
  const int q = sp.q > 0 ? sp.q : pol.q_default;
  if (sp.mode == 2 && batch > sp.grid && a.ndt_act >= 2 * q && a.sched_ctl) {
    static unsigned long long seen = 0;
    if (ns2d_first_on_device(seen)) BCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KS), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int nchunk = a.ndt_act / q;
    c.sched_nbig = 0;
    if (pol.long_first) ns2d_sched_chunks(a.ndt_act, q, (a.host ? a.host->sched_tail : 0), &c.sched_nbig, &nchunk);
    c.sched_q = q;
    BCN_HIP(hipMemsetAsync(a.sched_ctl, 0, a.sched_bytes, s));
    hipLaunchKernelGGL(KS, dim3(sp.grid), dim3(nt), lds, s, c, static_cast<SchedCtl*>(a.sched_ctl), batch, nchunk BCN_PRM_LAUNCH);
    BCN_HIP(hipGetLastError());
    if (a.host) a.host->launched = pol.sched_name;
    return BCN_OK;
  }
  static unsigned long long seen = 0;
  if (ns2d_first_on_device(seen)) BCN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // split only when replicas outnumber the CUs (otherwise every replica starts at once and the order cannot matter);
  // bcn_set_sched overrides the threshold (tests)
  constexpr int Q = 10;
  const bool split = pol.rank && sp.mode >= 1 && batch >= sp.lpt_min_batch && batch <= 2048 && a.ndt_act >= 4 * Q;
  if (a.sched_ctl) BCN_HIP(hipMemsetAsync(a.sched_ctl, 0, a.sched_bytes, s));   // cycle counters
  if (split) {   // timesteps [0, Q) in index order, the rest longest first
    c.it_end = Q; c.last_chunk = 0;
    hipLaunchKernelGGL(K, dim3(batch), dim3(nt), lds, s, c BCN_PRM_LAUNCH);
    pol.rank(c.sweeps, a.ndt_act, Q, batch, c.order_out, c.mask, s);
    c.first_chunk = 0; c.last_chunk = 1; c.it_begin = Q; c.it_end = a.ndt_act; c.order = c.order_out;
  }
  hipLaunchKernelGGL(K, dim3(batch), dim3(nt), lds, s, c BCN_PRM_LAUNCH);
  BCN_HIP(hipGetLastError());
  if (a.host) a.host->launched = pol.step_name;
  return BCN_OK;
}
