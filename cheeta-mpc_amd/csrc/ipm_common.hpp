#pragma once
// ipm_common.hpp — everything the dense IPM kernel families share that is not their linear algebra (k_ipm64.hpp with
// k_solve64, k_ipm72.hpp, k_ipm128x.hpp with k_solve128, k_ipm256.hpp, k_ric.hpp; namespace cmpc::ipm, brought in
// with `using namespace ipm;` in the kernel bodies): the numerical guards that must agree with the oracle, the
// compile-time loops and small device helpers, the phase stamps of the diagnostic builds, and the bookkeeping of the
// Mehrotra controller (statistics row, centering parameter, residual row, class-list lookup, stopping rule).
// Everything here is __forceinline__ or a macro: the kernels' code objects do not depend on where a piece is written.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cmpc/cmpc.h"

// ---- In-kernel s_memtime stamps, diagnostic builds only: cycles of each phase accumulated into NSEG slots and stored
// per QP as ptr[q][STRIDE] = the slots, then the total in slot NSEG. The _ON forms are the one implementation;
// IPM_STAMP_DECL / IPM_STAMP / IPM_STAMP_STORE are live under -DCMPC_IPM_STAMPS (lab/run_lab.sh; IpmArgs::stamps) and
// expand to nothing otherwise. Families with a switch of their own (k_ric.hpp) map their names onto the _ON forms.
#define IPM_STAMP_DECL_ON(NSEG)                                     \
  unsigned long long st_acc_[NSEG] = {};                            \
  const unsigned long long st_t0_ = ::cmpc::ipm::memtime();         \
  unsigned long long st_prev_ = st_t0_
#define IPM_STAMP_ON(k)                                             \
  do {                                                              \
    const unsigned long long t_ = ::cmpc::ipm::memtime();           \
    st_acc_[k] += t_ - st_prev_;                                    \
    st_prev_ = t_;                                                  \
  } while (0)
#define IPM_STAMP_STORE_ON(ptr, q, NSEG, STRIDE)                                              \
  do {                                                                                        \
    const unsigned long long t_ = ::cmpc::ipm::memtime();                                     \
    if ((ptr) && threadIdx.x == 0) {                                                          \
      for (int k_ = 0; k_ < (NSEG); ++k_) (ptr)[(size_t)(q) * (STRIDE) + k_] = st_acc_[k_];   \
      (ptr)[(size_t)(q) * (STRIDE) + (NSEG)] = t_ - st_t0_;                                   \
    }                                                                                         \
  } while (0)
#ifdef CMPC_IPM_STAMPS
#define IPM_STAMP_DECL(NSEG) IPM_STAMP_DECL_ON(NSEG)
#define IPM_STAMP(k) IPM_STAMP_ON(k)
#define IPM_STAMP_STORE(ptr, q, NSEG, STRIDE) IPM_STAMP_STORE_ON(ptr, q, NSEG, STRIDE)
#else
#define IPM_STAMP_DECL(NSEG) (void)0
#define IPM_STAMP(k) (void)0
#define IPM_STAMP_STORE(ptr, q, NSEG, STRIDE) (void)0
#endif

// ---- The stopping rule of every family, stated once (HPIPM's absolute rule and the oracle's precedence,
// oracle/cmpc_oracle.c:qp_ipm_run): a non-finite residual -> NAN_SOL; every residual within its tolerance -> SUCCESS;
// it >= iter_max -> MAX_ITER; mu underflow (m > 0 and not mu > Lim<T>::mu_min) -> MIN_STEP. The tests are evaluated in
// this order and only until one holds (in the kernels they are wave votes, or workgroup votes that carry a barrier),
// and the statement that holds sets `status` and leaves the iteration loop. A macro because the rule has to break out
// of the caller's loop without evaluating the later votes: a function taking the votes as lambdas cost SGPR spills in
// k_ipm64.
#define IPM_BREAK_IF_STOPPED(status, nan_vote, conv_vote, it, iter_max, mu_lost) \
  if (nan_vote) {                                                                \
    status = CMPC_NAN_SOL;                                                       \
    break;                                                                       \
  } else if (conv_vote) {                                                        \
    status = CMPC_SUCCESS;                                                       \
    break;                                                                       \
  } else if ((it) >= (iter_max)) {                                               \
    status = CMPC_MAX_ITER;                                                      \
    break;                                                                       \
  } else if (mu_lost) {                                                          \
    status = CMPC_MIN_STEP;                                                      \
    break;                                                                       \
  } else                                                                         \
    (void)0

namespace cmpc {
namespace ipm {

// Guards shared with the oracle (oracle/cmpc_oracle.c: the pivot guard of its Cholesky and the mu test of qp_ipm_run;
// oracle/ocp_ipm.c restates them for the OCP form): the kernels and the oracle must drop the same directions and stop
// at the same iteration.
template <typename T>
struct Lim;
template <>
struct Lim<double> {
  static constexpr double pivot_min = 1e-200;  // BLASFEO-style guard: smaller pivots drop their direction
  static constexpr double mu_min = 1e-300;     // mu underflow -> MIN_STEP instead of 0/0
};
template <>
struct Lim<float> {
  static constexpr float pivot_min = 1e-30f;
  static constexpr float mu_min = 1e-35f;
};

__device__ __forceinline__ unsigned long long memtime() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}

// compile-time loops: f(std::integral_constant<int, i>) for i = B .. E-1, and for i = E-1 down to B
template <int B, int E, typename F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    sfor<B + 1, E>(f);
  }
}
template <int B, int E, typename F>
__device__ __forceinline__ void sfor_down(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, E - 1>{});
    sfor_down<B, E - 1>(f);
  }
}

// Compiler-only ordering of LDS accesses: one wave's DS instructions execute in order, so a read issued after a
// write (or a write after a read) in program order sees the right data without s_waitcnt.
__device__ __forceinline__ void cbar() { asm volatile("" ::: "memory"); }
// Ordering of LDS traffic between the lanes of one wave: LDS writes drained (lgkmcnt) before the other lanes read them.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// Lane / wave ids the compiler cannot hoist: addresses derived from them are recomputed where they are used instead of
// staying live in ~100 VGPRs across the iteration. olane(): the one-wave kernels (the workgroup is the wave);
// olane_mw() / owave(): lane within its wave and wave index of a multi-wave workgroup.
__device__ __forceinline__ int olane() {
  int l = (int)threadIdx.x;
  asm volatile("" : "+v"(l));
  return l;
}
__device__ __forceinline__ int olane_mw() {
  int l = (int)threadIdx.x & 63;
  asm volatile("" : "+v"(l));
  return l;
}
__device__ __forceinline__ int owave() {
  int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  asm volatile("" : "+s"(w));
  return w;
}
// a wave-uniform flag as a scalar
__device__ __forceinline__ bool uflag(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }

__device__ __forceinline__ double rcp_raw(double x) { return __builtin_amdgcn_rcp(x); }
__device__ __forceinline__ float rcp_raw(float x) { return __builtin_amdgcn_rcpf(x); }
// reciprocal of a pivot: hardware estimate + one Newton step, 0 for pivots at or below the guard (and NaN)
template <typename T>
__device__ __forceinline__ T pivot_inv(T p) {
  T y = rcp_raw(p);
  const T e = fma(-p, y, T(1));
  y = fma(y, e, y);
  return p > T(Lim<T>::pivot_min) ? y : T(0);
}

// ---- Mehrotra controller bookkeeping. Statistics row of an iteration (cmpc_enable_stats): [0..2] alpha_aff, mu_aff,
// sigma of the predictor, [3..4] the step (one length for primal and dual), [5] mu, [6..9] the residuals (stat, eq = 0,
// ineq, comp). The row is opened with NaN in the step columns, which stay NaN at the iteration that stops.
template <typename Args>
__device__ __forceinline__ double* stat_row(const Args& a, int q, int it) {
  return a.stats + ((size_t)q * a.stats_cap + it) * CMPC_STAT_COLS;
}
template <typename T>
__device__ __forceinline__ void stat_residuals(double* sr, T mu, T rs, T ri, T rc) {
  sr[5] = (double)mu;
  sr[6] = (double)rs;
  sr[7] = 0.0;
  sr[8] = (double)ri;
  sr[9] = (double)rc;
}
template <typename T>
__device__ __forceinline__ void stat_open(double* sr, T mu, T rs, T ri, T rc) {
  for (int k = 0; k < 5; ++k) sr[k] = __builtin_nan("");
  stat_residuals(sr, mu, rs, ri, rc);
}
template <typename T>
__device__ __forceinline__ void stat_predictor(double* sr, T alpha, T maff, T sigma) {
  sr[0] = (double)alpha;
  sr[1] = (double)maff;
  sr[2] = (double)sigma;
}
template <typename T>
__device__ __forceinline__ void stat_step(double* sr, T alpha) {
  sr[3] = sr[4] = (double)alpha;
}
// centering parameter sigma = (mu_aff / mu)^3
template <typename T>
__device__ __forceinline__ T centering(T maff, T mu) {
  const T ratio = maff / mu;
  return ratio * ratio * ratio;
}
// final residuals of QP q (cmpc_get_residuals): res[q][4] = (stat, eq = 0, ineq, comp)
template <typename T>
__device__ __forceinline__ void res_store(double* res, int q, T rs, T ri, T rc) {
  double* o = res + (size_t)q * 4;
  o[0] = (double)rs;
  o[1] = 0.0;
  o[2] = (double)ri;
  o[3] = (double)rc;
}
// QP of this workgroup in size class cls into q; false if the workgroup has none and exits. With a compacted class
// list (IpmArgs::qlist[cls]) the real QPs come first and the surplus workgroups exit; grid = batch, so a corrupt list
// entry cannot address past it. (Returning the index with -1 for "none" adds a sign test the compiler cannot fold -
// a list entry below a grid of 2^31 or more - and changed k_ipm64's code object.)
template <typename Args>
__device__ __forceinline__ bool class_qp(const Args& a, int cls, int& q) {
  q = blockIdx.x;
  if (a.qlist[cls]) {
    if (q >= a.qcount[cls]) return false;
    q = a.qlist[cls][q];
    if ((unsigned)q >= gridDim.x) return false;
  }
  return true;
}

}  // namespace ipm
}  // namespace cmpc
