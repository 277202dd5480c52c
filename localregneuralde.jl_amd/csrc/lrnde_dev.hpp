// lrnde_dev.hpp — the device helpers that more than one translation unit of the library compiles: lrnde_kernels.hip and the
// one-launch SDE step kernels (lrnde_sde_eh_fast.hip, lrnde_sde_mil_fast.hip, lrnde_sde_sri_fast.hip).  The MFMA fragment type
// and chain step, the fp64 partial-sum vector and its fixed-order reduction, the integrator's control block.  Everything a
// kernel calls is __forceinline__ in an anonymous namespace: each translation unit inlines its own copy, nothing is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace lrnde {

// (named, not local to a translation unit: SdeFastArgs — lrnde_sde_fast.hpp, the argument of functions that one translation
// unit declares and another defines — holds pointers to both)
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Ctrl {  // device-resident integrator state, double-buffered by attempt parity
  int status, first;
  int iter, naccept, nreject, nf;
  int cur;  // uprev = ubuf[cur], k1 = kfsal[cur]; the step writes u -> ubuf[cur^1], k7 -> kfsal[cur^1]
  int isave, nsaved;
  float t, dt;  // start time and dt of the last attempted step
  float qold, q11, dtpropose;
  float eest_last, dt_init;
  float reg_error, reg_stiff;  // single-step modes: filled by k_finalize
  float stiff_num, stiff_den;  // ||k7-k6||_rms, ||u-g6||_rms (for the regulariser's reverse sweep)
};

}  // namespace lrnde

namespace {

using namespace lrnde;

constexpr int PSTRIDE = 4;   // doubles per workgroup in a partial-sum vector

// The same sum with DPP row operations instead of ds_bpermute shuffles (a double is two of them per step, six dependent
// steps): four v_add_f64 on DPP-moved halves give every lane its 16-lane row total, the four row totals are read with
// v_readlane and added in row order.  The total is wave-uniform.  (A different — still fixed — order of fp64 adds.)
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  return ((readlane_f64(v, 0) + readlane_f64(v, 16)) + readlane_f64(v, 32)) + readlane_f64(v, 48);
}

// every workgroup reduces the global partial vector in the same fixed order (wave 0)
struct Sum3 { double a, b, c; };
// (the loads and the sum are separate calls so that a caller can put other loads in flight between them; ALL = false
// reads the first sum of each triple only — the step prologue's error norm.  A loaded-but-unused value is not free here:
// its destination register is reused at once and the reuse waits for the load.)
struct PartLoads { double va[4], vb[4], vc[4]; };
template <bool ALL> __device__ __forceinline__ void part_issue(PartLoads& L, const double* p, int nwg) {
  const int lane = threadIdx.x & 63;
  // agent-scope loads (the vector was written by the previous launch / by RCCL), four workgroups' triples per lane in
  // flight at once: this reduction opens every step launch, one round trip per loop trip was on its critical path.
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = lane + 64 * u;
    const size_t o = (size_t)(i < nwg ? i : 0) * PSTRIDE;
    L.va[u] = __hip_atomic_load(p + o + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ALL) {
      L.vb[u] = __hip_atomic_load(p + o + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      L.vc[u] = __hip_atomic_load(p + o + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
template <bool ALL> __device__ __forceinline__ Sum3 part_finish(const PartLoads& L, const double* p, int nwg) {
  const int lane = threadIdx.x & 63;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  // The adds run in the same order as a plain loop over i = lane, lane + 64, ...
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (lane + 64 * u < nwg) { s0 += L.va[u]; if (ALL) { s1 += L.vb[u]; s2 += L.vc[u]; } }
  for (int i0 = lane + 256; i0 < nwg; i0 += 256) {
    double va[4], vb[4] = {0.0, 0.0, 0.0, 0.0}, vc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 64 * u;
      const size_t o = (size_t)(i < nwg ? i : i0) * PSTRIDE;
      va[u] = __hip_atomic_load(p + o + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ALL) {
        vb[u] = __hip_atomic_load(p + o + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        vc[u] = __hip_atomic_load(p + o + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + 64 * u < nwg) { s0 += va[u]; if (ALL) { s1 += vb[u]; s2 += vc[u]; } }
  }
  // lane totals -> wave total with DPP row operations (wave-uniform result; fp64 sums of fp32 squares: the rounded fp32
  // norm does not depend on the order of these adds)
  Sum3 r;
  r.a = wave_sum_dpp(s0);
  r.b = ALL ? wave_sum_dpp(s1) : 0.0;
  r.c = ALL ? wave_sum_dpp(s2) : 0.0;
  return r;
}
__device__ __forceinline__ Sum3 reduce_partials3(const double* p, int nwg) {
  PartLoads L;
  part_issue<true>(L, p, nwg);
  return part_finish<true>(L, p, nwg);
}

__device__ __forceinline__ float rms_from(double sumsq, double n) { return (float)sqrt(sumsq / n); }

constexpr int SEGK = 7;  // k-groups (of 16 rows) per canonical segment

__device__ __forceinline__ f32x4 mfma4(const f32x4& a, const f32x4& b, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}

}  // namespace
