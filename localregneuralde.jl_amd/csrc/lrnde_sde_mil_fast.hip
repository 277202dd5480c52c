// lrnde_sde_mil_fast.hip — one ATTEMPTED step of the adaptive Milstein solve (RKMilCommute, diagonal noise, Ito:
// src/perform_step.jl:108-170) as ONE launch with the step-size controller in its footer, for the shapes of
// lrnde_sde_fast.hpp (drift Chain(Dense(D => H, act), Dense(H => D)) without a time input, diffusion Dense(D => D),
// D <= 64, H <= 128).  A translation unit of its own: the library calls sde_mil_fast_launch (lrnde_sde_fast.hpp, with the
// argument struct SdeFastArgs); the control block (SdeCtl) is lrnde_stepctl.hpp's, the workgroup frame (SdeFrame: the layout, the
// resident weight fragments, dense1 / diffusion / dense2), the footer (sde_step_footer) and the launch dispatch
// (sde_fast_dispatch) are lrnde_sde_frame.hpp's; nothing goes through global memory between the first load of
// (u, W[i], W[i + m]) and the store of u_new.
// The step is two rounds instead of Euler-Heun's three:
//   1. du1 = f(u), L = g(u)                                  (:130-131)
//   2. gtmp = g(K + sqrt(dt) L),  K = u + dt du1             (:133-138; no drift evaluation: du2 / En are dead code in the
//                                                             reference, lrnde_sde_rkmil_step)
//   then  u_new = (K + L dW) + Dgj J,  Dgj = (gtmp - L) / sqrt(dt),  J = dW^2 / 2 - |dt| / 2          (:117-141)
//   and the residual of the four-argument _calculate_residuals, (u_new - u) / (abstol + max(|u|, |u_new|) reltol)
//   (:166-169, :218-220 — the reference's form, kept as it is).
// Arithmetic: the canonical k-ordered chains and the elementwise expressions of k_sde_rkmil, so u_new and EEst are the bits
// of k_sde_rkmil and of the oracle's rkmil_step.
// Footer: sde_step_footer with one drift evaluation per attempt.  The host keeps launches enqueued (sde_adaptive_device);
// there is no persistent form of this kernel.
#include <hip/hip_runtime.h>

#include "lrnde_sde_frame.hpp"

namespace {

using namespace lrnde;

// TREE: dW from the virtual tree (lrnde_sde_tree.hpp) instead of a.Wpath, recorded beside rec_u.
template <int DT, int HT, bool TREE = false>
__global__ __launch_bounds__(SF_NT) void k_sde_mil_fast(SdeFastArgs a) {
  if (!a.ctl) return;                // (the adaptive loop is this kernel's only caller)
  const SdeCtl cc = *a.ctl;          // written by the previous launch's last workgroup (kernel boundary in between) / by k_sde_ctl_init
  if (cc.status != ST_RUNNING) return;
  const int ad_i = cc.i, ad_m = cc.m, ad_slot = cc.naccept;
  const float dt = (float)ad_m * a.h;
  const float* up = cc.cur ? a.ub : a.ua;
  float* unp = cc.cur ? a.ua : a.ub;
  // LDS: two x tiles in B-operand layout ([kg][64 lanes] float4), the h tile, the diffusion results in C-fragment order
  __shared__ f32x4 xA[DT * 64], xB[DT * 64], hl[HT * 64], gl[DT * 64];
  __shared__ double red[4];
  const SdeFrame<DT, HT> F(a, hl, gl);
  const int lane = F.lane, wave = F.wave, t = F.t, row0 = F.row0, D = F.D;
  const bool has_d2 = F.has_d2, live = F.live;
  const size_t nn = F.nn;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 u4 = zero4, w4 = zero4;
  if (live) {
    u4 = F.ld4s(up);
    if constexpr (TREE) w4 = F.dtree(a.tree, TREE_STREAM_W, ad_i, ad_m);
    else w4 = F.dpath(a.Wpath, ad_i, ad_m);
  }
  if (has_d2) F.put(xA, u4);
  __syncthreads();
  const float sqdt = __builtin_sqrtf(dt), hdt = 0.5f * __builtin_fabsf(dt);
  // ---- round 1: du1 = f(u), L = g(u) (:130-131) ----
  F.dense1(xA);
  F.diffusion(xA);
  __syncthreads();
  f32x4 L = zero4, Kv = zero4;
  if (has_d2) {
    const f32x4 du1 = F.dense2();
    L = gl[t * 64 + lane];
    f32x4 tmp;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Kv[r] = u4[r] + dt * du1[r];          // :133
      tmp[r] = Kv[r] + sqdt * L[r];         // :136-137 (Ito)
    }
    F.put(xB, tmp);
  }
  __syncthreads();
  // ---- round 2: gtmp = g(tmp) (:138) ----
  F.diffusion(xB);
  __syncthreads();
  if (has_d2) {
    const f32x4 gt = gl[t * 64 + lane];
    f32x4 un;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float J = (0.5f * w4[r]) * w4[r] - hdt;                         // :117, :122
      const float Dgj = (gt[r] - L[r]) / sqdt;                              // :139
      un[r] = (Kv[r] + L[r] * w4[r]) + Dgj * J;                             // :141
      if (live && row0 + r < D) {
        const float sc = a.abstol + fmaxf_(__builtin_fabsf(u4[r]), __builtin_fabsf(un[r])) * a.reltol;
        const float rr = (un[r] - u4[r]) / sc;                              // :166, :218-220
        const float sq = rr * rr;
        acc += (double)sq;
      }
    }
    if (live) {
      F.st4s(unp, un);
      if (a.rec_u && ad_slot < a.rec_cap) F.st4s(a.rec_u + (size_t)ad_slot * nn, un);
      if constexpr (TREE) { if (a.tree.rec_dw && ad_slot < a.rec_cap) F.st4s(a.tree.rec_dw + (size_t)ad_slot * nn, w4); }
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) red[wave] = acc;
  }
  __syncthreads();
  sde_step_footer<DT>(a, red, dt, true, 1);
}

}  // namespace

namespace lrnde {

void sde_mil_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f) {
  sde_fast_dispatch(D, H, [&](auto dt, auto ht) {
    if (f.tree.on) hipLaunchKernelGGL((k_sde_mil_fast<dt.value, ht.value, true>), dim3(nwg), dim3(SF_NT), 0, st, f);
    else hipLaunchKernelGGL((k_sde_mil_fast<dt.value, ht.value>), dim3(nwg), dim3(SF_NT), 0, st, f);
  });
}

}  // namespace lrnde
