// lrnde_sde_eh_fast.hip — the Lamba Euler-Heun step (src/perform_step.jl:172-206) as ONE small-latency launch, for every
// NeuralDSDE whose drift is Chain(Dense(D => H, act), Dense(H => D)) without a time input and whose diffusion is
// Dense(D => D) (src/layers/neural_sde.jl:50-72; experiments/src/construct.jl:204-205 is D = 32, H = 64) with D <= 64 and
// H <= 128.  A translation unit of its own: the library calls sde_fast_launch / sde_persist_launch (lrnde_sde_fast.hpp), the
// kernel is written on the workgroup frame of lrnde_sde_frame.hpp.
//
// k_sde_step (the generic kernel) runs the step's six field evaluations through feval_tile: per evaluation it restages
// the biases, reloads the resident weight fragments from L2, and passes every intermediate (du1, L, K, tmp, ...) through
// global memory between evaluations — 28 us for 15.7 MFLOP.  Here nothing leaves the CU between the first load of (u, dW) and
// the store of u_new: the weights are resident fragments of the workgroup frame (SdeFrame, where the layout is described);
// a round = [drift Dense-1 + activation, and this wave's diffusion tile] barrier [drift Dense-2 of this wave's tile + the
// elementwise algebra] barrier; the step is three rounds: (f,g)(u) -> (f,g)(tmp) -> f(K), g(utilde).
// Arithmetic: the canonical dot products (k-ordered fma chains = v_mfma_f32_16x16x4_f32 chains over the k-groups in
// order, segments of 112 rows added left to right — H = 128 has two), the same activation polynomial and the same
// elementwise expressions as k_sde_step, so results are bit-identical to it and to the oracle
// (tests/test_gpu_parity.py::test_sde_*, tests/test_gpu_switches.py).  Rows beyond D / H are zero-padded fragments.
//
// The adaptive solve's controller (lrnde_sde_solve_adaptive, lrnde_sde_node_forward_record) runs in this kernel's footer
// (last workgroup to arrive): PI controller on EEst, position on the caller's Brownian grid, state buffer flip, and — for
// the layer's recorded forward — the dense record of the accepted steps (start index, length, end state) that the
// reverse sweep of lrnde_sde_node_backward_recorded walks.
#include <hip/hip_runtime.h>

#include "lrnde_sde_frame.hpp"

namespace {

using namespace lrnde;

// PERSIST: the whole adaptive solve in ONE cooperative launch.  The workgroups stay resident with their weight fragments and
// their columns' state in registers; a step ends in a grid barrier (tagged partial-sum slots + bounded polling) after which EVERY
// workgroup adds the partial sums in the same fixed order and runs the same controller on its own copy of the control
// block — the same decisions everywhere, no broadcast, and the arithmetic of a step is the code of the one-launch form.
// TREE: the adaptive solve's increments come from the virtual tree instead of a.Wpath, the descent spread over all four waves
// (F.wtree_fill -> 1 KB of LDS per 16 rows -> F.wtree_rd behind the step's first barrier).  W[i] is carried in registers: an
// accepted step's W[i + m] is the next step's W[i], a rejected step keeps it — one descent per attempt in the persistent form.
template <int DT, int HT, bool PERSIST = false, bool TREE = false>
__global__ __launch_bounds__(SF_NT) void k_sde_eh_fast(SdeFastArgs a) {
  const bool adapt = a.ctl != nullptr;
  int ad_i = 0, ad_m = 0, ad_slot = 0;
  SdeCtl cc{};
  if (adapt) {
    cc = *a.ctl;   // written by the previous launch's last workgroup (kernel boundary in between) / by k_sde_ctl_init
    if (cc.status != ST_RUNNING) return;
    ad_i = cc.i; ad_m = cc.m; ad_slot = cc.naccept;
    a.dt = (float)ad_m * a.h;
    a.u = cc.cur ? a.ub : a.ua;
    a.un = cc.cur ? a.ua : a.ub;
  } else if (a.dt_dev) a.dt = *a.dt_dev;
  __shared__ SdeCtl sh_cc;
  // LDS: three x tiles in B-operand layout (16 DT rows x 16 columns each: [kg][64 lanes] float4), the h tile, the
  // diffusion results in C-fragment order, the reduction scratch
  __shared__ f32x4 xA[DT * 64], xB[DT * 64], xC[DT * 64], hl[HT * 64], gl[DT * 64];
  __shared__ double red[4];
  const SdeFrame<DT, HT> F(a, hl, gl);
  const int lane = F.lane, wave = F.wave, t = F.t, row0 = F.row0, D = F.D;
  const bool has_d2 = F.has_d2, live = F.live;
  const size_t nn = F.nn;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 u4 = zero4, w4 = zero4;
  [[maybe_unused]] f32x4 wlo4 = zero4, whi4 = zero4;
  if (live) u4 = F.ld4s(a.u);
  [[maybe_unused]] float* wt = nullptr;   // TREE: W[k] of the workgroup's 16 DT x 16 tile
  if constexpr (TREE) {
    __shared__ float wt_[DT * 256];
    wt = wt_;
    if (adapt) {   // W[i] at the launch's position (zero without a descent at i = 0)
      F.wtree_fill(a.tree, TREE_STREAM_W, ad_i, a.B, wt);
      __syncthreads();
      if (live) wlo4 = F.wtree_rd(wt);
      __syncthreads();   // (wt is refilled below)
    }
  }
  for (int it = 0;; ++it) {   // (one trip unless PERSIST)
  SDE_STAMP(0);
  if constexpr (TREE) { if (adapt) F.wtree_fill(a.tree, TREE_STREAM_W, ad_i + ad_m, a.B, wt); }   // (every thread; read behind the barrier below)
  if (live) {
    if (adapt) {  // dW = W[i + m] - W[i], the path's own increment (the expression of k_sde_dw)
      if constexpr (!TREE) w4 = F.dpath(a.Wpath, ad_i, ad_m);
    } else {
      w4 = F.ld4s(a.dW);
      if (a.dW_scaled) {
        const float cz = __builtin_sqrtf(a.dt);
#pragma unroll
        for (int r = 0; r < 4; ++r) w4[r] = cz * w4[r];
        F.st4s(a.dW_scaled, w4);
      }
    }
  }
  if (has_d2) F.put(xA, u4);
  __syncthreads();
  if constexpr (TREE) {
    if (adapt && live) {   // (wt is next written at the top of the next step, barriers away)
      whi4 = F.wtree_rd(wt);
#pragma unroll
      for (int r = 0; r < 4; ++r) w4[r] = whi4[r] - wlo4[r];
    }
  }
  const float dt = a.dt, hdt = dt / 2.0f, sqdt = __builtin_sqrtf(dt);

  if constexpr (!PERSIST) {
    if (a.idt_phase) {
      // StochasticDiffEq.sde_determine_initdt's evaluations and norms (UPSTREAM-RECALL; the expressions of k_sde_initdt):
      // phase 1: f0 = f(u), g0 = g(u) -> sums of (u / sk)^2 and (max(|f0 + 3 g0|, |f0 - 3 g0|) / sk)^2;
      // phase 2: dt0 from phase 1's sums (every workgroup adds them in the same fixed order), u1 = u + dt0 f0, f1, g1 ->
      //          sum of (max(|df + dg|, |df - dg|) / sk)^2.  The launch ends here.
      __shared__ double red2[4];
      __shared__ float sh_dt0;
      F.dense1(xA);
      F.diffusion(xA);
      __syncthreads();
      f32x4 f0 = zero4, g0 = zero4;
      if (has_d2) { f0 = F.dense2(); g0 = gl[t * 64 + lane]; }
      double a0 = 0.0, a1 = 0.0;
      if (a.idt_phase == 1) {
        if (live) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (row0 + r >= D) continue;
            const float sk = a.abstol + __builtin_fabsf(u4[r]) * a.reltol;
            const float G0 = 3.0f * g0[r];
            const float r0 = u4[r] / sk;
            const float r1 = fmaxf_(__builtin_fabsf(f0[r] + G0), __builtin_fabsf(f0[r] - G0)) / sk;
            a0 += (double)(r0 * r0); a1 += (double)(r1 * r1);
          }
        }
      } else {
        if (threadIdx.x < 64) {
          const Sum3 s = reduce_partials3(a.idt_part, (int)gridDim.x);
          if (lane == 0) {
            const float d0 = (float)sqrt(s.a / a.n_norm), d1 = (float)sqrt(s.b / a.n_norm);
            const float dt0 = initdt_dt0(d0, d1, a.idt_dtmax);
            sh_dt0 = dt0;
            if (blockIdx.x == 0) { a.idt_scal[0] = dt0; a.idt_scal[1] = d1; }
          }
        }
        __syncthreads();
        const float dt0 = sh_dt0;
        if (has_d2) {
          f32x4 u1;
#pragma unroll
          for (int r = 0; r < 4; ++r) u1[r] = u4[r] + dt0 * f0[r];
          F.put(xB, u1);
        }
        __syncthreads();
        F.dense1(xB);
        F.diffusion(xB);
        __syncthreads();
        if (has_d2) {
          const f32x4 f1 = F.dense2();
          const f32x4 g1 = gl[t * 64 + lane];
          if (live) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (row0 + r >= D) continue;
              const float sk = a.abstol + __builtin_fabsf(u4[r]) * a.reltol;
              const float G0 = 3.0f * g0[r], G1 = 3.0f * g1[r];
              const float dg = fmaxf_(__builtin_fabsf(G0 - G1), __builtin_fabsf(G0 + G1));
              const float df = f1[r] - f0[r];
              const float r2 = fmaxf_(__builtin_fabsf(df + dg), __builtin_fabsf(df - dg)) / sk;
              a0 += (double)(r2 * r2);
            }
          }
        }
      }
      if (has_d2) {
        a0 = wave_sum_dpp(a0); a1 = wave_sum_dpp(a1);
        if (lane == 0) { red[wave] = a0; red2[wave] = a1; }
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        double t0s = red[0], t1s = red2[0];
#pragma unroll
        for (int w = 1; w < DT; ++w) { t0s += red[w]; t1s += red2[w]; }
        double* pp = (a.idt_phase == 1 ? a.idt_part : a.idt_part2) + (size_t)blockIdx.x * PSTRIDE;
        pp[0] = t0s; pp[1] = t1s; pp[2] = 0.0;
      }
      return;
    }
  }
  SDE_STAMP(1);
  // ---- round 1: du1 = f(u), L = g(u) (:174-176) ----
  F.dense1(xA);
  SDE_STAMP(8);
  F.diffusion(xA);
  SDE_STAMP(9);
  __syncthreads();
  SDE_STAMP(10);
  f32x4 du1 = zero4, L = zero4, Kv = zero4;
  if (has_d2) {
    du1 = F.dense2();
    SDE_STAMP(11);
    L = gl[t * 64 + lane];
    f32x4 tmp, ut;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Kv[r] = u4[r] + dt * du1[r];          // :175
      tmp[r] = Kv[r] + L[r] * w4[r];        // :179,183
      ut[r] = u4[r] + L[r] * sqdt;          // :196
    }
    F.put(xB, tmp); F.put(xC, ut);
  }
  SDE_STAMP(12);
  __syncthreads();
  SDE_STAMP(2);
  // ---- round 2: g(tmp), f(tmp) at t + dt (:184, :191) ----
  F.dense1(xB);
  F.diffusion(xB);
  __syncthreads();
  f32x4 un = zero4;
  if (has_d2) {
    const f32x4 f2 = F.dense2();
    const f32x4 g2 = gl[t * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gtmp2 = 0.5f * (L[r] + g2[r]);
      const float noise2 = gtmp2 * w4[r];
      un[r] = (u4[r] + hdt * (du1[r] + f2[r])) + noise2;   // :191
    }
    if (live) {
      if (!PERSIST) F.st4s(a.un, un);   // (PERSIST: the state lives in registers until the solve ends)
      if (a.rec_u && ad_slot < a.rec_cap) F.st4s(a.rec_u + (size_t)ad_slot * nn, un);
      if constexpr (TREE) { if (a.tree.rec_dw && ad_slot < a.rec_cap) F.st4s(a.tree.rec_dw + (size_t)ad_slot * nn, w4); }
    }
    F.put(xA, Kv);   // xA is free: every wave has read it (barrier above)
  }
  __syncthreads();
  SDE_STAMP(3);
  // ---- round 3: du2 = f(K, t + dt) (:193), g(utilde, t) (:197) ----
  F.dense1(xA);
  F.diffusion(xC);
  __syncthreads();
  double acc = 0.0;
  if (has_d2) {
    const f32x4 du2 = F.dense2();
    const f32x4 g3 = gl[t * 64 + lane];
    if (live) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (row0 + r >= D) continue;
        const float Ed = (dt * (du2[r] - du1[r])) / 2.0f;                        // :194
        const float ggp = (g3[r] - L[r]) / sqdt;                                 // :197
        const float En = (ggp * (w4[r] * w4[r])) / 2.0f;                         // :198
        const float sc = a.abstol + fmaxf_(__builtin_fabsf(u4[r]), __builtin_fabsf(un[r])) * a.reltol;
        const float rr = (a.delta * Ed + En) / sc;                               // :214-216
        const float sq = rr * rr;
        acc += (double)sq;
      }
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) red[wave] = acc;
  }
  __syncthreads();
  SDE_STAMP(4);
  if constexpr (PERSIST) {
    const int nwg = (int)gridDim.x + a.dbg_stall;
    double* blk = a.part2 + (size_t)(it & 1) * nwg * PSTRIDE;   // (two blocks: a fast workgroup's next step must not overwrite what a slow one still reads)
    if (threadIdx.x < 64) {
      // The step's grid barrier IS the exchange of the partial sums: a workgroup publishes {sum, tag} as ONE 16-byte agent-scope
      // store — tag = step number and a checksum of the sum's bits, so that a reader can tell a slot of this step from a stale
      // or (should a 16-byte access ever be split) a torn one — and every workgroup polls all slots with 16-byte loads until
      // each carries this step's tag.  Two trips past the L2 per step (publish, poll) instead of four (store, arrive, poll,
      // read).  Bounded: 50 ms on the 100-MHz clock, then the solve ends with an error instead of hanging the queue.
      typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
      const unsigned step_tag = (unsigned)(it + 1);
      if (lane == 0) {
        const unsigned long long vb = __builtin_bit_cast(unsigned long long, sde_wg_total<DT>(red));
        const u32x4_ w = {(unsigned)vb, (unsigned)(vb >> 32), (unsigned)(vb >> 32) ^ (unsigned)vb, step_tag};
        double* p = blk + (size_t)blockIdx.x * PSTRIDE;
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(w) : "memory");
      }
      float qpow = fastpow(cc.qold, a.beta2);   // (ahead of the wait: see sde_ctl_update)
      asm volatile("" : "+v"(qpow));              // (pinned here: the value is only used after the polling loop)
      PartLoads L;
      const unsigned long long t0c = __builtin_amdgcn_s_memrealtime();
      bool ok = true;
      for (;;) {
        u32x4_ v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = lane + 64 * u;
          const double* p = blk + (size_t)(i < nwg ? i : 0) * PSTRIDE;
          asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v[u]) : "v"(p) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bool good = true;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          asm volatile("" : "+v"(v[u]));
          const bool mine = lane + 64 * u < nwg;
          good = good && (!mine || (v[u].w == step_tag && v[u].z == (v[u].x ^ v[u].y)));
          L.va[u] = __builtin_bit_cast(double, (unsigned long long)v[u].x | ((unsigned long long)v[u].y << 32));
        }
        if (__ballot(good) == ~0ull) break;
        if (__builtin_amdgcn_s_memrealtime() - t0c > 5000000ull) { ok = false; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      SDE_STAMP(5);
      SdeCtl c2 = cc;
      if (!ok) c2.status = LRNDE_HIP_ERROR;
      else {
        const Sum3 s3 = part_finish<false>(L, blk, nwg);   // (the fixed order of every reduction of these partials)
        const float eest = rms_from(s3.a, a.n_norm);
        sde_ctl_update(c2, eest, dt, a, blockIdx.x == 0 && lane == 0, qpow, 3);
      }
      if (lane == 0) sh_cc = c2;
    }
    __syncthreads();
    SDE_STAMP(6);
    const int nacc0 = cc.naccept;
    cc = sh_cc;
    if constexpr (TREE) { if (cc.naccept != nacc0) wlo4 = whi4; }
    if (cc.naccept != nacc0) u4 = un;   // accepted: the end state is the next step's start state (rows of the Dense-2 waves)
    if (cc.status != ST_RUNNING) {
      if (live) F.st4s(cc.cur ? a.ub : a.ua, u4);
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        *a.ctl = cc;
        __hip_atomic_store(a.prog, sde_report_pack((unsigned)(it + 1), (unsigned)cc.status),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      return;
    }
    ad_i = cc.i; ad_m = cc.m; ad_slot = cc.naccept;
    a.dt = (float)ad_m * a.h;
    continue;
  } else {
  if (a.march_n > 0) {
    if (threadIdx.x == 0) {
      double* p = a.march_part + ((size_t)it * gridDim.x + blockIdx.x) * PSTRIDE;
      p[0] = sde_wg_total<DT>(red); p[1] = 0.0; p[2] = 0.0;
    }
    if (it + 1 == a.march_n) return;
    u4 = un;                       // the end state is the next step's start state (rows of the Dense-2 waves)
    a.dW += nn; a.un += nn;
    __syncthreads();               // red and the tiles are rewritten by the next step
    continue;
  }
  if (!a.arrive) {   // (a single step whose caller reduces the partials)
    if (threadIdx.x == 0) { double* p = a.part + (size_t)blockIdx.x * PSTRIDE; p[0] = sde_wg_total<DT>(red); p[1] = 0.0; p[2] = 0.0; }
    return;
  }
  sde_step_footer<DT>(a, red, dt, adapt, 3);   // fills the fixed-grid record / runs the controller
  return;
  }
  }   // for (it)
}

}  // namespace

namespace lrnde {

void sde_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f) {
  sde_fast_dispatch(D, H, [&](auto dt, auto ht) {
    if (f.tree.on) hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value, false, true>), dim3(nwg), dim3(SF_NT), 0, st, f);
    else hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value>), dim3(nwg), dim3(SF_NT), 0, st, f);
  });
}

// the persistent form.  coop: a cooperative launch (all workgroups resident, or the call fails and the caller takes the
// launch-per-step loop) — the API's guarantee costs 25-30 us per launch; !coop: a plain launch, for grids far smaller than the
// chip, whose barrier is bounded (a workgroup that waits 50 ms for the others ends the solve with an error and the caller runs
// the loop instead).  Returns the launch's hipError_t.
hipError_t sde_persist_launch(int D, int H, int nwg, hipStream_t st, SdeFastArgs& f, bool coop) {
  hipError_t e = hipErrorInvalidValue;   // (a shape outside the gate: nothing is launched)
  sde_fast_dispatch(D, H, [&](auto dt, auto ht) {
    void* args[] = {&f};
    if (f.tree.on) {
      if (!coop) { hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value, true, true>), dim3(nwg), dim3(SF_NT), 0, st, f); e = hipGetLastError(); }
      else e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(k_sde_eh_fast<dt.value, ht.value, true, true>), dim3(nwg), dim3(SF_NT), args, 0, st);
    } else
    if (!coop) { hipLaunchKernelGGL((k_sde_eh_fast<dt.value, ht.value, true>), dim3(nwg), dim3(SF_NT), 0, st, f); e = hipGetLastError(); }
    else e = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(k_sde_eh_fast<dt.value, ht.value, true>), dim3(nwg), dim3(SF_NT), args, 0, st);
  });
  return e;
}

}  // namespace lrnde
