// lrnde_wide_discrete.hpp — the discrete adjoint of a wide Dense-chain handle's recorded Tsit5 solve.
// Included by lrnde_kernels.hip inside its anonymous namespace, behind lrnde_wide_adjoint.hpp (wadj_each, the stage record's
// use, wadj_mu_item: the block engine of the batch-wide parameter cotangent) and lrnde_chain_discrete.hpp, whose head states
// the method: the frozen grid, FSAL differentiated, saves inside a step by the Tsit5 interpolant, the reverse sweep of a
// column in six numbered steps.  This file runs that sweep for the wide handle; nothing of the method changes.
//
// TWO launches per recorded step, newest step first, all enqueued by the host up front (N is the record's length: no
// controller, no control block, nothing is waited for):
//
//   k_wdisc_step  one workgroup of NT threads per tile of NB = 16 columns (k_vjp_wide's map).  Replay: from (uprev_n, k1_n)
//                 of the dense record the stage inputs g_2..g_6, u_new and k2..k6 by the forward's own expressions
//                 (stage_value<2>, WideStepEpi::stage_x, wdisc_stage_time) through wide_feval WITH a record: every layer's
//                 input and act', act0 and act0' of the stage input, go to the stage record, one slot per stage 2..7.
//                 Reverse, stages 7..2: delta_l = g .* act' written over act' in the slot, g <- W^T delta (wide_gemm on the
//                 transposed image), w = g .* act0', then steps 4 / 5 of the sweep on the vectors.  k2..k6, u_new, ck[1..7]
//                 and cu are B*D vectors in global memory (L2), lam is z[0, B*D); between launches kap lives in ck[1]'s
//                 vector.  Every pass over ck, cu, lam and the cotangents has wadj_each's element map (a thread re-reads
//                 only what it wrote itself, also across launches); k2..k6 and u_new are written and read by the lane that
//                 ends the row quad (WideQuad), as in k_step_wide.
//                 n < 0, the tail: one evaluation at (x, t_0) with a record into slot 0, dx = (lam + J(x, t_0)^T kap) + the
//                 cotangents of a saved start state.
//   k_wdisc_mu    the parameter cotangent over the whole batch from the stage records (k_wadj_mu's work items, one wave
//                 per stage), then for every parameter  acc = mu; acc += K_7; ...; acc += K_2; mu = acc  (the tail: the one
//                 K of (x, t_0)).  The kernel boundary in front of it is the grid-wide dependency on the tiles' records.
//
// Order of accumulation (fixed; no float atomics; two calls give the same bits): steps newest first, stages 7..2, step 0's
// k1 last; K_s the tiles' four-MFMA products added in tile order from 0 (lrnde_wide_adjoint.hpp).  Columns past B carry
// lam = 0 and a zero stage input: they add exact zeros.

constexpr int WDISC_SLOTS = 6;   // stage-record slots: stage S of the step in slot S - 2; the tail's evaluation in slot 0
constexpr int WDISC_VECS = 14;   // B*D vectors beside z: k2..k6 (0..4), u_new (5), ck[1..7] (6..12), cu (13)

struct WDiscArgs {
  const float* dense; const float* dense_t; const float* dense_dt;   // the forward's record
  int nrec;              // N
  size_t n_lam;          // B * D
  const float* ser_t;    // [nser] the times of the caller's series, ascending (device)
  const float* du;       // [nser][B*D] their cotangents
  int nser;
  float t2;
  int B, nwg;
  float* z;              // [B*D + P]: lam, then mu
  float* vec;            // [WDISC_VECS][B*D]
  float* rec;            // [WDISC_SLOTS][nwg][recfloats]
};

// the forward time of stage S = 2..7 of a step (k_step_wide's expression)
__device__ __forceinline__ float wdisc_stage_time(int S, float t, float dt) {
  const float cS = S == 2 ? (float)Tsit5::C[0] : (S == 3 ? (float)Tsit5::C[1] : (S == 4 ? (float)Tsit5::C[2] : (float)Tsit5::C[3]));
  return S >= 6 ? t + dt : t + cS * dt;
}
__device__ __forceinline__ float* wdisc_rec(const WDiscArgs& a, const WideDev& wd, int slot, int tile) {
  return a.rec + ((size_t)slot * a.nwg + tile) * wd.recfloats;
}

// the stage input y(e) of the tile -> act0(y) in the B-fragment tile xl and in the record, act0'(y) in the record
template <class Y> __device__ __forceinline__ void wdisc_stage_in(const WideDev& wd, int b0, int nvalid, float* xl, float* rec, Y&& yv) {
  const int D = wd.D, Dp = (D + 15) & ~15;
  float* ra0 = rec + wd.meta[WM_RAOFF];
  float* rdu = rec + wd.rduoff;
  for (int idx = threadIdx.x; idx < Dp * NB; idx += NT) {
    const int n = idx / Dp, row = idx - n * Dp;
    const bool ok = n < nvalid && row < D;
    const float y = ok ? yv((size_t)(b0 + n) * D + row) : 0.f;
    const float h = ok ? act_apply(wd.in_act, y) : 0.f;
    xl[lds_index(row, n)] = h;
    ra0[row * NB + n] = h;
    rdu[row * NB + n] = ok ? act_deriv_c(wd.in_act, y, h) : 0.f;
  }
}

// w = J^T c from the stage record rec (k_vjp_wide's backward pass; delta_l stays in the act' rows for k_wdisc_mu):
// fin(e, w_e) for every real element of the tile in wadj_each's map.  The LDS buffers are free on entry and on return.
template <class Cot, class Fin>
__device__ __forceinline__ void wdisc_back(const WideDev& wd, const WideSmem& s, int b0, int nvalid, float* rec, Cot&& cot, Fin&& fin) {
  const int D = wd.D;
  float* gc = s.xa;
  float* gn = s.xb;
  wide_stage(D, b0, nvalid, gc, [&](size_t e, int, int) { return cot(e); });
  __syncthreads();
  for (int l = wd.L - 1; l >= 0; --l) {
    const int* mt_ = wd.meta + l * WMETA;
    const int MT = mt_[WM_MT], KG = mt_[WM_KG];
    float* rz = rec + mt_[WM_RZOFF];
    for (int idx = threadIdx.x; idx < MT * 16 * NB; idx += NT) {
      const int li = lds_index(idx >> 4, idx & 15);
      const float d = gc[li] * rz[idx];
      gc[li] = d;
      rz[idx] = d;
    }
    __syncthreads();
    wide_gemm(wd.wg + mt_[WM_GOFF], KG, MT, wd.partcap, gc, s.part, [&](int mt, const f32x4& vv, int ln) {
      float* d = gn + ((mt * 64 + (ln & 15)) << 2) + (ln >> 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) d[r * 64] = vv[r];
    });
    __syncthreads();
    float* tmp = gc; gc = gn; gn = tmp;
  }
  const float* rdu = rec + wd.rduoff;
  wadj_each(D, b0, nvalid, [&](size_t e, int row, int n) { fin(e, gc[lds_index(row, n)] * rdu[row * NB + n]); });
  __syncthreads();
}

__global__ __launch_bounds__(NT) void k_wdisc_step(WDiscArgs a, WideDev wd, int n) {
  const WideSmem s = wide_carve(wd);
  const int D = wd.D;
  const int b0 = blockIdx.x * NB, nvalid = min(NB, a.B - b0);
  const size_t nst = a.n_lam;
  float* const lam = a.z;
  float* const ck = a.vec + 6 * nst;    // ck[j + 1] = ck + j * nst
  float* const cu = a.vec + 13 * nst;
  auto cot = [&](int q, size_t e) { return a.du[(size_t)q * nst + e]; };

  if (n < 0) {   // k1_0 = f(x, t_0): x is step 0's uprev
    const float t0 = a.dense_t[0];
    float* rec = wdisc_rec(a, wd, 0, blockIdx.x);
    float* src = s.xa;
    float* dst = s.xb;
    wdisc_stage_in(wd, b0, nvalid, src, rec, [&](size_t e) { return a.dense[e]; });
    __syncthreads();
    wide_feval(wd, s, src, dst, t0, rec, [&](int, int, const f32x4&) {});
    __syncthreads();
    wdisc_back(wd, s, b0, nvalid, rec, [&](size_t e) { return ck[e]; }, [&](size_t e, float w) {
      float v = lam[e] + w;
      for (int q = a.nser - 1; q >= 0; --q)   // a saved start state
        if (a.ser_t[q] <= t0) v = v + cot(q, e);
      lam[e] = v;
    });
    return;
  }

  const float t = a.dense_t[n], dt = a.dense_dt[n];
  const bool newest = n + 1 == a.nrec;
  const float tend = newest ? a.t2 : a.dense_t[n + 1];
  const float* dd = a.dense + (size_t)n * REC_ARRAYS * nst;
  // 2., 3. ck[1..6] = 0, ck[7] = kap, cu = 0, then the saves strictly inside the step in descending order (those at its end
  // were taken when the sweep stood there; the newest step first takes the ones at t2 into lam)
  wadj_each(D, b0, nvalid, [&](size_t e, int, int) {
    float c[7], cuv = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) c[j] = 0.f;
    c[6] = newest ? 0.f : ck[e];
    if (newest) {
      float l0 = 0.f;
      for (int q = a.nser - 1; q >= 0 && a.ser_t[q] >= a.t2; --q) l0 = l0 + cot(q, e);
      lam[e] = l0;
    }
    for (int q = a.nser - 1; q >= 0 && a.ser_t[q] > t; --q) {
      if (!(a.ser_t[q] < tend)) continue;
      const float theta = (a.ser_t[q] - t) / dt;
      float bw[7];
      tsit5_bweights(theta, bw);
      const float g = cot(q, e);
      cuv = cuv + g;
#pragma unroll
      for (int j = 0; j < 7; ++j) c[j] = c[j] + (dt * bw[j]) * g;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) ck[(size_t)j * nst + e] = c[j];
    cu[e] = cuv;
  });

  // 1. the forward's stages with a record
  WideStepEpi ep;
  ep.uprev = dd; ep.unew = a.vec + 5 * nst; ep.k1 = dd + nst; ep.k7 = nullptr; ep.ks0 = a.vec; ep.g6 = nullptr; ep.nst = nst;
  ep.dt = dt; ep.abstol = 0.f; ep.reltol = 0.f;
  ep.want_stiff = 0; ep.in_act = wd.in_act; ep.D = D; ep.b0 = b0; ep.nvalid = nvalid; ep.v4 = (D & 3) == 0;
  float* src = s.xa;
  float* dst = s.xb;
  wdisc_stage_in(wd, b0, nvalid, src, wdisc_rec(a, wd, 0, blockIdx.x), [&](size_t e) {
    const float kv = ep.k1[e];
    return stage_value<2>(ep.uprev[e], &kv, dt);
  });
  __syncthreads();
#pragma unroll 1
  for (int S = 2; S <= 7; ++S) {
    const float ts = wdisc_stage_time(S, t, dt);
    float* rec = wdisc_rec(a, wd, S - 2, blockIdx.x);
    float* recn = wdisc_rec(a, wd, S < 7 ? S - 1 : S - 2, blockIdx.x);   // the next stage's slot takes its input
    wide_feval(wd, s, src, dst, ts, rec, [&](int mt, int l, const f32x4& kv) {
      if (S == 7) return;   // (k7 itself is not needed: only the record at u_new)
      const WideQuad q = wide_quad(mt, l, D, b0, nvalid);
      f32x4 x;
      switch (S) {   // (uniform over the workgroup)
        case 2: x = ep.stage_x<2>(q, kv); break;
        case 3: x = ep.stage_x<3>(q, kv); break;
        case 4: x = ep.stage_x<4>(q, kv); break;
        case 5: x = ep.stage_x<5>(q, kv); break;
        default: x = ep.stage_x<6>(q, kv); break;
      }
      wide_put(dst, mt, q, wd.in_act, x);
      float* ra0 = recn + wd.meta[WM_RAOFF] + q.row0 * NB + q.n;
      float* rdu = recn + wd.rduoff + q.row0 * NB + q.n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = r < q.nrow;
        const float h = ok ? act_apply(wd.in_act, x[r]) : 0.f;
        ra0[r * NB] = h;
        rdu[r * NB] = ok ? act_deriv_c(wd.in_act, x[r], h) : 0.f;
      }
    });
    __syncthreads();
    float* tmp = src; src = dst; dst = tmp;
  }

  // 4. stage 7 at u_new: lam = lam + w; cu = cu + lam; ck[j] = ck[j] + (dt * a_7j) * lam
  wdisc_back(wd, s, b0, nvalid, wdisc_rec(a, wd, 5, blockIdx.x), [&](size_t e) { return ck[6 * nst + e]; }, [&](size_t e, float w) {
    const float lv = lam[e] + w;
    cu[e] = cu[e] + lv;
#pragma unroll
    for (int j = 0; j < 6; ++j) ck[(size_t)j * nst + e] = ck[(size_t)j * nst + e] + (dt * (float)Tsit5::A[15 + j]) * lv;
  });
  // 5. stages 6..2: cu = cu + w; ck[j] = ck[j] + (dt * a_Sj) * w for j < S; 6. after stage 2: lam = cu plus the cotangents
  // saved exactly at t_n (n > 0), kap = ck[1] (it stays in its vector)
#pragma unroll 1
  for (int S = 6; S >= 2; --S) {
    const int off = (S - 2) * (S - 1) / 2;
    wdisc_back(wd, s, b0, nvalid, wdisc_rec(a, wd, S - 2, blockIdx.x), [&](size_t e) { return ck[(size_t)(S - 1) * nst + e]; },
               [&](size_t e, float w) {
      float cv = cu[e] + w;
      for (int j = 0; j < S - 1; ++j) ck[(size_t)j * nst + e] = ck[(size_t)j * nst + e] + (dt * (float)Tsit5::A[off + j]) * w;
      if (S > 2) { cu[e] = cv; return; }
      if (n > 0)
        for (int q = a.nser - 1; q >= 0 && a.ser_t[q] >= t; --q)
          if (a.ser_t[q] == t) cv = cv + cot(q, e);
      lam[e] = cv;
    });
  }
}

// grid: min(work items, CHADJ_MAX_MU_BLOCKS) workgroups of WADJ_MU_NT threads; wave s < 6 forms stage s + 2 (n < 0: wave 0
// the tail's evaluation)
__global__ __launch_bounds__(WADJ_MU_NT) void k_wdisc_mu(WDiscArgs a, WideDev wd, int nitems, int n) {
  constexpr int NBLK = WADJ_MB * WADJ_MB;
  __shared__ float ks[7][NBLK * 256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool step = n >= 0;
  const bool active = wave < (step ? WDISC_SLOTS : 1);
  const float ts = step ? wdisc_stage_time(wave + 2, a.dense_t[n], a.dense_dt[n]) : a.dense_t[0];
  const float* slot0 = wdisc_rec(a, wd, active ? wave : 0, 0);
  float* mu = a.z + a.n_lam;
  auto finish = [&](size_t i, int e) {
    float acc = mu[i];
    if (step) {
#pragma unroll
      for (int q = WDISC_SLOTS - 1; q >= 0; --q) acc = acc + ks[q][e];   // stages 7..2
    } else {
      acc = acc + ks[0][e];
    }
    mu[i] = acc;
  };
#pragma unroll 1
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    wadj_mu_item(wd, slot0, a.nwg, active, wave, lane, ts, it, ks, finish);
    __syncthreads();
  }
}
