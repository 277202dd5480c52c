// lrnde_chain_discrete.hpp — the discrete adjoint of a small Dense-chain handle's recorded Tsit5 solve as ONE launch over
// the step record.  Included by lrnde_kernels.hip inside its anonymous namespace, behind
// lrnde_chain_adjoint.hpp (ChAdjSmem, chadj_put, chadj_eval_tail) and lrnde_chain.hpp (tile, layer arithmetic, images).
//
// Semantics (UPSTREAM-RECALL, frozen grid: what a tape — TrackerAdjoint / ReverseDiffAdjoint — gives upstream, where
// DiffEqBase's norm of tracked arrays works on values, so the step-size controller is not differentiated):
//   loss = <cotangents, saved states> (+ w_reg * reg_val, whose gradient stays step_reg_sweep's, added by the caller).
//   The record is lrnde_node_forward_record(_ts)'s: accepted steps n = 0..N-1 with t_n, dt_n (dense_t, dense_dt) and
//   uprev_n, k1_n (the first two of the record's five arrays).  The gradient is the exact derivative of the discrete
//   forward map with the times and step sizes constants; rejected attempts do not appear; FSAL is differentiated
//   (k1_{n+1} is k7_n); a state saved inside a step is that step's Tsit5 interpolant, its cotangent g flows into uprev_n
//   (g) and k1..k7 ((dt * b_i(theta)) g) with theta = (ts - t_n) / dt_n in fp32 and tsit5_bweights, exactly the forward
//   footer's; a state saved at a step's end is a copy of u; a saved start state is a copy of x.
//
// Reverse sweep of a column (lam: cotangent of the state at the current time, kap: cotangent of the next step's k1):
//   lam = sum of the cotangents saved at t2 (descending series index), kap = 0.  For n = N-1 .. 0:
//     1. k2..k6, the stage inputs and u_new from (uprev_n, k1_n) by stage_value / chain_layer (the forward's bits)
//     2. ck[1..6] = 0, ck[7] = kap, cu = 0
//     3. the saves with t_n < ts < t_{n+1}, in descending time: cu = cu + g; ck[i] = ck[i] + (dt * b_i) * g, i = 1..7
//     4. stage 7: w = J(u_new, t + dt)^T ck[7]; lam = lam + w; cu = cu + lam; ck[j] = ck[j] + (dt * a_7j) * lam, j = 1..6
//     5. stages s = 6..2: w = J(g_s, t + c_s dt)^T ck[s]; cu = cu + w; ck[j] = ck[j] + (dt * a_sj) * w, j < s
//     6. lam = cu; for n > 0 the cotangents saved exactly at t_n are added (descending index); kap = ck[1]
//   dx = (lam + J(x, t_0)^T kap) + the cotangents of saved states at or before t_0 (descending index).
//
// Order of accumulation (fixed; no float atomics; two calls give the same bits): every VJP leaves the tile's parameter
// cotangent, the fma chain over the tile's columns in column order (k_vjp_chain's); element q of the workgroup's partial
// vector has one owning thread, which adds the VJPs' values in the order of the sweep: steps newest first, stages 7..2
// inside a step, step 0's k1 last.  k_chain_pgsum then sums the workgroups' partials in workgroup order from 0.
//
// Kernel: k_vjp_chain's grid, one workgroup of NT threads per tile of CNB = 8 columns; each workgroup walks the N steps on
// its own.  No workgroup waits on another, no control block is read, and the loop bounds (N, the number of series times)
// are kernel arguments; the series times are a device table written before the launch.  uprev, k1..k6, ck[1..7], cu and
// lam of a column stay in the registers of its threads (CEPT floats each); the forward weight image is in LDS for the whole
// launch, the backward image too when it fits (ChDiscArgs::wg_lds), and the workgroup's partial vector as well when it
// fits beside both (ChDiscArgs::p_lds), otherwise it is read-modify-written in global memory by its owning threads.

struct ChDiscArgs {
  const float* dense; const float* dense_t; const float* dense_dt;   // the forward's record
  int nrec;              // N
  size_t n_lam;          // B * D
  const float* ser_t;    // [nser] the times of the caller's series, ascending (device)
  const float* du;       // [nser][B*D] their cotangents
  int nser;
  float t2;
  float* lam_out;        // [B*D] dx
  float* gpart;          // [nwg][P]
  int B;
  int wg_lds, gfloats;   // the backward image is copied to LDS too; its length (floats)
  int p_lds;             // the workgroup's parameter partial lives in LDS until the end
};

// dynamic LDS: chain_lds_bytes (lrnde_adj_route.hpp) with this tail behind the images, the record and the partial
constexpr size_t CHDISC_LDS_TAIL = 32;

// the series times by value, up to 64 per launch: no copy from pageable host memory sits in front of the sweep
struct ChDiscBegin { float* dst; int off, n; float v[64]; };
__global__ __launch_bounds__(64) void k_chdisc_begin(ChDiscBegin b) {
  if ((int)threadIdx.x < b.n) b.dst[b.off + threadIdx.x] = b.v[threadIdx.x];
}

__global__ __launch_bounds__(NT) void k_chain_dsweep(ChDiscArgs a, ChainDev cd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  ChAdjSmem s;
  s.w = reinterpret_cast<float*>(smem);
  float* wgl = s.w + cd.wfloats;
  s.v = wgl + (a.wg_lds ? ((a.gfloats + 3) & ~3) : 0);
  float* pl = s.v + cd.gboff + 2 * CMAXW * CNB;
  s.red = nullptr; s.bc = nullptr;
  s.wg = a.wg_lds ? wgl : cd.wg;
  chain_load_weights(cd, s.w);
  if (a.wg_lds)
    for (int i = threadIdx.x; i < a.gfloats; i += NT) wgl[i] = cd.wg[i];
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, a.B - b0);
  const ChainSlots sl = chain_slots(cd.D, b0, nvalid);
  const size_t nst = a.n_lam;
  float* gp = a.p_lds ? pl : a.gpart + (size_t)blockIdx.x * cd.P;
  // the partial vector starts at zero, every element written by the thread that owns it in chadj_eval_tail
  for (int l = 0; l < cd.L; ++l) {
    const int* mt = cd.meta + l * CMETA;
    const int nq = mt[CM_OUT] * (mt[CM_IN] + cd.td) + mt[CM_OUT];
    float* gpl = gp + mt[CM_POFF];
    for (int q = threadIdx.x; q < nq; q += NT) gpl[q] = 0.f;
  }
  float* xa = s.v + cd.gboff;   // the forward recomputation's two activation buffers: the VJP's cotangent buffers
  float* xb = xa + CMAXW * CNB;

  float lam[CEPT], kap[CEPT], up[CEPT], cu[CEPT], w[CEPT], kr[6][CEPT], ck[7][CEPT];
#pragma unroll
  for (int i = 0; i < CEPT; ++i) { lam[i] = 0.f; kap[i] = 0.f; up[i] = 0.f; }
  auto cot = [&](int q, int i) { return sl.valid[i] ? a.du[(size_t)q * nst + sl.g[i]] : 0.f; };
  int q = a.nser - 1;
  for (; q >= 0 && a.ser_t[q] >= a.t2; --q) {
#pragma unroll
    for (int i = 0; i < CEPT; ++i) lam[i] = lam[i] + cot(q, i);
  }
  __syncthreads();

  // J(y, tt)^T c -> w, and the tile's parameter cotangent added to gp
#define LRNDE_CHDISC_VJP(YEXPR, TT, C)                                                          \
  do {                                                                                          \
    _Pragma("unroll") for (int i = 0; i < CEPT; ++i) {                                          \
      if (!sl.in[i]) continue;                                                                  \
      const float y_ = sl.valid[i] ? (YEXPR) : 0.f;                                             \
      chadj_put(cd, s, sl.lidx[i], y_, (C)[i]);                                                 \
    }                                                                                           \
    chadj_eval_tail<true>(cd, s, sl, (TT), w, gp);                                              \
  } while (0)
  // the stage input of stage S from uprev and k1..k(S-1) (stage_value: the forward's expression)
#define LRNDE_CHDISC_X(S) stage_value<S>(up[i], kvs_[i], dt)
#define LRNDE_CHDISC_KV(S)                                                                      \
  float kvs_[CEPT][6];                                                                          \
  _Pragma("unroll") for (int i = 0; i < CEPT; ++i)                                              \
    _Pragma("unroll") for (int j = 0; j < 6; ++j) kvs_[i][j] = kr[j][i];
  // forward stage S: k_S = f(stage input, TS)
#define LRNDE_CHDISC_FWD(S, TS)                                                                 \
  do {                                                                                          \
    LRNDE_CHDISC_KV(S)                                                                          \
    _Pragma("unroll") for (int i = 0; i < CEPT; ++i) {                                          \
      const float x_ = LRNDE_CHDISC_X(S);                                                       \
      if (sl.in[i]) xa[sl.lidx[i]] = sl.valid[i] ? act_apply(cd.in_act, x_) : 0.f;              \
    }                                                                                           \
    __syncthreads();                                                                            \
    const float* r_ = chain_feval(cd, s.w, xa, xb, (TS));                                       \
    _Pragma("unroll") for (int i = 0; i < CEPT; ++i) kr[S - 1][i] = sl.valid[i] ? r_[sl.lidx[i]] : 0.f; \
    __syncthreads();                                                                            \
  } while (0)
  // reverse stage S (2..6): w = J(g_S, TS)^T ck[S]; cu += w; ck[j] += (dt * a_Sj) * w for j < S
#define LRNDE_CHDISC_REV(S, TS)                                                                 \
  do {                                                                                          \
    constexpr int off_ = (S - 2) * (S - 1) / 2;                                                 \
    { LRNDE_CHDISC_KV(S) LRNDE_CHDISC_VJP(LRNDE_CHDISC_X(S), (TS), ck[S - 1]); }                \
    _Pragma("unroll") for (int i = 0; i < CEPT; ++i) {                                          \
      cu[i] = cu[i] + w[i];                                                                     \
      _Pragma("unroll") for (int j = 0; j < S - 1; ++j) ck[j][i] = ck[j][i] + (dt * (float)Tsit5::A[off_ + j]) * w[i]; \
    }                                                                                           \
  } while (0)

  for (int n = a.nrec - 1; n >= 0; --n) {
    const float t = a.dense_t[n], dt = a.dense_dt[n];
    const float* dd = a.dense + (size_t)n * REC_ARRAYS * nst;
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      up[i] = sl.valid[i] ? dd[sl.g[i]] : 0.f;
      kr[0][i] = sl.valid[i] ? dd[nst + sl.g[i]] : 0.f;
#pragma unroll
      for (int j = 1; j < 6; ++j) kr[j][i] = 0.f;
    }
    // 1. the forward's stages (src/perform_step.jl:11-18), the stage times as k_step_chain writes them
    LRNDE_CHDISC_FWD(2, t + (float)Tsit5::C[0] * dt);
    LRNDE_CHDISC_FWD(3, t + (float)Tsit5::C[1] * dt);
    LRNDE_CHDISC_FWD(4, t + (float)Tsit5::C[2] * dt);
    LRNDE_CHDISC_FWD(5, t + (float)Tsit5::C[3] * dt);
    LRNDE_CHDISC_FWD(6, t + dt);
    // 2.
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
#pragma unroll
      for (int j = 0; j < 6; ++j) ck[j][i] = 0.f;
      ck[6][i] = kap[i]; cu[i] = 0.f;
    }
    // 3. the saves strictly inside the step (those at its end were taken when the sweep stood there)
    for (; q >= 0 && a.ser_t[q] > t; --q) {
      const float theta = (a.ser_t[q] - t) / dt;
      float bw[7];
      tsit5_bweights(theta, bw);
#pragma unroll
      for (int i = 0; i < CEPT; ++i) {
        const float g = cot(q, i);
        cu[i] = cu[i] + g;
#pragma unroll
        for (int j = 0; j < 7; ++j) ck[j][i] = ck[j][i] + (dt * bw[j]) * g;
      }
    }
    // 4. stage 7 at u_new
    { LRNDE_CHDISC_KV(7) LRNDE_CHDISC_VJP(LRNDE_CHDISC_X(7), t + dt, ck[6]); }
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      lam[i] = lam[i] + w[i];
      cu[i] = cu[i] + lam[i];
#pragma unroll
      for (int j = 0; j < 6; ++j) ck[j][i] = ck[j][i] + (dt * (float)Tsit5::A[15 + j]) * lam[i];
    }
    // 5.
    LRNDE_CHDISC_REV(6, t + dt);
    LRNDE_CHDISC_REV(5, t + (float)Tsit5::C[3] * dt);
    LRNDE_CHDISC_REV(4, t + (float)Tsit5::C[2] * dt);
    LRNDE_CHDISC_REV(3, t + (float)Tsit5::C[1] * dt);
    LRNDE_CHDISC_REV(2, t + (float)Tsit5::C[0] * dt);
    // 6.
#pragma unroll
    for (int i = 0; i < CEPT; ++i) { lam[i] = cu[i]; kap[i] = ck[0][i]; }
    if (n > 0) {
      for (; q >= 0 && a.ser_t[q] == t; --q) {
#pragma unroll
        for (int i = 0; i < CEPT; ++i) lam[i] = lam[i] + cot(q, i);
      }
    }
  }
  if (a.nrec > 0) {   // k1_0 = f(x, t_0): up holds step 0's uprev
    LRNDE_CHDISC_VJP(up[i], a.dense_t[0], kap);
#pragma unroll
    for (int i = 0; i < CEPT; ++i) lam[i] = lam[i] + w[i];
  }
  for (; q >= 0; --q) {   // a saved start state
#pragma unroll
    for (int i = 0; i < CEPT; ++i) lam[i] = lam[i] + cot(q, i);
  }
#undef LRNDE_CHDISC_REV
#undef LRNDE_CHDISC_FWD
#undef LRNDE_CHDISC_KV
#undef LRNDE_CHDISC_X
#undef LRNDE_CHDISC_VJP
#pragma unroll
  for (int i = 0; i < CEPT; ++i)
    if (sl.valid[i]) a.lam_out[sl.g[i]] = lam[i];
  if (a.p_lds) {
    __syncthreads();
    float* out = a.gpart + (size_t)blockIdx.x * cd.P;
    for (int i = threadIdx.x; i < cd.P; i += NT) out[i] = pl[i];
  }
}
