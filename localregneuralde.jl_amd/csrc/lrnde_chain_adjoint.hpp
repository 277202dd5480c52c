// lrnde_chain_adjoint.hpp — the continuous adjoint of a Dense-chain handle with the controller on the device
// (DESIGN.md 4.9.1).  Included by lrnde_kernels.hip inside its anonymous namespace, behind lrnde_adjoint.hpp (AdjCtrl,
// AdjStage, AdjArgs, the pinned progress word) and lrnde_chain.hpp (tile, layer arithmetic, weight images).
//
// The reversed-time Tsit5 solve on z = [lambda (B*D); mu (P)] that vec_tsit5_solve + adj_rhs run with ~20 launches and
// a norm read-back per attempted step, in TWO launches per attempted step and no host wait:
//
//   k_chadj_step  one workgroup of NT threads per tile of CNB = 8 batch columns (k_vjp_chain's column -> workgroup map).
//                 Wave 0 runs the footer of attempt j-1 and the header of attempt j (chadj_prologue: adj_prologue's
//                 controller, plus the cotangent impulses, which do not end a segment here); block 0 publishes it.
//                 Then the six stages: stage lambda from z and the earlier K's (k_axpy's expression), y(t) from the
//                 dense record, forward through the L layers keeping every layer's input and act' in LDS, backward
//                 (delta = g .* act', g <- W^T delta) and the tile's parameter cotangent in Lux order.  lambda, the
//                 stage lambdas and the lambda parts of K1..K7 of a column stay in the registers of its threads; the
//                 forward weight image is in LDS, the backward image too when it fits (ChAdjArgs::wg_lds).
//   k_chadj_mu    mu never feeds the right-hand side, so nothing between the stages needs a grid-wide sum: the step
//                 kernel leaves one partial vector per (stage, workgroup) in gpart, and this launch sums them, forms the
//                 mu part of z_new, of K7 (the next attempt's K1) and of utilde, and the mu partials of the error norm.
//
// Summation order (fixed; no float atomics): a tile's parameter cotangent is the fma chain over its columns in column
// order (k_vjp_chain's); the mu part of K_s is the sum of the tiles' partials in workgroup order, from 0 (k_chain_pgsum's
// order, so K_s has the bits the host loop gives it); the stages enter mu_new and utilde in the order s = 1..7 of k_axpy
// (s = c_1 K_1; s = s + c_j K_j).  The error norm's fp64 partials (one per workgroup of each launch) are summed
// lane-strided in index order and by wave_sum_dpp's tree.
//
// Buffers: z / z_new = adj_zb(g, cur / cur^1), K1 / K7 = adj_K(g, 0 / 6, cur) of the handle's adjoint allocation;
// gpart [7][nwg][P] floats (slot 0: a re-evaluated K1 and initdt's two evaluations, slots 1..6: stages 2..7);
// dpart [5][np] doubles, np = nwg + nmu (sets 0..2: initdt's d0, d1, d2; sets 3 + (j & 1): attempt j's error norm,
// double-buffered because a fast workgroup of attempt j writes while a slow one still reads attempt j-1's).

struct ChAdjImp { float s; const float* du; };  // a cotangent added to lambda when the reversed solve lands on s

struct ChAdjCtrl {
  AdjCtrl c;
  int iimp;        // impulses before this index have been passed
  int hit;         // the step accepted by this prologue landed on impulses [imp0, imp1): lambda += du, K1 re-evaluated
  int imp0, imp1;
  AdjStage st_hit; // the dense-record position of that re-evaluation
  // the wide handle's stage record (lrnde_wide_adjoint.hpp): the slot that holds K1's evaluation and its forward time
  int k1slot; float k1t;
};

struct ChAdjArgs {
  AdjArgs g;             // (g.ctl, g.part, g.ipart, g.sync are not used here)
  ChAdjCtrl* cc;         // [2], by attempt parity
  const ChAdjImp* imp; int nimp;   // s0 < s < s1, ascending (device)
  float* gpart;          // [7][nwg][P]
  double* dpart;         // [5][np]
  int B, nwg, nmu, np;
  int wg_lds;            // the backward weight image is copied to LDS too
  int gfloats;           // its length (floats)
};

enum { CHADJ_STEP = 0, CHADJ_INIT_A = 1, CHADJ_INIT_B = 2 };
constexpr int CHADJ_MU_NT = 7 * 64;          // k_chadj_mu: wave w sums slot w
// (CHADJ_MAX_WG, CHADJ_MAX_MU_BLOCKS, CHADJ_LDS_MAX, CHADJ_SCRATCH_MAX: the gate's limits, lrnde_adj_route.hpp)

__device__ __forceinline__ double* chadj_set(const ChAdjArgs& a, int set) { return a.dpart + (size_t)set * a.np; }

// sum of one set of norm partials (wave 0; every lane returns the total): lane-strided in index order, then the DPP tree
__device__ __forceinline__ double chadj_sum(const double* p, int n) {
  double s = 0.0;
  for (int i = threadIdx.x & 63; i < n; i += 64) s += p[i];
  return wave_sum_dpp(s);
}

__device__ __forceinline__ void chadj_report(const ChAdjArgs& a, const ChAdjCtrl& c, int j) {
  a.cc[(j + 1) & 1] = c;
  if (a.g.hstat) {
    adj_hstat_fill(a.g.hstat, c.c);
    __hip_atomic_store(a.g.hstat + ADJ_R_SEQ, a.g.seq0 + j + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// footer of attempt j-1 + header of attempt j (wave 0 of every workgroup, identical inputs => identical results):
// adj_prologue's, with the cotangent impulses handled in place
__device__ __forceinline__ ChAdjCtrl chadj_prologue(const ChAdjArgs& a, int j) {
  const AdjArgs& g = a.g;
  const int lane = threadIdx.x & 63;
  ChAdjCtrl cc = a.cc[j & 1];
  AdjCtrl& c = cc.c;
  const AdjRecLanes rec = adj_rec_load(g);
  const float stop_l = (lane < g.nstops) ? g.stops[lane] : 3.0e38f;
  const bool pub = blockIdx.x == 0 && lane == 0;
  c.do_step = 0; cc.hit = 0;
  if (c.status != ST_RUNNING) {
    if (pub) chadj_report(a, cc, j);
    return cc;
  }
  const PiConsts pi = pi_tsit5();
  const float dtmax = g.dtmax, dtmin = g.dtmin;
  const double ntot = (double)g.n_lam + (double)g.P;
  float t = c.t, dt = c.dt;
  if (c.first) {
    // ode_determine_initdt from the partial sums of d0, d1 (dt0, as init phase B formed it) and d2
    const float d0 = (float)sqrt(chadj_sum(chadj_set(a, 0), a.np) / ntot);
    const float d1 = (float)sqrt(chadj_sum(chadj_set(a, 1), a.np) / ntot);
    const float d2 = (float)sqrt(chadj_sum(chadj_set(a, 2), a.np) / ntot);
    const float dt0 = initdt_dt0(d0, d1, dtmax);
    dt = initdt_tail(dt0, d1, d2, 5.0f, dtmax);
    c.dt0 = dt0; c.nf = 3; c.dt_init = dt; c.dtpropose = dt;
    c.qold = QOLDINIT; c.q11 = 1.0f;
  } else {
    const float eest = (float)sqrt(chadj_sum(chadj_set(a, 3 + ((j + 1) & 1)), a.np) / ntot);
    c.eest_last = eest;
    if (eest != eest) {
      c.status = LRNDE_DT_NAN;
    } else {
      const PiStep ps = pi_step(pi, g.exact_pow, eest, pi_pow(g.exact_pow, c.qold, pi.beta2), c.q11);
      c.q11 = ps.q11;
      if (eest <= 1.0f) {
        c.naccept++;
        c.qold = pi_qold(eest);
        t = snap_magnitude(c.t, c.dt, c.tstop);
        c.dtpropose = pi_propose(c.dt, ps.q, dtmax, dt_floor(t, dtmin));
        c.cur ^= 1;  // z <- z_new, K1 <- K7 (FSAL)
        cc.k1slot = (cc.k1slot + 6) & 7; cc.k1t = c.st[5].t;
        dt = c.dtpropose;
        // a cotangent impulse at the saved time just reached (vec_tsit5_solve: lambda += du, K1 re-evaluated, nf += 1)
        while (cc.iimp < a.nimp && a.imp[cc.iimp].s < t) ++cc.iimp;
        cc.imp0 = cc.iimp;
        while (cc.iimp < a.nimp && a.imp[cc.iimp].s == t && t < g.s1) ++cc.iimp;
        cc.imp1 = cc.iimp;
        if (cc.imp1 > cc.imp0) { cc.hit = 1; c.nf += 1; cc.st_hit = adj_lookup_lanes(g, rec, -t); cc.k1t = cc.st_hit.t; }
      } else {
        c.nreject++;
        dt = pi_reject_dt(pi, c.dt, c.q11);
      }
    }
  }
  adj_header(g, c, rec, stop_l, t, dt);
  if (c.status == ST_DONE) cc.hit = 0;
  if (pub) chadj_report(a, cc, j);
  return cc;
}

// ode_determine_initdt's evaluation point (one wave; every lane returns it): the start for CHADJ_INIT_A; for CHADJ_INIT_B
// s0 + dt0 with dt0 from the partials of d0 and d1.  st_hit is its dense-record position.
__device__ __forceinline__ ChAdjCtrl chadj_init_ctrl(const ChAdjArgs& a, int mode) {
  const AdjArgs& g = a.g;
  const AdjRecLanes rec = adj_rec_load(g);
  ChAdjCtrl cc = a.cc[0];
  float ts = g.s0;
  if (mode == CHADJ_INIT_B) {
    const double ntot = (double)g.n_lam + (double)g.P;
    const float d0 = (float)sqrt(chadj_sum(chadj_set(a, 0), a.np) / ntot);
    const float d1 = (float)sqrt(chadj_sum(chadj_set(a, 1), a.np) / ntot);
    cc.c.dt0 = initdt_dt0(d0, d1, g.dtmax);
    ts = g.s0 + cc.c.dt0;
  }
  cc.st_hit = adj_lookup_lanes(g, rec, -ts);
  return cc;
}

struct ChAdjSmem { float* w; const float* wg; float* v; double* red; ChAdjCtrl* bc; };
// dynamic LDS: chain_lds_bytes (lrnde_adj_route.hpp) with this tail behind the images and the record
constexpr size_t CHADJ_LDS_TAIL = NW * 3 * sizeof(double) + sizeof(ChAdjCtrl) + 32;

// One element of the tile enters the VJP once its y is known: a_0 = act0(y), act0'(y) and the cotangent lam of f at its LDS
// slot (the element's thread; a barrier follows in chadj_eval_tail)
__device__ __forceinline__ void chadj_put(const ChainDev& cd, const ChAdjSmem& s, int lidx, float y, float lam) {
  float* lds = s.v;
  const float h = act_apply(cd.in_act, y);
  (lds + cd.meta[CM_AOFF])[lidx] = h;
  (lds + cd.uoff)[lidx] = act_deriv_c(cd.in_act, y, h);
  (lds + cd.gboff)[lidx] = lam;
}

// The part after "y is known" (every in-tile element went through chadj_put): forward through the L layers at time t
// keeping every layer's input and act', backward, and the tile's parameter cotangent: gp[q] = the tile's sum (ACC false,
// the continuous loop) or gp[q] + the tile's sum (ACC true, the discrete sweep: element q always has the same thread)
template <bool ACC>
__device__ __forceinline__ void chadj_eval_tail(const ChainDev& cd, const ChAdjSmem& s, const ChainSlots& sl, float t, float* kout, float* gp) {
  float* lds = s.v;
  float* du = lds + cd.uoff;
  float* ga = lds + cd.gboff;
  float* gb = ga + CMAXW * CNB;
  __syncthreads();
  for (int l = 0; l < cd.L; ++l) {
    const int* mt = cd.meta + l * CMETA;
    float* xout = (l + 1 < cd.L) ? lds + mt[CMETA + CM_AOFF] : gb;
    chain_layer(s.w + mt[CM_WOFF], mt[CM_IN], mt[CM_OUT], mt[CM_OUTP], cd.td, mt[CM_ACT], lds + mt[CM_AOFF], xout, lds + mt[CM_ZOFF], t);
    __syncthreads();
  }
  float* gc = ga;
  float* gn = gb;
  for (int l = cd.L - 1; l >= 0; --l) {
    const int* mt = cd.meta + l * CMETA;
    const int in = mt[CM_IN], out = mt[CM_OUT];
    const float* al = lds + mt[CM_AOFF];
    const float* zl = lds + mt[CM_ZOFF];
    for (int e = threadIdx.x; e < out * CNB; e += NT) gc[e] = gc[e] * zl[e];  // delta = g .* act'(z)
    __syncthreads();
    {  // this layer's block of the flat Lux vector: vec(W) (out x (in+td)), then b
      const int nw = out * (in + cd.td);
      float* gpl = gp + mt[CM_POFF];
      for (int q = threadIdx.x; q < nw + out; q += NT) {
        float acc = 0.f;
        if (q < nw) {
          const int o = q % out, k = q / out;
          if (k < in) {
#pragma unroll
            for (int n = 0; n < CNB; ++n) acc = fma_(gc[o * CNB + n], al[k * CNB + n], acc);
          } else {
#pragma unroll
            for (int n = 0; n < CNB; ++n) acc = fma_(gc[o * CNB + n], t, acc);
          }
        } else {
          const int o = q - nw;
#pragma unroll
          for (int n = 0; n < CNB; ++n) acc = acc + gc[o * CNB + n];
        }
        gpl[q] = ACC ? gpl[q] + acc : acc;
      }
    }
    // g_prev[k][n] = sum_o W[o][k] delta[o][n]  (o ascending)
    const float* wg = s.wg + mt[CM_GOFF];
    for (int e = threadIdx.x; e < in * CNB; e += NT) {
      const int k = e >> 3, n = e & (CNB - 1);
      float acc = 0.f;
#pragma unroll 4
      for (int o = 0; o < out; ++o) acc = fma_(wg[(size_t)o * in + k], gc[o * CNB + n], acc);
      gn[e] = acc;
    }
    __syncthreads();
    float* tmp = gc; gc = gn; gn = tmp;
  }
#pragma unroll
  for (int i = 0; i < CEPT; ++i) kout[i] = sl.in[i] ? gc[sl.lidx[i]] * du[sl.lidx[i]] : 0.f;
  __syncthreads();
}

// K = [J^T lam; the tile's (df/dp)^T lam] at (y(t) of the dense record, t): k_vjp_chain's arithmetic with lam and the
// result in the registers of the element's thread and the weights in LDS
__device__ __forceinline__ void chadj_eval(const ChainDev& cd, const ChAdjSmem& s, const ChainSlots& sl, const ChAdjArgs& a,
                                           const AdjStage& st, const float* lam, float* kout, float* gp) {
  const size_t nst = a.g.n_lam;
  const float* dense = a.g.dense + (size_t)st.lo * REC_ARRAYS * nst;
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    if (!sl.in[i]) continue;
    float y = 0.f;
    if (sl.valid[i]) {
      const size_t g = sl.g[i];
      y = tsit5_rec_eval(dense[g], dense[nst + g], dense[2 * nst + g], dense[3 * nst + g], dense[4 * nst + g], st.theta, st.ddt);
    }
    chadj_put(cd, s, sl.lidx[i], y, lam[i]);
  }
  chadj_eval_tail<false>(cd, s, sl, st.t, kout, gp);
}

// mode CHADJ_STEP: attempt j.  CHADJ_INIT_A: K1 = rhs(z, s0) and the lambda partials of d0, d1.  CHADJ_INIT_B: initdt's
// second evaluation at z + dt0*K1 and the lambda partials of d2.
__global__ __launch_bounds__(NT) void k_chadj_step(ChAdjArgs a, ChainDev cd, int j, int mode) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  ChAdjSmem s;
  s.w = reinterpret_cast<float*>(smem);
  float* wgl = s.w + cd.wfloats;
  s.v = wgl + (a.wg_lds ? ((a.gfloats + 3) & ~3) : 0);
  s.red = reinterpret_cast<double*>(s.v + cd.gboff + 2 * CMAXW * CNB);
  s.bc = reinterpret_cast<ChAdjCtrl*>(s.red + NW * 3);
  s.wg = a.wg_lds ? wgl : cd.wg;
  chain_load_weights(cd, s.w);
  if (a.wg_lds)
    for (int i = threadIdx.x; i < a.gfloats; i += NT) wgl[i] = cd.wg[i];
  const AdjArgs& g = a.g;
  const int b0 = blockIdx.x * CNB, nvalid = min(CNB, a.B - b0);
  const ChainSlots sl = chain_slots(cd.D, b0, nvalid);
  const size_t P = g.P;
  float* gp0 = a.gpart + (size_t)blockIdx.x * P;
  const size_t gstride = (size_t)a.nwg * P;

  if (mode != CHADJ_STEP) {
    // ---- ode_determine_initdt's evaluations (vec_tsit5_solve's first block) ----
    if (threadIdx.x < 64) {
      const ChAdjCtrl cc = chadj_init_ctrl(a, mode);
      if ((threadIdx.x & 63) == 0) *s.bc = cc;
    }
    __syncthreads();
    const float dt0 = s.bc->c.dt0;
    const AdjStage st = s.bc->st_hit;
    const float* z = adj_zb(g, 0);
    float* K1 = adj_K(g, 0, 0);
    float lam[CEPT], x[CEPT], k1[CEPT], kk[CEPT];
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      lam[i] = sl.valid[i] ? z[sl.g[i]] : 0.f;
      k1[i] = (mode == CHADJ_INIT_B && sl.valid[i]) ? K1[sl.g[i]] : 0.f;
      x[i] = (mode == CHADJ_INIT_B) ? lam[i] + (dt0 * 1.0f) * k1[i] : lam[i];
    }
    chadj_eval(cd, s, sl, a, st, x, kk, gp0);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int i = 0; i < CEPT; ++i) {
      if (!sl.valid[i]) continue;
      const float sa = __builtin_fabsf(lam[i]);
      const float sc = g.abstol + fmaxf_(sa, sa) * g.reltol;
      if (mode == CHADJ_INIT_A) {
        K1[sl.g[i]] = kk[i];
        const float r0 = lam[i] / sc, r1 = kk[i] / sc;
        a0 += (double)(r0 * r0); a1 += (double)(r1 * r1);
      } else {
        const float r2 = (kk[i] - k1[i]) / sc;
        a2 += (double)(r2 * r2);
      }
    }
    block_sum3(s.red, a0, a1, a2);
    if (threadIdx.x == 0) {
      if (mode == CHADJ_INIT_A) { chadj_set(a, 0)[blockIdx.x] = a0; chadj_set(a, 1)[blockIdx.x] = a1; }
      else chadj_set(a, 2)[blockIdx.x] = a2;
    }
    return;
  }

  if (threadIdx.x < 64) {
    const ChAdjCtrl cc = chadj_prologue(a, j);
    if ((threadIdx.x & 63) == 0) *s.bc = cc;
  }
  __syncthreads();
  if (!s.bc->c.do_step) return;
  const int cur = s.bc->c.cur;
  const float dt = s.bc->c.dt;
  float* z = adj_zb(g, cur);
  float* zn = adj_zb(g, cur ^ 1);
  float* K1 = adj_K(g, 0, cur);
  float* K7 = adj_K(g, 6, cur);
  float lam[CEPT], lamn[CEPT], x[CEPT], kr[7][CEPT];
#pragma unroll
  for (int i = 0; i < CEPT; ++i) { lam[i] = sl.valid[i] ? z[sl.g[i]] : 0.f; lamn[i] = 0.f; }
  if (s.bc->hit) {
    // lambda += du (k_axpy's one-term form with dt = c = 1), K1 re-evaluated at the modified state
    for (int q = s.bc->imp0; q < s.bc->imp1; ++q) {
      const float* du = a.imp[q].du;
#pragma unroll
      for (int i = 0; i < CEPT; ++i)
        if (sl.valid[i]) lam[i] = lam[i] + (1.0f * 1.0f) * du[sl.g[i]];
    }
    const AdjStage sh = s.bc->st_hit;
    chadj_eval(cd, s, sl, a, sh, lam, kr[0], gp0);
#pragma unroll
    for (int i = 0; i < CEPT; ++i)
      if (sl.valid[i]) { z[sl.g[i]] = lam[i]; K1[sl.g[i]] = kr[0][i]; }
  } else {
#pragma unroll
    for (int i = 0; i < CEPT; ++i) kr[0][i] = sl.valid[i] ? K1[sl.g[i]] : 0.f;
  }
  // stage S: lambda_S = lambda + dt * sum_j a_Sj K_j (k_axpy: left to right; ONE term: lambda + (dt*a21)*K1), K_S = rhs
#define LRNDE_CHADJ_STAGE(S)                                                                   \
  do {                                                                                         \
    constexpr int off_ = (S - 2) * (S - 1) / 2;                                                \
    _Pragma("unroll") for (int i = 0; i < CEPT; ++i) {                                         \
      if (S == 2) {                                                                            \
        const float c_ = dt * (float)Tsit5::A[0];                                              \
        x[i] = lam[i] + c_ * kr[0][i];                                                         \
      } else {                                                                                 \
        float sm_ = (float)Tsit5::A[off_] * kr[0][i];                                          \
        _Pragma("unroll") for (int q = 1; q < S - 1; ++q) sm_ = sm_ + (float)Tsit5::A[off_ + q] * kr[q][i]; \
        x[i] = lam[i] + dt * sm_;                                                              \
      }                                                                                        \
      if (S == 7) { lamn[i] = x[i]; if (sl.valid[i]) zn[sl.g[i]] = x[i]; }                     \
    }                                                                                          \
    const AdjStage st_ = s.bc->c.st[S - 2];                                                    \
    chadj_eval(cd, s, sl, a, st_, x, kr[S - 1], gp0 + (size_t)(S - 1) * gstride);              \
  } while (0)
  LRNDE_CHADJ_STAGE(2);
  LRNDE_CHADJ_STAGE(3);
  LRNDE_CHADJ_STAGE(4);
  LRNDE_CHADJ_STAGE(5);
  LRNDE_CHADJ_STAGE(6);
  LRNDE_CHADJ_STAGE(7);
#undef LRNDE_CHADJ_STAGE
  // K7 (the next attempt's K1 if this one is accepted) and the lambda part of the error norm (k_adj_err's expressions)
  double aerr = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll
  for (int i = 0; i < CEPT; ++i) {
    if (!sl.valid[i]) continue;
    K7[sl.g[i]] = kr[6][i];
    float sm = (float)Tsit5::BT[0] * kr[0][i];
#pragma unroll
    for (int q = 1; q < 7; ++q) sm = sm + (float)Tsit5::BT[q] * kr[q][i];
    const float ut = 0.f + dt * sm;
    const float sc = g.abstol + fmaxf_(__builtin_fabsf(lam[i]), __builtin_fabsf(lamn[i])) * g.reltol;
    const float r = ut / sc;
    aerr += (double)(r * r);
  }
  block_sum3(s.red, aerr, u1, u2);
  if (threadIdx.x == 0) chadj_set(a, 3 + (j & 1))[blockIdx.x] = aerr;
}

// sum over the workgroups of slot `slot`, element i, in workgroup order from 0 (k_chain_pgsum's order)
__device__ __forceinline__ float chadj_slot_sum(const ChAdjArgs& a, int slot, size_t i) {
  const size_t P = a.g.P;
  const float* p = a.gpart + (size_t)slot * a.nwg * P + i;
  float acc = 0.f;
  int w = 0;
  for (; w + 8 <= a.nwg; w += 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = p[(size_t)(w + q) * P];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc = acc + v[q];
  }
  for (; w < a.nwg; ++w) acc = acc + p[(size_t)w * P];
  return acc;
}

// the mu part of an attempt (or of an init phase): wave w of a block sums slot w for the block's 64 parameters, wave 0
// then combines them.  Blocks take chunks of 64 parameters round robin; each writes one fp64 partial of the norm.
__global__ __launch_bounds__(CHADJ_MU_NT) void k_chadj_mu(ChAdjArgs a, int j, int mode) {
  __shared__ float ks[7][64];
  const AdjArgs& g = a.g;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t n = g.n_lam, P = g.P;
  if (mode != CHADJ_STEP) {
    // init A: K1_mu = sum of slot 0, partials of d0 and d1; init B: K_mu of the second evaluation, partial of d2
    if (wave != 0) return;
    const float* z = adj_zb(g, 0) + n;
    float* K1 = adj_K(g, 0, 0) + n;
    double a0 = 0.0, a1 = 0.0;
    for (size_t ch = blockIdx.x; ch * 64 < P; ch += gridDim.x) {
      const size_t i = ch * 64 + lane;
      if (i >= P) continue;
      const float kv = chadj_slot_sum(a, 0, i);
      const float zv = z[i];
      const float sa = __builtin_fabsf(zv);
      const float sc = g.abstol + fmaxf_(sa, sa) * g.reltol;
      if (mode == CHADJ_INIT_A) {
        K1[i] = kv;
        const float r0 = zv / sc, r1 = kv / sc;
        a0 += (double)(r0 * r0); a1 += (double)(r1 * r1);
      } else {
        const float r2 = (kv - K1[i]) / sc;
        a0 += (double)(r2 * r2);
      }
    }
    a0 = wave_sum_dpp(a0); a1 = wave_sum_dpp(a1);
    if (lane == 0) {
      if (mode == CHADJ_INIT_A) { chadj_set(a, 0)[a.nwg + blockIdx.x] = a0; chadj_set(a, 1)[a.nwg + blockIdx.x] = a1; }
      else chadj_set(a, 2)[a.nwg + blockIdx.x] = a0;
    }
    return;
  }
  const ChAdjCtrl cc = a.cc[(j + 1) & 1];   // published by block 0 of this attempt's k_chadj_step
  if (!cc.c.do_step) return;
  const int cur = cc.c.cur;
  const float dt = cc.c.dt;
  const float* z = adj_zb(g, cur) + n;
  float* zn = adj_zb(g, cur ^ 1) + n;
  float* K1 = adj_K(g, 0, cur) + n;
  float* K7 = adj_K(g, 6, cur) + n;
  double acc = 0.0;
  for (size_t ch = blockIdx.x; ch * 64 < P; ch += gridDim.x) {
    const size_t i = ch * 64 + lane;
    const bool in = i < P;
    if (in && (wave > 0 || cc.hit)) ks[wave][lane] = chadj_slot_sum(a, wave, i);
    __syncthreads();
    if (wave == 0 && in) {
      float kv[7];
      if (cc.hit) { kv[0] = ks[0][lane]; K1[i] = kv[0]; }
      else kv[0] = K1[i];
#pragma unroll
      for (int q = 1; q < 7; ++q) kv[q] = ks[q][lane];
      const float zv = z[i];
      float sm = (float)Tsit5::A[15] * kv[0];
#pragma unroll
      for (int q = 1; q < 6; ++q) sm = sm + (float)Tsit5::A[15 + q] * kv[q];
      const float znv = zv + dt * sm;
      zn[i] = znv;
      K7[i] = kv[6];
      float se = (float)Tsit5::BT[0] * kv[0];
#pragma unroll
      for (int q = 1; q < 7; ++q) se = se + (float)Tsit5::BT[q] * kv[q];
      const float ut = 0.f + dt * se;
      const float sc = g.abstol + fmaxf_(__builtin_fabsf(zv), __builtin_fabsf(znv)) * g.reltol;
      const float r = ut / sc;
      acc += (double)(r * r);
    }
    __syncthreads();
  }
  if (wave == 0) {
    acc = wave_sum_dpp(acc);
    if (lane == 0) chadj_set(a, 3 + (j & 1))[a.nwg + blockIdx.x] = acc;
  }
}

// The start of a chain handle's reversed solve: the control blocks and (up to 64 per launch, by value) the tstops and
// the impulse table, so that no copy from pageable host memory sits in front of the solve
struct ChAdjBegin {
  ChAdjCtrl* cc; float s0; int init;
  float* stops; int nstops, soff;
  ChAdjImp* imp; int nimp, ioff;
  float sv[64]; ChAdjImp iv[64];
};
__global__ __launch_bounds__(64) void k_chadj_begin(ChAdjBegin b) {
  const int lane = threadIdx.x;
  if (lane < b.nstops) b.stops[b.soff + lane] = b.sv[lane];
  if (lane < b.nimp) b.imp[b.ioff + lane] = b.iv[lane];
  if (lane != 0 || !b.init) return;
  ChAdjCtrl c;
  memset(&c, 0, sizeof(c));
  c.c.status = ST_RUNNING; c.c.first = 1; c.c.t = b.s0; c.c.qold = QOLDINIT; c.c.q11 = 1.0f;
  c.k1t = -b.s0;
  b.cc[0] = c; b.cc[1] = c;
}
