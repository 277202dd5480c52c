// lrnde_wide_adjoint.hpp — the continuous adjoint of a wide Dense-chain handle with the controller on the device
// (DESIGN.md 4.12.1).  Included by lrnde_kernels.hip inside its anonymous namespace, behind lrnde_wide_chain.hpp (tile,
// wide_gemm, wide_feval, the VJP record's layout) and lrnde_chain_adjoint.hpp (ChAdjCtrl, chadj_prologue, the norm
// partial sets, k_chadj_begin: the controller, its protocol and its begin launch are the small chain's, shared).
//
// The reversed-time Tsit5 solve on z = [lambda (B*D); mu (P)] that vec_tsit5_solve + adj_rhs run with six k_vjp_wide +
// k_chain_pgsum pairs and a norm read-back per attempted step, in TWO launches per attempted step and no host wait:
//
//   k_wadj_step  one workgroup of NT threads per tile of NB = 16 batch columns (k_vjp_wide's column -> workgroup map).
//                Wave 0 runs chadj_prologue; block 0 publishes it.  Then six stages, each k_vjp_wide's arithmetic: the
//                stage lambda from z and the earlier K's (k_axpy's expression), y(t) from the dense record, wide_feval
//                keeping every layer's input and act', delta = g .* act', g <- W^T delta (wide_gemm on the transposed
//                image), the lambda part of K_s.  z, z_new and K1..K7 stay in global memory (L2); the element map of
//                every pass over them is wide_stage's, so a thread re-reads only what it wrote itself.  Instead of a
//                parameter cotangent the kernel leaves a_l and delta_l of every layer in a stage record.
//   k_wadj_mu    mu never feeds the right-hand side.  One launch per attempt forms every stage's (df/dp)^T lambda over
//                the whole batch from the stage records, then the mu part of z_new, of K7 and of utilde and the mu
//                partials of the error norm.
//
// Stage record: [8 slots][nwg tiles][recfloats] floats, one tile's part in k_vjp_wide's record layout ([row][16]; the
// act' rows of a layer hold delta once the backward pass has been over them).  Stage S = 2..7 of an attempt goes to slot
// (k1slot + S - 1) & 7; an accepted step's K7 slot becomes the next attempt's k1slot (FSAL, no copy), a rejected step
// keeps it, an impulse re-evaluates K1 into it.  ChAdjCtrl carries k1slot and the forward time K1 was evaluated at.
//
// Summation order (fixed; no float atomics): K_s^mu[o][k] = 0 + p_0 + p_1 + ... over the tiles in order (k_chain_pgsum's
// chain), p_w = k_vjp_wide's four MFMAs from a zero accumulator over the tile's columns (an fma chain in column order);
// the time column fma(delta, t_s, acc) over the columns, the bias a plain sum.  The stages enter mu_new and utilde in
// k_axpy's order s = 1..7.  Norm partials: one fp64 per workgroup of each launch, sets 3 + (j & 1) (chadj_set).

struct WAdjArgs {
  ChAdjArgs a;     // (a.gpart, a.wg_lds, a.gfloats are not used here)
  float* rec;      // [8][nwg][recfloats]
};

constexpr int WADJ_SLOTS = 8;
constexpr int WADJ_MU_NT = 7 * 64;        // k_wadj_mu: wave s forms stage s + 1
// (its grid is at most CHADJ_MAX_MU_BLOCKS workgroups, one norm partial each, as k_chadj_mu's; more work items than that
//  take further trips)
static_assert(sizeof(ChAdjCtrl) == 53 * 4, "wide_device_gate counts two control blocks; tests/wide_chain_adjoint_cases.py restates it with this size");
constexpr int WADJ_MB = 2;                // output blocks per side of a work item: 2 x 2 blocks of 16 x 16 share their operands

constexpr size_t WADJ_LDS_TAIL = WIDE_LDS_TAIL + sizeof(ChAdjCtrl);   // the control block sits behind the forward carve's tail (wadj_ctrl)
__device__ __forceinline__ ChAdjCtrl* wadj_ctrl(const WideSmem& s) { return reinterpret_cast<ChAdjCtrl*>(s.bc + 1); }
__device__ __forceinline__ float* wadj_rec(const WAdjArgs& w, const WideDev& wd, int slot, int tile) {
  return w.rec + ((size_t)slot * w.a.nwg + tile) * wd.recfloats;
}

// every real element of the tile in wide_stage's element map (the one map of all passes over z and the K's)
template <class F> __device__ __forceinline__ void wadj_each(int D, int b0, int nvalid, F&& fn) {
  const int Dp = (D + 15) & ~15;
  for (int idx = threadIdx.x; idx < Dp * NB; idx += NT) {
    const int n = idx / Dp, row = idx - n * Dp;
    if (n < nvalid && row < D) fn((size_t)(b0 + n) * D + row, row, n);
  }
}

// K = J^T lam at (y(t) of the dense record, t), k_vjp_wide's arithmetic; lamv(g) is the stage lambda of element g.
// a_l and delta_l of every layer stay in rec.  kout: the lambda part of K.
template <class Lam>
__device__ __forceinline__ void wadj_eval(const WideDev& wd, const WideSmem& s, const AdjArgs& g, const AdjStage& st, int b0,
                                          int nvalid, float* rec, Lam&& lamv, float* kout) {
  const int D = wd.D;
  float* src = s.xa;
  float* dst = s.xb;
  {
    float* ra0 = rec + wd.meta[WM_RAOFF];
    float* rdu = rec + wd.rduoff;
    const size_t nst = g.n_lam;
    const float* dense = g.dense + (size_t)st.lo * REC_ARRAYS * nst;
    const int Dp = (D + 15) & ~15;
    for (int idx = threadIdx.x; idx < Dp * NB; idx += NT) {
      const int n = idx / Dp, row = idx - n * Dp;
      float y = 0.f;
      if (n < nvalid && row < D) {
        const size_t e = (size_t)(b0 + n) * D + row;
        y = tsit5_rec_eval(dense[e], dense[nst + e], dense[2 * nst + e], dense[3 * nst + e], dense[4 * nst + e], st.theta, st.ddt);
      }
      const float h = act_apply(wd.in_act, y);
      src[lds_index(row, n)] = h;
      ra0[row * NB + n] = h;
      rdu[row * NB + n] = act_deriv_c(wd.in_act, y, h);
    }
  }
  __syncthreads();
  wide_feval(wd, s, src, dst, st.t, rec, [&](int, int, const f32x4&) {});
  __syncthreads();
  float* gc = src;
  float* gn = dst;
  wide_stage(D, b0, nvalid, gc, [&](size_t e, int, int) { return lamv(e); });
  __syncthreads();
  for (int l = wd.L - 1; l >= 0; --l) {
    const int* mt_ = wd.meta + l * WMETA;
    const int MT = mt_[WM_MT], KG = mt_[WM_KG];
    float* rz = rec + mt_[WM_RZOFF];
    for (int idx = threadIdx.x; idx < MT * 16 * NB; idx += NT) {  // delta = g .* act'(z), kept for k_wadj_mu
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
  wadj_each(D, b0, nvalid, [&](size_t e, int row, int n) { kout[e] = gc[lds_index(row, n)] * rdu[row * NB + n]; });
  __syncthreads();
}

// mode CHADJ_STEP: attempt j.  CHADJ_INIT_A: K1 = rhs(z, s0) into slot 0 and the lambda partials of d0, d1.
// CHADJ_INIT_B: initdt's second evaluation at z + dt0*K1 into slot 1 (lambda part: K2's buffer) and the partials of d2.
__global__ __launch_bounds__(NT) void k_wadj_step(WAdjArgs w, WideDev wd, int j, int mode) {
  const WideSmem s = wide_carve(wd);
  ChAdjCtrl* bc = wadj_ctrl(s);
  const ChAdjArgs& a = w.a;
  const AdjArgs& g = a.g;
  const int D = wd.D;
  const int b0 = blockIdx.x * NB, nvalid = min(NB, a.B - b0);

  if (mode != CHADJ_STEP) {
    if (threadIdx.x < 64) {
      const ChAdjCtrl cc = chadj_init_ctrl(a, mode);
      if (threadIdx.x == 0) *bc = cc;
    }
    __syncthreads();
    const float dt0 = bc->c.dt0;
    const AdjStage st = bc->st_hit;
    const float* z = adj_zb(g, 0);
    float* K1 = adj_K(g, 0, 0);
    float* K2 = adj_K(g, 1, 0);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (mode == CHADJ_INIT_A) {
      wadj_eval(wd, s, g, st, b0, nvalid, wadj_rec(w, wd, 0, blockIdx.x), [&](size_t e) { return z[e]; }, K1);
      wadj_each(D, b0, nvalid, [&](size_t e, int, int) {
        const float lam = z[e], sa = __builtin_fabsf(lam);
        const float sc = g.abstol + fmaxf_(sa, sa) * g.reltol;
        const float r0 = lam / sc, r1 = K1[e] / sc;
        a0 += (double)(r0 * r0); a1 += (double)(r1 * r1);
      });
    } else {
      wadj_eval(wd, s, g, st, b0, nvalid, wadj_rec(w, wd, 1, blockIdx.x), [&](size_t e) { return z[e] + (dt0 * 1.0f) * K1[e]; }, K2);
      wadj_each(D, b0, nvalid, [&](size_t e, int, int) {
        const float sa = __builtin_fabsf(z[e]);
        const float sc = g.abstol + fmaxf_(sa, sa) * g.reltol;
        const float r2 = (K2[e] - K1[e]) / sc;
        a2 += (double)(r2 * r2);
      });
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
    if (threadIdx.x == 0) *bc = cc;
  }
  __syncthreads();
  if (!bc->c.do_step) return;
  const int cur = bc->c.cur, k1slot = bc->k1slot;
  const float dt = bc->c.dt;
  float* z = adj_zb(g, cur);
  float* zn = adj_zb(g, cur ^ 1);
  float* const K1 = adj_K(g, 0, cur);
  float* const K7 = adj_K(g, 6, cur);
  auto Kq = [&](int q) -> float* { return q == 0 ? K1 : (q == 6 ? K7 : g.base + (size_t)(4 + q) * g.N); };   // adj_K(g, q, cur)
  if (bc->hit) {
    // lambda += du (k_axpy's one-term form with dt = c = 1), K1 re-evaluated at the modified state into its slot
    const int imp0 = bc->imp0, imp1 = bc->imp1;
    const AdjStage sh = bc->st_hit;
    wadj_eval(wd, s, g, sh, b0, nvalid, wadj_rec(w, wd, k1slot, blockIdx.x), [&](size_t e) {
      float lam = z[e];
      for (int q = imp0; q < imp1; ++q) lam = lam + (1.0f * 1.0f) * a.imp[q].du[e];
      z[e] = lam;
      return lam;
    }, K1);
  }
  // stage S: lambda_S = lambda + dt * sum_j a_Sj K_j (k_axpy: left to right; ONE term: lambda + (dt*a21)*K1), K_S = rhs
#pragma unroll 1
  for (int S = 2; S <= 7; ++S) {
    const int off = (S - 2) * (S - 1) / 2;
    const AdjStage st = bc->c.st[S - 2];
    wadj_eval(wd, s, g, st, b0, nvalid, wadj_rec(w, wd, (k1slot + S - 1) & 7, blockIdx.x), [&](size_t e) {
      float x;
      if (S == 2) {
        const float c_ = dt * (float)Tsit5::A[0];
        x = z[e] + c_ * K1[e];
      } else {
        float sm = (float)Tsit5::A[off] * K1[e];
        for (int q = 1; q < S - 1; ++q) sm = sm + (float)Tsit5::A[off + q] * Kq(q)[e];
        x = z[e] + dt * sm;
      }
      if (S == 7) zn[e] = x;
      return x;
    }, Kq(S - 1));
  }
  // the lambda part of the error norm (k_adj_err's expressions)
  double aerr = 0.0, u1 = 0.0, u2 = 0.0;
  wadj_each(D, b0, nvalid, [&](size_t e, int, int) {
    float sm = (float)Tsit5::BT[0] * K1[e];
#pragma unroll
    for (int q = 1; q < 7; ++q) sm = sm + (float)Tsit5::BT[q] * Kq(q)[e];
    const float ut = 0.f + dt * sm;
    const float sc = g.abstol + fmaxf_(__builtin_fabsf(z[e]), __builtin_fabsf(zn[e])) * g.reltol;
    const float r = ut / sc;
    aerr += (double)(r * r);
  });
  block_sum3(s.red, aerr, u1, u2);
  if (threadIdx.x == 0) chadj_set(a, 3 + (j & 1))[blockIdx.x] = aerr;
}

// ---- the mu launch ----
// Work items, layer by layer: first the groups of WADJ_MB x WADJ_MB output blocks of vec(W) (ceil(MT/2) * ceil(KG/2) per
// layer), then chunks of 64 outputs of the time column and the bias (ceil(out/64) per layer).
struct WAdjItem { int l, vec, i; };   // layer; 0: block group i, 1: vector chunk i
__device__ __forceinline__ int wadj_layer_groups(const int* mt_) { return ((mt_[WM_MT] + WADJ_MB - 1) / WADJ_MB) * ((mt_[WM_KG] + WADJ_MB - 1) / WADJ_MB); }
__device__ __forceinline__ int wadj_layer_chunks(const int* mt_) { return (mt_[WM_OUT] + 63) / 64; }
__device__ __forceinline__ WAdjItem wadj_item(const WideDev& wd, int it) {
  for (int l = 0; l < wd.L; ++l) {
    const int* mt_ = wd.meta + l * WMETA;
    const int ng = wadj_layer_groups(mt_), nc = wadj_layer_chunks(mt_);
    if (it < ng) return WAdjItem{l, 0, it};
    it -= ng;
    if (it < nc) return WAdjItem{l, 1, it};
    it -= nc;
  }
  return WAdjItem{-1, 0, 0};
}

// One parameter's end of an attempt from its seven K_s (chadj's k_chadj_mu expressions): z_new, K7 and the squared
// scaled utilde
__device__ __forceinline__ double wadj_mu_finish(const AdjArgs& g, const float (&kv)[7], float dt, float zv, float* zn, float* K7) {
  float sm = (float)Tsit5::A[15] * kv[0];
#pragma unroll
  for (int q = 1; q < 6; ++q) sm = sm + (float)Tsit5::A[15 + q] * kv[q];
  const float znv = zv + dt * sm;
  *zn = znv;
  *K7 = kv[6];
  float se = (float)Tsit5::BT[0] * kv[0];
#pragma unroll
  for (int q = 1; q < 7; ++q) se = se + (float)Tsit5::BT[q] * kv[q];
  const float ut = 0.f + dt * se;
  const float sc = g.abstol + fmaxf_(__builtin_fabsf(zv), __builtin_fabsf(znv)) * g.reltol;
  const float r = ut / sc;
  return (double)(r * r);
}

// One work item of the parameter cotangent over the whole batch (the block engine k_wadj_mu and k_wdisc_mu share): wave s
// (active: it has a stage) forms K_s of the item from the stage record whose tile 0 starts at slot0 (tiles recfloats apart)
// into ks[s], with its stage's forward time ts; then finish(i, e) is called by one thread for every real parameter i of
// the item, e its place in ks[.].  All WADJ_MU_NT threads of the workgroup call it; the caller synchronises before the next.
template <class Fin>
__device__ __forceinline__ void wadj_mu_item(const WideDev& wd, const float* slot0, int nwg, bool active, int wave, int lane, float ts,
                                             int it, float (*ks)[WADJ_MB * WADJ_MB * 256], Fin&& finish) {
  constexpr int MB = WADJ_MB, NBLK = MB * MB;
  const int lr = lane & 15, lq = lane >> 4;
  const WAdjItem wi = wadj_item(wd, it);
  const int* mt_ = wd.meta + wi.l * WMETA;
  const int in = mt_[WM_IN], out = mt_[WM_OUT], MT = mt_[WM_MT], KG = mt_[WM_KG];
  const size_t pl = (size_t)mt_[WM_POFF];
  if (!wi.vec) {
    const int ngo = (MT + MB - 1) / MB;
    const int ot0 = (wi.i % ngo) * MB, kt0 = (wi.i / ngo) * MB;
    if (active) {
      // K_s[o][k] of the MB x MB blocks: per tile the four MFMAs from zero (columns as their K dimension), then one add
      const float* base = slot0;
      int aoff[MB], doff[MB];
#pragma unroll
      for (int u = 0; u < MB; ++u) {   // (a block past the layer's edge repeats the last one; it is not stored)
        aoff[u] = mt_[WM_RAOFF] + (min(kt0 + u, KG - 1) * 16 + lr) * NB + lq;
        doff[u] = mt_[WM_RZOFF] + (min(ot0 + u, MT - 1) * 16 + lr) * NB + lq;
      }
      f32x4 sum[NBLK];
#pragma unroll
      for (int b = 0; b < NBLK; ++b) sum[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int t = 0; t < nwg; ++t) {
        const float* r = base + (size_t)t * wd.recfloats;
        float av[MB][4], dv[MB][4];
#pragma unroll
        for (int u = 0; u < MB; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q) { av[u][q] = r[aoff[u] + 4 * q]; dv[u][q] = r[doff[u] + 4 * q]; }
#pragma unroll
        for (int uo = 0; uo < MB; ++uo)
#pragma unroll
          for (int uk = 0; uk < MB; ++uk) {
            f32x4 p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) p = __builtin_amdgcn_mfma_f32_16x16x4f32(av[uk][q], dv[uo][q], p, 0, 0, 0);
            f32x4& sm = sum[uo * MB + uk];
            sm.x = sm.x + p.x; sm.y = sm.y + p.y; sm.z = sm.z + p.z; sm.w = sm.w + p.w;
          }
      }
#pragma unroll
      for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) ks[wave][((b * 4 + r) * 4 + lq) * 16 + lr] = sum[b][r];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NBLK * 256; e += WADJ_MU_NT) {
      const int b = e >> 8, r = (e >> 6) & 3, q = (e >> 4) & 3, x = e & 15;
      const int o = (ot0 + b / MB) * 16 + x, k = (kt0 + b % MB) * 16 + q * 4 + r;
      if (o < out && k < in) finish(pl + (size_t)out * k + o, e);
    }
  } else {
    // the t column (k = in) and the bias (k = in + td) of outputs wi.i*64 ..: lane = output, wave = stage
    const int o = wi.i * 64 + lane;
    if (active && o < out) {
      const float* base = slot0 + mt_[WM_RZOFF] + o * NB;
      float st_ = 0.f, sb_ = 0.f;
      for (int t = 0; t < nwg; ++t) {
        const f32x4* d4 = reinterpret_cast<const f32x4*>(base + (size_t)t * wd.recfloats);
        float dl[NB];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const f32x4 v = d4[q]; dl[4 * q] = v.x; dl[4 * q + 1] = v.y; dl[4 * q + 2] = v.z; dl[4 * q + 3] = v.w; }
        float pt = 0.f, pb = 0.f;
#pragma unroll
        for (int c = 0; c < NB; ++c) { pt = fma_(dl[c], ts, pt); pb = pb + dl[c]; }
        st_ = st_ + pt; sb_ = sb_ + pb;
      }
      ks[wave][lane] = st_; ks[wave][64 + lane] = sb_;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 128; e += WADJ_MU_NT) {
      const int which = e >> 6, oo = wi.i * 64 + (e & 63);
      if (oo < out && (which == 1 || wd.td)) finish(pl + (size_t)out * (in + (which ? wd.td : 0)) + oo, e);
    }
  }
}

__global__ __launch_bounds__(WADJ_MU_NT) void k_wadj_mu(WAdjArgs w, WideDev wd, int nitems, int j, int mode) {
  constexpr int MB = WADJ_MB, NBLK = MB * MB;
  __shared__ float ks[7][NBLK * 256];
  __shared__ double red[7 * 3];
  const ChAdjArgs& a = w.a;
  const AdjArgs& g = a.g;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t n = g.n_lam;
  // which evaluations this launch sums: stage slots and their forward times (wave s: its own)
  int nstage, slot;
  float ts;
  int cur = 0;
  float dt = 0.f;
  if (mode == CHADJ_STEP) {
    const ChAdjCtrl* cc = a.cc + ((j + 1) & 1);   // published by block 0 of this attempt's k_wadj_step
    if (!cc->c.do_step) return;
    cur = cc->c.cur; dt = cc->c.dt;
    nstage = 7;
    slot = (cc->k1slot + wave) & 7;
    ts = wave == 0 ? cc->k1t : cc->c.st[wave - 1].t;
  } else {
    const ChAdjCtrl ci = chadj_init_ctrl(a, mode);
    nstage = 1;
    slot = mode == CHADJ_INIT_A ? 0 : 1;
    ts = ci.st_hit.t;
  }
  const bool active = wave < nstage;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  const float* z = adj_zb(g, cur) + n;
  float* zn = adj_zb(g, cur ^ 1) + n;
  float* K1 = adj_K(g, 0, cur) + n;
  float* K7 = adj_K(g, 6, cur) + n;
  // one parameter of the item: its K's are ks[0..nstage)[e]
  auto finish = [&](size_t i, int e) {
    if (mode == CHADJ_STEP) {
      float kv[7];
#pragma unroll
      for (int q = 0; q < 7; ++q) kv[q] = ks[q][e];
      acc0 += wadj_mu_finish(g, kv, dt, z[i], zn + i, K7 + i);
      return;
    }
    const float kv = ks[0][e];
    const float zv = z[i];
    const float sa = __builtin_fabsf(zv);
    const float sc = g.abstol + fmaxf_(sa, sa) * g.reltol;
    if (mode == CHADJ_INIT_A) {
      K1[i] = kv;
      const float r0 = zv / sc, r1 = kv / sc;
      acc0 += (double)(r0 * r0); acc1 += (double)(r1 * r1);
    } else {
      const float r2 = (kv - K1[i]) / sc;
      acc2 += (double)(r2 * r2);
    }
  };
#pragma unroll 1
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    wadj_mu_item(wd, wadj_rec(w, wd, slot, 0), a.nwg, active, wave, lane, ts, it, ks, finish);
    __syncthreads();
  }
  // one fp64 partial (three in init A / B's sets) per workgroup: the waves' sums in wave order
  acc0 = wave_sum_dpp(acc0); acc1 = wave_sum_dpp(acc1); acc2 = wave_sum_dpp(acc2);
  if (lane == 0) { red[wave * 3] = acc0; red[wave * 3 + 1] = acc1; red[wave * 3 + 2] = acc2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < 7; ++q) { s0 += red[q * 3]; s1 += red[q * 3 + 1]; s2 += red[q * 3 + 2]; }
    const int slotp = a.nwg + blockIdx.x;
    if (mode == CHADJ_STEP) chadj_set(a, 3 + (j & 1))[slotp] = s0;
    else if (mode == CHADJ_INIT_A) { chadj_set(a, 0)[slotp] = s0; chadj_set(a, 1)[slotp] = s1; }
    else chadj_set(a, 2)[slotp] = s2;
  }
}
