// lrnde_sde_model.hpp — the MNIST-SDE model around the NeuralDSDE layer (experiments/src/construct.jl:202-210):
//   Chain(flatten, downsample = Dense(Din => D), neural_dsde, sol_to_arr, classifier = Dense(D => K)),
//   loss = logitcrossentropy(y_pred, y) + w_reg * reg_val (construct.jl:18-31).
// The downsample layer forward and backward as fp32 MFMA kernels, the classifier head of lrnde_cls_fused.hpp on the SDE
// handle, and the model's recorded forward / pullback as wrappers of lrnde_sde_node_forward_record_alg /
// lrnde_sde_node_backward_recorded.  Included by lrnde_kernels.hip after the classifier head.
//
// Parameters of the downsample layer: the flat Lux block [vec(W) (D x Din, column-major: W[o][k] at o + D*k); b (D)].
//
// Summation order (what the bits of a result depend on):
//   forward  u0[b][o]: the k range is cut into DSM_NW = 8 segments of seg = 4 * ceil(ceil(Din / 4) / 8) consecutive k
//            (a function of Din alone); inside a segment the products are accumulated four k at a time, ascending, by
//            v_mfma_f32_16x16x4_f32; the eight segment sums are added in segment order ((s0 + s1) + ... + s7), the bias
//            last.  Nothing depends on B, on the sample's place in its 16-sample tile or on the workgroup.
//   backward dW[o][k], db[o]: the batch is cut into groups of four consecutive samples; wave w of the workgroup owns the
//            groups g = w, w + 8, w + 16, ... and accumulates them ascending (one MFMA per group), the eight wave sums
//            are added in wave order ((p0 + p1) + ... + p7).  db is the column k = Din of the same GEMM against ones.
//            A round of the eight waves covers DSM_BR = 32 samples.  No atomics.

namespace {

constexpr int DSM_NW = 8;               // waves per workgroup: K segments (forward), interleaved batch groups (backward)
constexpr int DSM_NT = 64 * DSM_NW;
constexpr int DSM_MS = 16;              // samples per forward workgroup: one MFMA tile
constexpr int DSM_KC = 64;              // k values a wave stages per trip
constexpr int DSM_LS = DSM_KC + 4;      // LDS row stride: 16-byte aligned rows, the 16 x 4 operand read hits 64 banks
constexpr int DSM_OG = 64;              // outputs per workgroup: four MFMA tiles
constexpr int DSM_BR = 4 * DSM_NW;      // samples per round of the backward's waves

__host__ __device__ inline int dsm_seg(int Din) { return 4 * ((((Din + 3) / 4) + DSM_NW - 1) / DSM_NW); }

// u0 = x W^T + b.  grid (ceil(B / 16), ceil(D / 64)); x is staged through LDS, each wave its own segment (VEC: 16-byte loads,
// Din a multiple of 4 and x 16-byte aligned), W is read from memory (L2: every workgroup reads the same block).
// NT: MFMA tiles of outputs the workgroup holds (compile time: no branch between the unrolled loads).
template <bool VEC, int NT>
__global__ __launch_bounds__(DSM_NT) void k_dsm_fwd(const float* __restrict__ x, const float* __restrict__ pd, float* __restrict__ u0,
                                                    int B, int Din, int D) {
  __shared__ __attribute__((aligned(16))) float sm[DSM_NW * DSM_MS * DSM_LS];   // the staged x; afterwards the waves' partial tiles
  static_assert(DSM_NW * DSM_MS * DSM_LS >= DSM_NW * 4 * 256, "the partial tiles alias the staging buffer");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int b0 = blockIdx.x * DSM_MS, ob = blockIdx.y * DSM_OG;
  const int seg = dsm_seg(Din);
  const int kbeg = w * seg, kend = kbeg + seg < Din ? kbeg + seg : Din;
  float* xs = sm + w * (DSM_MS * DSM_LS);
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < seg; c0 += DSM_KC) {
    const int kb = kbeg + c0;
    if (VEC) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int idx = lane + 64 * r, row = idx >> 4, c4 = 4 * (idx & 15), b = b0 + row, k = kb + c4;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (b < B && k < kend) v = *reinterpret_cast<const f32x4*>(x + (size_t)b * Din + k);
        *reinterpret_cast<f32x4*>(xs + row * DSM_LS + c4) = v;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int idx = lane + 64 * r, row = idx >> 6, col = idx & 63, b = b0 + row, k = kb + col;
        xs[row * DSM_LS + col] = (b < B && k < kend) ? x[(size_t)b * Din + k] : 0.f;
      }
    }
    __syncthreads();
    if (kb < kend) {   // (wave-uniform; the loads are unconditional at a clamped index so that they all go out together)
#pragma unroll
      for (int g = 0; g < DSM_KC / 4; ++g) {
        const int k = kb + 4 * g + lk;
        const float a = xs[li * DSM_LS + 4 * g + lk];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int o = ob + 16 * n + li;
          const bool ok = k < kend && o < D;
          const float wl = pd[ok ? (size_t)D * k + o : (size_t)0];
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok ? wl : 0.f, acc[n], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // the waves' tiles [w][n][sample][output], then the segment sums in segment order and the bias
#pragma unroll
  for (int n = 0; n < NT; ++n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) sm[((w * 4 + n) * 16 + (lk * 4 + r)) * 16 + li] = acc[n][r];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < DSM_MS * DSM_OG; e += DSM_NT) {
    const int i = e >> 6, oo = e & 63, n = oo >> 4, j = oo & 15, b = b0 + i, o = ob + oo;
    if (b < B && o < D) {
      float s = sm[(n * 16 + i) * 16 + j];
#pragma unroll
      for (int ww = 1; ww < DSM_NW; ++ww) s = s + sm[((ww * 4 + n) * 16 + i) * 16 + j];
      u0[(size_t)b * D + o] = s + pd[(size_t)D * Din + o];
    }
  }
}

// dpd = [du0^T x, du0^T 1].  grid (ceil((Din + 1) / 16), ceil(D / 64)): a workgroup owns 16 columns k (k = Din: the bias) and
// up to 64 rows o; the batch is the MFMA reduction dimension.
template <int NT>
__global__ __launch_bounds__(DSM_NT) void k_dsm_bwd(const float* __restrict__ x, const float* __restrict__ du0, float* __restrict__ dpd,
                                                    int B, int Din, int D) {
  __shared__ float red[DSM_NW * 4 * 256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int k0 = blockIdx.x * 16, ob = blockIdx.y * DSM_OG;
  const int k = k0 + li, ng = (B + 3) / 4;
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  // four of the wave's groups per trip, their loads issued together (unconditional, at a clamped index), then their MFMAs in
  // ascending group order; a group past the batch contributes zeros
  for (int g0 = w; g0 < ng; g0 += 4 * DSM_NW) {
    float xv[4], dv[4][NT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = 4 * (g0 + u * DSM_NW) + lk;
      const bool xok = b < B && k < Din;
      const float xl = x[xok ? (size_t)b * Din + k : (size_t)0];
      xv[u] = xok ? xl : ((b < B && k == Din) ? 1.0f : 0.f);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int o = ob + 16 * n + li;
        const bool dok = b < B && o < D;
        const float dl = du0[dok ? (size_t)b * D + o : (size_t)0];
        dv[u][n] = dok ? dl : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[u][n], xv[u], acc[n], 0, 0, 0);
  }
#pragma unroll
  for (int n = 0; n < NT; ++n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[((w * 4 + n) * 16 + (lk * 4 + r)) * 16 + li] = acc[n][r];   // [w][n][row o][column k]
  }
  __syncthreads();
  for (int e = threadIdx.x; e < DSM_OG * 16; e += DSM_NT) {
    const int oo = e & 63, j = e >> 6, n = oo >> 4, i = oo & 15, o = ob + oo, kk = k0 + j;
    if (o < D && kk <= Din) {
      float s = red[(n * 16 + i) * 16 + j];
#pragma unroll
      for (int ww = 1; ww < DSM_NW; ++ww) s = s + red[((ww * 4 + n) * 16 + i) * 16 + j];
      dpd[(size_t)D * kk + o] = s;
    }
  }
}

// dx = du0 W (only when the caller asks: x is data in the experiment).  One thread per element, o ascending.
__global__ void k_dsm_dx(const float* du0, const float* pd, float* dx, int B, int Din, int D) {
  const size_t n = (size_t)B * Din;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / Din, k = i % Din;
    float s = 0.f;
    for (int o = 0; o < D; ++o) s = fma_(du0[b * D + o], pd[(size_t)D * k + o], s);
    dx[i] = s;
  }
}

int dsm_check(lrnde_sde* s, int32_t B, int32_t Din) {
  lrnde_ctx* c = s->drift;
  if (c->hung) return fail(c, LRNDE_HIP_ERROR, "the handle's queue stopped making progress in an earlier call: destroy the handle");
  if (B < 1 || Din < 1) return fail(c, LRNDE_BADARG, "batch and input size must be positive (got B = %d, Din = %d)", B, Din);
  if ((size_t)B * (size_t)(Din > c->desc.state_dim ? Din : c->desc.state_dim) > ((size_t)1 << 40) || (B + DSM_MS - 1) / DSM_MS > 0x7fffffff / 2)
    return fail(c, LRNDE_BADARG, "batch too large");
  HIPCHK(c, hipSetDevice(c->device));
  return LRNDE_OK;
}
// enqueued on the handle's stream, no synchronisation
int dsm_forward_enqueue(lrnde_sde* s, const float* x, int32_t B, int32_t Din, const float* pd, float* u0) {
  lrnde_ctx* c = s->drift;
  const int D = c->desc.state_dim;
  // D <= 64: one workgroup row with ceil(D / 16) tiles; beyond: rows of four tiles (columns past D are masked)
  const int nt = D <= DSM_OG ? (D + 15) / 16 : 4;
  const dim3 grid((B + DSM_MS - 1) / DSM_MS, (D + DSM_OG - 1) / DSM_OG);
  const bool vec = Din % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#define DSM_FWD(V, N) hipLaunchKernelGGL((k_dsm_fwd<V, N>), grid, dim3(DSM_NT), 0, c->stream, x, pd, u0, B, Din, D)
  if (vec) { if (nt == 1) DSM_FWD(true, 1); else if (nt == 2) DSM_FWD(true, 2); else if (nt == 3) DSM_FWD(true, 3); else DSM_FWD(true, 4); }
  else { if (nt == 1) DSM_FWD(false, 1); else if (nt == 2) DSM_FWD(false, 2); else if (nt == 3) DSM_FWD(false, 3); else DSM_FWD(false, 4); }
#undef DSM_FWD
  HIPCHK(c, hipGetLastError());
  return LRNDE_OK;
}
int dsm_backward_enqueue(lrnde_sde* s, const float* x, int32_t B, int32_t Din, const float* pd, const float* du0, float* dpd, float* dx) {
  lrnde_ctx* c = s->drift;
  const int D = c->desc.state_dim;
  const int nt = D <= DSM_OG ? (D + 15) / 16 : 4;
  const dim3 grid((Din + 1 + 15) / 16, (D + DSM_OG - 1) / DSM_OG);
#define DSM_BWD(N) hipLaunchKernelGGL((k_dsm_bwd<N>), grid, dim3(DSM_NT), 0, c->stream, x, du0, dpd, B, Din, D)
  if (nt == 1) DSM_BWD(1); else if (nt == 2) DSM_BWD(2); else if (nt == 3) DSM_BWD(3); else DSM_BWD(4);
#undef DSM_BWD
  if (dx) hipLaunchKernelGGL(k_dsm_dx, dim3(sde_nb((size_t)B * Din)), dim3(256), 0, c->stream, du0, pd, dx, B, Din, D);
  HIPCHK(c, hipGetLastError());
  return LRNDE_OK;
}

}  // namespace

extern "C" {

int lrnde_sde_dense_forward(lrnde_sde* s, const float* x, int32_t B, int32_t Din, const float* pd, float* u0) {
  if (!s) return LRNDE_BADARG;
  if (!x || !pd || !u0) return fail(s->drift, LRNDE_BADARG, "null pointer");
  int rc = dsm_check(s, B, Din);
  if (rc) return rc;
  if ((rc = dsm_forward_enqueue(s, x, B, Din, pd, u0))) return rc;
  HIPCHK(s->drift, hipStreamSynchronize(s->drift->stream));
  return LRNDE_OK;
}

int lrnde_sde_dense_backward(lrnde_sde* s, const float* x, int32_t B, int32_t Din, const float* pd, const float* du0, float* dpd, float* dx) {
  if (!s) return LRNDE_BADARG;
  if (!x || !pd || !du0 || !dpd) return fail(s->drift, LRNDE_BADARG, "null pointer");
  int rc = dsm_check(s, B, Din);
  if (rc) return rc;
  if ((rc = dsm_backward_enqueue(s, x, B, Din, pd, du0, dpd, dx))) return rc;
  HIPCHK(s->drift, hipStreamSynchronize(s->drift->stream));
  return LRNDE_OK;
}

// the head of lrnde_classifier_ce on the SDE handle's state size, stream and workspace: same kernels, same arithmetic
int lrnde_sde_classifier_ce(lrnde_sde* s, const float* u, int32_t B, const float* pc, int32_t K, const int32_t* labels, float* loss_host,
                            float* logits, float* du, float* dpc) {
  if (!s) return LRNDE_BADARG;
  return lrnde_classifier_ce(s->drift, u, B, pc, K, labels, loss_host, logits, du, dpc);
}

int lrnde_sde_model_forward_record_ce(lrnde_sde* s, const float* x, int32_t Din, const float* pd, const float* W, int32_t nfine, int32_t B,
                                      float t0, float t2, const lrnde_sde_adapt_opts* o, int32_t mode, float t1_or_rand,
                                      const float* z_local, int32_t save_start, const float* saveat_host, int32_t nsave, float* u_series,
                                      float* t_series_host, int32_t cap_series, int32_t* nseries_host, float* reg_val_host,
                                      int32_t* nfe_drift_host, int32_t* nfe_diffusion_host, lrnde_stats* st, float* t1_used_host,
                                      int32_t which, const lrnde_sri_tableau* tab, const float* Z, const float* z2_local, const float* pc,
                                      int32_t K, const int32_t* labels, float* loss_host, float* logits, float* dpc) {
  if (!s) return LRNDE_BADARG;
  lrnde_ctx* c = s->drift;
  s->mdl_gen = 0;
  if (!x || !pd || !pc || !labels || !loss_host) return fail(c, LRNDE_BADARG, "null pointer");
  if (K < 1 || K > 16) return fail(c, LRNDE_BADARG, "bad argument (1 <= K <= 16)");
  int rc = dsm_check(s, B, Din);
  if (rc) return rc;
  const size_t n = (size_t)B * c->desc.state_dim;
  HIPCHK(c, s->mdl_u0.grow(n));
  // the downsample goes into the queue ahead of the layer's launches; the head behind them, from the layer's hook, ahead of
  // the layer's closing synchronisation — which then delivers the loss
  if ((rc = dsm_forward_enqueue(s, x, B, Din, pd, s->mdl_u0))) return rc;
  int nser = 0;
  s->fwd_hook = [&](const float* u_end, int ns) -> int {
    nser = ns;
    HIPCHK(c, s->mdl_duser.grow((size_t)ns * n));   // the series cotangent: zero but for the head's du on sol.u[end]
    if (ns > 1) HIPCHK(c, hipMemsetAsync(s->mdl_duser, 0, sizeof(float) * (size_t)(ns - 1) * n, c->stream));
    return cls_enqueue(c, u_end, B, pc, K, labels, logits, s->mdl_duser + (size_t)(ns - 1) * n, dpc);
  };
  rc = lrnde_sde_node_forward_record_alg(s, s->mdl_u0, W, nfine, B, t0, t2, o, mode, t1_or_rand, z_local, save_start, saveat_host, nsave,
                                         u_series, t_series_host, cap_series, nseries_host, reg_val_host, nfe_drift_host,
                                         nfe_diffusion_host, st, t1_used_host, which, tab, Z, z2_local);
  s->fwd_hook = nullptr;
  if (rc) return rc;
  if ((rc = cls_finish(c, B, K, loss_host))) return rc;
  s->mdl_x = x; s->mdl_pd = pd; s->mdl_Din = Din; s->mdl_B = B; s->mdl_nser = nser;
  s->mdl_gen = sde_node_generation(s);
  return LRNDE_OK;
}

int lrnde_sde_model_backward_recorded(lrnde_sde* s, int32_t B, float w_reg, float* dpd, float* dp_drift, float* dp_diff, float* dx) {
  if (!s) return LRNDE_BADARG;
  lrnde_ctx* c = s->drift;
  if (!dpd || !dp_drift || !dp_diff) return fail(c, LRNDE_BADARG, "null pointer");
  if (B < 1) return fail(c, LRNDE_BADARG, "batch must be positive (got %d)", B);
  // the layer's record must still be the one this model forward made: a later forward on the handle replaced it
  if (!s->mdl_gen || s->mdl_gen != sde_node_generation(s) || s->mdl_B != B)
    return fail(c, LRNDE_BADARG, "no usable record (call lrnde_sde_model_forward_record_ce first; a later forward replaces it)");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)B * c->desc.state_dim;
  HIPCHK(c, s->mdl_dxn.grow(n));
  s->defer_wait = true;   // (the one-launch sweep leaves its closing wait to this call's)
  int rc = lrnde_sde_node_backward_recorded(s, B, s->mdl_duser, s->mdl_nser, w_reg, s->mdl_dxn, dp_drift, dp_diff);
  s->defer_wait = false;
  if (rc) return rc;
  if ((rc = dsm_backward_enqueue(s, s->mdl_x, B, s->mdl_Din, s->mdl_pd, s->mdl_dxn, dpd, dx))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return LRNDE_OK;
}

}  // extern "C"
