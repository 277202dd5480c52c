// lrnde_latent.hpp — the layers around the Dense-chain field in the PhysioNet Latent ODE
// (experiments/src/construct.jl:230-252): Recurrence(LatentGRUCell) (src/layers/latent_ode.jl:1-48), rec_to_gen,
// ReparameterizeLayer (src/layers/common.jl:47-77), gen_to_data and the loss (construct.jl:36-76,
// experiments/src/utils.jl:94-101).  Included by lrnde_kernels.hip at file scope; it needs lrnde.h, lrnde_hooks.h,
// lrnde_math.hpp and lrnde_buf.hpp only.
//
// Sizes: I = in_dims, F = 2I + 1 rows of x_t, H = hidden_dims, L = latent_dims, N = node_dims.
//
// Tile: LNB = 8 batch columns per workgroup of LNT = 512 threads; thread (j = tid >> 3, n = tid & 7) works on column n.
// Columns are independent: nothing depends on B or on which workgroup holds a column.  Activations live in LDS as
// [row][LNB].
//
// Canonical accumulation order (the same in every kernel here and in tests/latent_host.cpp):
//   first layers of update_gate / reset_gate / new_state, input vcat(y_mean, y_std, x_t) resp. vcat(y_mean.*r, y_std.*r, x_t):
//     z[o] = (fma chain from 0 over the x_t rows f = 0..F-1 (W[o][2L+f] * x_t[f]), continued over the carry rows
//             k = 0..2L-1 (W[o][k] * carry[k])) + b[o];
//   every other Dense (the gates' second layers, rec_to_gen, gen_to_data):
//     z[o] = (fma chain from 0 over k = 0..in-1 of W[o][k] * in[k]) + b[o];
//   activations tanhf_c / sigmoid_c (lrnde_math.hpp); y_mean .* r is one multiplication;
//   new_y = (1 - u) * s + u * y as written: a subtraction, two multiplications, an addition (no fma);
//   mask_t = (x_t[I] + x_t[I+1] + ... + x_t[2I], added in row order from 0) > 0; where it is false the carry is copied;
//   z0 = mu + expf_c(logvar * 0.5f) * eps: a multiplication, then an addition.
// The x_t part of a first layer comes first so that it could leave the serial loop without changing a bit; this
// kernel does not hoist it (the x_t projections of all steps do not fit LDS next to the weights).
//
// latent_ode.jl:37 builds new_y_mean from new_state_STD, so rows 0..L-1 of new_state's second layer never reach an
// output.  The parameters keep their place in the flat vector; the kernels do not evaluate those rows and their
// cotangent is written as exact zeros.
//
// Forward (k_lat_fwd): ONE launch; the weight image of the three gates (first layers [u1 | r1 | n1] side by side,
// rows = x_t rows, carry rows, bias; second layers [u2 | r2]; new_state's std rows) is copied to LDS once and stays
// (109 KB at 37/40/50: one workgroup per CU); the T steps run inside the launch; a step at which no column of the
// tile is observed is skipped (the carry passes through).  The tail applies rec_to_gen and the reparameterisation
// (weights read from global memory once).  The kernel RECORDS what the backward needs, per step and tile:
// the step's input carry (2L), the three hidden layers (3H), u, r, s (3L); and for the tail y, g1, exp(logvar/2), eps.
//
// Backward (k_lat_bwd): ONE launch walks the steps in reverse from the record.  Parameter cotangent: every image
// element belongs to one thread, which continues ONE fma chain per element: over the steps in reverse, within a step over
// the tile's columns in column order; the workgroup's partial vector is summed over the workgroups in workgroup order
// and scattered to the flat Lux order by k_lat_pgsum (the k_chain_pgsum protocol).  No atomics.
//
// Decode + loss (k_lat_dec, k_lat_dec_sum): one workgroup per column: gen_to_data on every saved state, the log
// likelihood, the KL term and every cotangent; gen_to_data's parameter cotangent is a per-column partial (over the
// saved times in time order) summed over the columns in column order, the loss a sum over the columns in column order.

namespace {

constexpr int LNB = 8;
constexpr int LNT = 512;
constexpr int LNJ = LNT / LNB;   // 64 rows of threads
constexpr int LAT_MAX_T = 4096;  // steps whose mask flags fit the LDS table

struct LatGeom {
  int I, F, H, L, N;
  int OPA, OPB, OPD, OPE, OPG;      // floats per image row (outputs rounded up to even)
  int offB, offD, ldsw, offE, offG, wimg;   // image offsets (floats); [0, ldsw) lives in LDS
  int Kin;                           // 2L + F
  int SZg, SZn, off_rg, P;           // flat sizes of a gate / new_state, offset of rec_to_gen, encoder parameters
  int RW, TW;                        // rows of a step record / of the tail record
};

inline int lat_even(int v) { return v + (v & 1); }

inline LatGeom lat_geom(const lrnde_latent_desc& d) {
  LatGeom g{};
  g.I = d.in_dims; g.F = 2 * d.in_dims + 1; g.H = d.hidden_dims; g.L = d.latent_dims; g.N = d.node_dims;
  g.Kin = 2 * g.L + g.F;
  g.OPA = lat_even(3 * g.H); g.OPB = lat_even(2 * g.L); g.OPD = lat_even(g.L); g.OPE = lat_even(g.L); g.OPG = lat_even(2 * g.N);
  g.offB = (g.F + 2 * g.L + 1) * g.OPA;
  g.offD = g.offB + (g.H + 1) * g.OPB;
  g.ldsw = (g.offD + (g.H + 1) * g.OPD + 3) / 4 * 4;
  g.offE = g.ldsw;
  g.offG = g.offE + (2 * g.L + 1) * g.OPE;
  g.wimg = (g.offG + (g.L + 1) * g.OPG + 3) / 4 * 4;
  g.SZg = g.H * g.Kin + g.H + g.L * g.H + g.L;
  g.SZn = g.H * g.Kin + g.H + 2 * g.L * g.H + 2 * g.L;
  g.off_rg = 2 * g.SZg + g.SZn;
  g.P = g.off_rg + g.L * 2 * g.L + g.L + 2 * g.N * g.L + 2 * g.N;
  g.RW = 5 * g.L + 3 * g.H;
  g.TW = 3 * g.L + 2 * g.N;
  return g;
}

// flat Lux index of image element e (-1: padding)
__host__ __device__ inline int lat_src(const LatGeom& g, int e) {
  const int H = g.H, L = g.L, F = g.F;
  if (e < g.offB) {
    const int row = e / g.OPA, o = e % g.OPA;
    if (o >= 3 * H) return -1;
    const int gate = o / H, oo = o % H;
    const int base = gate < 2 ? gate * g.SZg : 2 * g.SZg;
    if (row < F) return base + oo + (2 * L + row) * H;
    if (row < F + 2 * L) return base + oo + (row - F) * H;
    return base + H * g.Kin + oo;
  }
  if (e < g.offD) {
    const int q = e - g.offB, row = q / g.OPB, o = q % g.OPB;
    if (o >= 2 * L) return -1;
    const int base = (o / L) * g.SZg + H * g.Kin + H, l = o % L;
    return row < H ? base + l + row * L : base + L * H + l;
  }
  if (e < g.ldsw) {
    const int q = e - g.offD, row = q / g.OPD, o = q % g.OPD;
    if (o >= L || row > H) return -1;
    const int base = 2 * g.SZg + H * g.Kin + H;
    return row < H ? base + (L + o) + row * 2 * L : base + 2 * L * H + L + o;
  }
  if (e < g.offG) {
    const int q = e - g.offE, row = q / g.OPE, o = q % g.OPE;
    if (o >= L) return -1;
    return row < 2 * L ? g.off_rg + o + row * L : g.off_rg + 2 * L * L + o;
  }
  {
    const int q = e - g.offG, row = q / g.OPG, o = q % g.OPG;
    if (o >= 2 * g.N || row > L) return -1;
    const int base = g.off_rg + 2 * L * L + L;
    return row < L ? base + o + row * 2 * g.N : base + 2 * g.N * L + o;
  }
}

__global__ void k_lat_pack(LatGeom g, const float* p, float* img) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < g.wimg; e += gridDim.x * blockDim.x) {
    const int s = lat_src(g, e);
    img[e] = s >= 0 ? p[s] : 0.f;
  }
}

// dp[flat] = sum over the workgroups in workgroup order; the dead rows of new_state's second layer get exact zeros
__global__ void k_lat_pgsum(LatGeom g, const float* part, int nwg, float* dp) {
  const int ndead = g.L * g.H + g.L;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < g.wimg + ndead; e += gridDim.x * blockDim.x) {
    if (e >= g.wimg) {   // latent_ode.jl:37: new_state_mean is never used
      const int q = e - g.wimg, base = 2 * g.SZg + g.H * g.Kin + g.H;
      if (q < g.L * g.H) dp[base + (q % g.L) + (q / g.L) * 2 * g.L] = 0.f;
      else dp[base + 2 * g.L * g.H + (q - g.L * g.H)] = 0.f;
      continue;
    }
    const int s = lat_src(g, e);
    if (s < 0) continue;
    float acc = 0.f;
    for (int w = 0; w < nwg; ++w) acc = acc + part[(size_t)w * g.wimg + e];
    dp[s] = acc;
  }
}

struct LatSmem {
  float *w, *xs, *yb, *h1, *ug, *rg, *sg, *c, *o2;    // forward and backward
  float *dY, *dYn, *dz1, *dz2, *dzs, *dc;             // backward only
  unsigned char* m8;
};
__host__ __device__ inline size_t lat_act_floats(const LatGeom& g, bool bwd) {
  size_t n = (size_t)g.F * LNB + 2 * g.L * LNB + (size_t)g.OPA * LNB + 3 * (size_t)g.L * LNB + 2 * g.L * LNB + 2 * g.N * LNB;
  if (bwd) n += 2 * (size_t)(2 * g.L * LNB) + (size_t)g.OPA * LNB + 2 * g.L * LNB + g.L * LNB + 2 * g.L * LNB;
  return n;
}
inline size_t lat_smem_bytes(const LatGeom& g, bool bwd, int T) {
  return ((size_t)g.ldsw + lat_act_floats(g, bwd)) * sizeof(float) + (size_t)(T + 1) * LNB + 16;
}
__device__ __forceinline__ LatSmem lat_carve(const LatGeom& g, bool bwd) {
  extern __shared__ __attribute__((aligned(16))) char lat_smem[];
  LatSmem s;
  float* p = reinterpret_cast<float*>(lat_smem);
  s.w = p; p += g.ldsw;
  s.xs = p; p += g.F * LNB;
  s.yb = p; p += 2 * g.L * LNB;
  s.h1 = p; p += g.OPA * LNB;
  s.ug = p; p += g.L * LNB;
  s.rg = p; p += g.L * LNB;
  s.sg = p; p += g.L * LNB;
  s.c = p; p += 2 * g.L * LNB;
  s.o2 = p; p += 2 * g.N * LNB;
  s.dY = s.dYn = s.dz1 = s.dz2 = s.dzs = s.dc = nullptr;
  if (bwd) {
    s.dY = p; p += 2 * g.L * LNB;
    s.dYn = p; p += 2 * g.L * LNB;
    s.dz1 = p; p += g.OPA * LNB;
    s.dz2 = p; p += 2 * g.L * LNB;
    s.dzs = p; p += g.L * LNB;
    s.dc = p; p += 2 * g.L * LNB;
  }
  s.m8 = reinterpret_cast<unsigned char*>(p);
  return s;
}

__device__ __forceinline__ void lat_load_weights(const LatGeom& g, const float* img, float* w) {
  const float4* src = reinterpret_cast<const float4*>(img);
  float4* dst = reinterpret_cast<float4*>(w);
  for (int i = threadIdx.x; i < g.ldsw / 4; i += LNT) dst[i] = src[i];
}

// mask flags of every step of the tile: m8[t * LNB + n] = (sum of rows I..2I of x_t, in row order) > 0
__device__ __forceinline__ void lat_mask_table(const LatGeom& g, const float* x, int b0, int nvalid, int T, unsigned char* m8) {
  for (int e = threadIdx.x; e < T * LNB; e += LNT) {
    const int t = e / LNB, n = e % LNB;
    float s = 0.f;
    if (n < nvalid) {
      const float* xp = x + ((size_t)(b0 + n) * T + t) * g.F;
      for (int f = g.F / 2; f < g.F; ++f) s = s + xp[f];
    }
    m8[e] = s > 0.f ? 1 : 0;
  }
}
__device__ __forceinline__ bool lat_any(const unsigned char* m8, int t) {
  bool a = false;
#pragma unroll
  for (int n = 0; n < LNB; ++n) a = a || m8[t * LNB + n];
  return a;
}
__device__ __forceinline__ void lat_load_x(const LatGeom& g, const float* x, int b0, int nvalid, int T, int t, float* xs) {
  for (int e = threadIdx.x; e < g.F * LNB; e += LNT) {
    const int n = e / g.F, f = e % g.F;
    xs[f * LNB + n] = n < nvalid ? x[((size_t)(b0 + n) * T + t) * g.F + f] : 0.f;
  }
}

struct LatFwdArgs {
  const float* x; const float* eps; const float* img;
  int B, T, training;
  float *y, *mu, *lv, *z0;
  float *rec, *trec;
};

__global__ __launch_bounds__(LNT) void k_lat_fwd(LatGeom g, LatFwdArgs a) {
  using lrnde::fma_;
  const LatSmem s = lat_carve(g, false);
  const int tid = threadIdx.x, n = tid & (LNB - 1), j = tid >> 3;
  const int b0 = blockIdx.x * LNB, nvalid = min(LNB, a.B - b0);
  const int H = g.H, L = g.L, F = g.F, N = g.N, T = a.T;
  lat_load_weights(g, a.img, s.w);
  lat_mask_table(g, a.x, b0, nvalid, T, s.m8);
  for (int e = tid; e < 2 * L * LNB; e += LNT) s.yb[e] = e < L * LNB ? 0.f : 1.f;   // latent_ode.jl:20-21
  __syncthreads();
  const float* wA = s.w;
  const float* wB = s.w + g.offB;
  const float* wD = s.w + g.offD;
  const int o0 = 2 * j;
  float* rec_tile = a.rec + (size_t)blockIdx.x * T * g.RW * LNB;
  for (int t = 0; t < T; ++t) {
    if (!lat_any(s.m8, t)) continue;   // nobody in the tile is observed: every carry passes through (latent_ode.jl:40-43)
    float* rec = rec_tile + (size_t)t * g.RW * LNB;
    lat_load_x(g, a.x, b0, nvalid, T, t, s.xs);
    __syncthreads();
    // A: first layers [u1 | r1 | n1]: the x_t rows for all three, the carry rows for u1 and r1
    float a0 = 0.f, a1 = 0.f;
    if (o0 < 3 * H) {
      const float* wp = wA + o0;
      for (int k = 0; k < F; ++k) {
        const float xv = s.xs[k * LNB + n];
        const float2 w = *reinterpret_cast<const float2*>(wp + k * g.OPA);
        a0 = fma_(w.x, xv, a0);
        a1 = fma_(w.y, xv, a1);
      }
      if (o0 < 2 * H) {
        for (int k = 0; k < 2 * L; ++k) {
          const float yv = s.yb[k * LNB + n];
          const float2 w = *reinterpret_cast<const float2*>(wp + (F + k) * g.OPA);
          a0 = fma_(w.x, yv, a0);
          a1 = fma_(w.y, yv, a1);
        }
        const float2 b = *reinterpret_cast<const float2*>(wp + (F + 2 * L) * g.OPA);
        s.h1[o0 * LNB + n] = lrnde::tanhf_c(a0 + b.x);
        s.h1[(o0 + 1) * LNB + n] = lrnde::tanhf_c(a1 + b.y);   // (2H is even: the pair stays inside [u1 | r1])
      }
    }
    __syncthreads();
    // B: second layers [u2 | r2], sigmoid; the reset gate's rows also form y .* r
    for (int o = j; o < 2 * L; o += LNJ) {
      const float* src = s.h1 + (o < L ? 0 : H) * LNB;
      float acc = 0.f;
      for (int k = 0; k < H; ++k) acc = fma_(wB[k * g.OPB + o], src[k * LNB + n], acc);
      const float v = lrnde::sigmoid_c(acc + wB[H * g.OPB + o]);
      if (o < L) {
        s.ug[o * LNB + n] = v;
      } else {
        const int l = o - L;
        s.rg[l * LNB + n] = v;
        s.c[l * LNB + n] = s.yb[l * LNB + n] * v;
        s.c[(L + l) * LNB + n] = s.yb[(L + l) * LNB + n] * v;
      }
    }
    __syncthreads();
    // C: new_state's first layer continues its x_t chain over vcat(y_mean .* r, y_std .* r)
    if (o0 >= 2 * H && o0 < 3 * H) {
      const float* wp = wA + o0;
      for (int k = 0; k < 2 * L; ++k) {
        const float cv = s.c[k * LNB + n];
        const float2 w = *reinterpret_cast<const float2*>(wp + (F + k) * g.OPA);
        a0 = fma_(w.x, cv, a0);
        a1 = fma_(w.y, cv, a1);
      }
      const float2 b = *reinterpret_cast<const float2*>(wp + (F + 2 * L) * g.OPA);
      s.h1[o0 * LNB + n] = lrnde::tanhf_c(a0 + b.x);
      if (o0 + 1 < 3 * H) s.h1[(o0 + 1) * LNB + n] = lrnde::tanhf_c(a1 + b.y);
    }
    __syncthreads();
    // D: new_state's std rows, the convex combination and the mask; the step's record
    for (int e = tid; e < 3 * H * LNB; e += LNT) rec[2 * L * LNB + e] = s.h1[e];
    const bool m = s.m8[t * LNB + n] != 0;
    for (int l = j; l < L; l += LNJ) {
      float acc = 0.f;
      for (int k = 0; k < H; ++k) acc = fma_(wD[k * g.OPD + l], s.h1[(2 * H + k) * LNB + n], acc);
      const float sv = lrnde::tanhf_c(acc + wD[H * g.OPD + l]);
      const float u = s.ug[l * LNB + n], ym = s.yb[l * LNB + n], ys = s.yb[(L + l) * LNB + n];
      const float om = 1.0f - u;
      // latent_ode.jl:37-38: BOTH halves are built from new_state_std
      const float nm = om * sv + u * ym;
      const float ns = om * sv + u * ys;
      rec[l * LNB + n] = ym;
      rec[(L + l) * LNB + n] = ys;
      rec[(2 * L + 3 * H + l) * LNB + n] = u;
      rec[(3 * L + 3 * H + l) * LNB + n] = s.rg[l * LNB + n];
      rec[(4 * L + 3 * H + l) * LNB + n] = sv;
      s.yb[l * LNB + n] = m ? nm : ym;
      s.yb[(L + l) * LNB + n] = m ? ns : ys;
    }
    __syncthreads();
  }
  // ---- tail: y, rec_to_gen, reparameterisation ----
  float* trec = a.trec + (size_t)blockIdx.x * g.TW * LNB;
  for (int e = tid; e < 2 * L * LNB; e += LNT) {
    const int row = e / LNB, nn = e % LNB;
    trec[e] = s.yb[e];
    if (nn < nvalid && a.y) a.y[(size_t)(b0 + nn) * 2 * L + row] = s.yb[e];
  }
  const float* wE = a.img + g.offE;
  const float* wG = a.img + g.offG;
  for (int l = j; l < L; l += LNJ) {
    float acc = 0.f;
    for (int k = 0; k < 2 * L; ++k) acc = fma_(wE[k * g.OPE + l], s.yb[k * LNB + n], acc);
    const float v = lrnde::tanhf_c(acc + wE[2 * L * g.OPE + l]);
    s.c[l * LNB + n] = v;
    trec[(2 * L + l) * LNB + n] = v;
  }
  __syncthreads();
  for (int o = j; o < 2 * N; o += LNJ) {
    float acc = 0.f;
    for (int k = 0; k < L; ++k) acc = fma_(wG[k * g.OPG + o], s.c[k * LNB + n], acc);
    s.o2[o * LNB + n] = acc + wG[L * g.OPG + o];
  }
  __syncthreads();
  for (int i = j; i < N; i += LNJ) {
    const float mu = s.o2[i * LNB + n], lv = s.o2[(N + i) * LNB + n];
    float ev = 0.f, ep = 0.f, z = mu, lvo = mu;   // common.jl:73-77: the Val(false) branch returns mu three times
    if (a.training) {                             // common.jl:61-71
      ep = n < nvalid ? a.eps[(size_t)(b0 + n) * N + i] : 0.f;
      ev = lrnde::expf_c(lv * 0.5f);
      const float pe = ev * ep;
      z = mu + pe;
      lvo = lv;
    }
    trec[(3 * L + i) * LNB + n] = ev;
    trec[(3 * L + N + i) * LNB + n] = ep;
    if (n < nvalid) {
      const size_t gi = (size_t)(b0 + n) * N + i;
      if (a.mu) a.mu[gi] = mu;
      if (a.lv) a.lv[gi] = lvo;
      if (a.z0) a.z0[gi] = z;
    }
  }
}

struct LatBwdArgs {
  const float* x; const float* img;
  const float *dy, *dz0, *dmu, *dlv;
  int B, T, training;
  const float *rec, *trec;
  float* part;
  float* dx;
};

__global__ __launch_bounds__(LNT) void k_lat_bwd(LatGeom g, LatBwdArgs a) {
  using lrnde::fma_;
  const LatSmem s = lat_carve(g, true);
  const int tid = threadIdx.x, n = tid & (LNB - 1), j = tid >> 3;
  const int b0 = blockIdx.x * LNB, nvalid = min(LNB, a.B - b0);
  const int H = g.H, L = g.L, F = g.F, N = g.N, T = a.T;
  lat_load_weights(g, a.img, s.w);
  lat_mask_table(g, a.x, b0, nvalid, T, s.m8);
  const float* wA = s.w;
  const float* wB = s.w + g.offB;
  const float* wD = s.w + g.offD;
  const float* wE = a.img + g.offE;
  const float* wG = a.img + g.offG;
  float* part = a.part + (size_t)blockIdx.x * g.wimg;
  const float* trec = a.trec + (size_t)blockIdx.x * g.TW * LNB;
  // ---- tail: reparameterisation and rec_to_gen ----
  for (int e = tid; e < 3 * L * LNB; e += LNT) {   // y -> yb, g1 -> c
    if (e < 2 * L * LNB) s.yb[e] = trec[e];
    else s.c[e - 2 * L * LNB] = trec[e];
  }
  for (int i = j; i < N; i += LNJ) {
    float gmu = 0.f, glv = 0.f;
    if (n < nvalid) {
      const size_t gi = (size_t)(b0 + n) * N + i;
      const float dz = a.dz0 ? a.dz0[gi] : 0.f, dm = a.dmu ? a.dmu[gi] : 0.f, dl = a.dlv ? a.dlv[gi] : 0.f;
      if (a.training) {   // z0 = mu + exp(logvar / 2) * eps
        const float ev = trec[(3 * L + i) * LNB + n], ep = trec[(3 * L + N + i) * LNB + n];
        gmu = dz + dm;
        glv = (dz * ep) * (ev * 0.5f) + dl;
      } else {            // z0 = mu0 = logvar = mu
        gmu = (dz + dm) + dl;
      }
    }
    s.o2[i * LNB + n] = gmu;
    s.o2[(N + i) * LNB + n] = glv;
  }
  __syncthreads();
  for (int k = j; k < L; k += LNJ) {   // d g1 -> d (pre-activation of rec_to_gen's first layer), kept in dzs
    float acc = 0.f;
    for (int o = 0; o < 2 * N; ++o) acc = fma_(wG[k * g.OPG + o], s.o2[o * LNB + n], acc);
    const float g1 = s.c[k * LNB + n];
    s.dzs[k * LNB + n] = acc * (1.0f - g1 * g1);
  }
  for (int e = tid; e < g.wimg - g.offG; e += LNT) {   // rec_to_gen's second layer
    const int row = e / g.OPG, o = e % g.OPG;
    float acc = 0.f;
    if (o < 2 * N && row <= L)
      for (int nn = 0; nn < nvalid; ++nn) acc = fma_(s.o2[o * LNB + nn], row < L ? s.c[row * LNB + nn] : 1.0f, acc);
    part[g.offG + e] = acc;
  }
  __syncthreads();
  for (int i = j; i < 2 * L; i += LNJ) {
    float acc = 0.f;
    for (int k = 0; k < L; ++k) acc = fma_(wE[i * g.OPE + k], s.dzs[k * LNB + n], acc);
    // (a cotangent of y itself, Recurrence used alone, joins here)
    s.dY[i * LNB + n] = a.dy ? acc + (n < nvalid ? a.dy[(size_t)(b0 + n) * 2 * L + i] : 0.f) : acc;
  }
  for (int e = tid; e < g.offG - g.offE; e += LNT) {   // rec_to_gen's first layer
    const int row = e / g.OPE, k = e % g.OPE;
    float acc = 0.f;
    if (k < L)
      for (int nn = 0; nn < nvalid; ++nn) acc = fma_(s.dzs[k * LNB + nn], row < 2 * L ? s.yb[row * LNB + nn] : 1.0f, acc);
    part[g.offE + e] = acc;
  }
  for (int e = tid; e < g.ldsw; e += LNT) part[e] = 0.f;   // (the thread that continues element e below)
  __syncthreads();
  float* dY = s.dY;
  float* dYn = s.dYn;
  const float* rec_tile = a.rec + (size_t)blockIdx.x * T * g.RW * LNB;
  for (int t = T - 1; t >= 0; --t) {
    if (!lat_any(s.m8, t)) {
      if (a.dx)
        for (int e = tid; e < F * LNB; e += LNT) {
          const int nn = e / F, f = e % F;
          if (nn < nvalid) a.dx[((size_t)(b0 + nn) * T + t) * F + f] = 0.f;
        }
      continue;
    }
    const float* rec = rec_tile + (size_t)t * g.RW * LNB;
    lat_load_x(g, a.x, b0, nvalid, T, t, s.xs);
    for (int e = tid; e < g.RW * LNB; e += LNT) {
      const float v = rec[e];
      const int row = e / LNB;
      if (row < 2 * L) s.yb[e] = v;
      else if (row < 2 * L + 3 * H) s.h1[e - 2 * L * LNB] = v;
      else s.ug[e - (2 * L + 3 * H) * LNB] = v;   // ug, rg, sg are contiguous
    }
    __syncthreads();
    const bool m = s.m8[t * LNB + n] != 0;
    // P1: the convex combination and the mask
    for (int l = j; l < L; l += LNJ) {
      const float gm = dY[l * LNB + n], gs = dY[(L + l) * LNB + n];
      float dzs = 0.f, dzu = 0.f, pm = gm, ps = gs;
      if (m) {
        const float u = s.ug[l * LNB + n], sv = s.sg[l * LNB + n], ym = s.yb[l * LNB + n], ys = s.yb[(L + l) * LNB + n];
        const float dsv = (1.0f - u) * (gm + gs);
        const float du = (ym - sv) * gm + (ys - sv) * gs;
        dzs = dsv * (1.0f - sv * sv);
        dzu = du * lrnde::sigmoid_deriv_c(u);
        pm = u * gm;
        ps = u * gs;
      }
      s.dzs[l * LNB + n] = dzs;
      s.dz2[l * LNB + n] = dzu;
      dYn[l * LNB + n] = pm;
      dYn[(L + l) * LNB + n] = ps;
    }
    __syncthreads();
    // P2: through new_state's second layer (std rows) and update_gate's second layer
    for (int it = j; it < 2 * H; it += LNJ) {
      const int k = it % H;
      float acc = 0.f;
      if (it < H) {
        for (int l = 0; l < L; ++l) acc = fma_(wB[k * g.OPB + l], s.dz2[l * LNB + n], acc);
        const float h = s.h1[k * LNB + n];
        s.dz1[k * LNB + n] = acc * (1.0f - h * h);
      } else {
        for (int l = 0; l < L; ++l) acc = fma_(wD[k * g.OPD + l], s.dzs[l * LNB + n], acc);
        const float h = s.h1[(2 * H + k) * LNB + n];
        s.dz1[(2 * H + k) * LNB + n] = acc * (1.0f - h * h);
      }
    }
    __syncthreads();
    // P3: d vcat(y_mean .* r, y_std .* r)
    for (int i = j; i < 2 * L; i += LNJ) {
      const float* wp = wA + (F + i) * g.OPA + 2 * H;
      float acc = 0.f;
      for (int k = 0; k < H; ++k) acc = fma_(wp[k], s.dz1[(2 * H + k) * LNB + n], acc);
      s.dc[i * LNB + n] = acc;
    }
    __syncthreads();
    // P4: the reset gate
    for (int l = j; l < L; l += LNJ) {
      const float r = s.rg[l * LNB + n], ym = s.yb[l * LNB + n], ys = s.yb[(L + l) * LNB + n];
      const float d0 = s.dc[l * LNB + n], d1 = s.dc[(L + l) * LNB + n];
      const float dr = d0 * ym + d1 * ys;
      s.dz2[(L + l) * LNB + n] = dr * lrnde::sigmoid_deriv_c(r);
      dYn[l * LNB + n] = dYn[l * LNB + n] + d0 * r;
      dYn[(L + l) * LNB + n] = dYn[(L + l) * LNB + n] + d1 * r;
    }
    __syncthreads();
    // P5: through reset_gate's second layer
    for (int k = j; k < H; k += LNJ) {
      float acc = 0.f;
      for (int l = 0; l < L; ++l) acc = fma_(wB[k * g.OPB + L + l], s.dz2[(L + l) * LNB + n], acc);
      const float h = s.h1[(H + k) * LNB + n];
      s.dz1[(H + k) * LNB + n] = acc * (1.0f - h * h);
    }
    __syncthreads();
    // P6: the carry through u1 and r1, and dx_t through all three first layers
    for (int i = j; i < 2 * L; i += LNJ) {
      const float* wp = wA + (F + i) * g.OPA;
      float acc = 0.f;
      for (int o = 0; o < 2 * H; ++o) acc = fma_(wp[o], s.dz1[o * LNB + n], acc);
      dYn[i * LNB + n] = dYn[i * LNB + n] + acc;
    }
    if (a.dx)
      for (int f = j; f < F; f += LNJ) {
        const float* wp = wA + f * g.OPA;
        float acc = 0.f;
        for (int o = 0; o < 3 * H; ++o) acc = fma_(wp[o], s.dz1[o * LNB + n], acc);
        if (n < nvalid) a.dx[((size_t)(b0 + n) * T + t) * F + f] = acc;
      }
    // P7: the parameter cotangent of the tile, one chain per image element (columns in column order)
    for (int e = tid; e < g.ldsw; e += LNT) {
      float acc = part[e];
      if (e < g.offB) {
        const int row = e / g.OPA, o = e % g.OPA;
        if (o >= 3 * H) continue;
        const float* dz = s.dz1 + o * LNB;
        if (row < F) {
          for (int nn = 0; nn < nvalid; ++nn) acc = fma_(dz[nn], s.xs[row * LNB + nn], acc);
        } else if (row < F + 2 * L) {
          const int i = row - F;
          if (o < 2 * H) {
            for (int nn = 0; nn < nvalid; ++nn) acc = fma_(dz[nn], s.yb[i * LNB + nn], acc);
          } else {
            const float* r = s.rg + (i < L ? i : i - L) * LNB;
            for (int nn = 0; nn < nvalid; ++nn) acc = fma_(dz[nn], s.yb[i * LNB + nn] * r[nn], acc);
          }
        } else {
          for (int nn = 0; nn < nvalid; ++nn) acc = fma_(dz[nn], 1.0f, acc);
        }
      } else if (e < g.offD) {
        const int q = e - g.offB, row = q / g.OPB, o = q % g.OPB;
        if (o >= 2 * L) continue;
        const float* dz = s.dz2 + o * LNB;
        const float* in = s.h1 + ((o < L ? 0 : H) + row) * LNB;
        for (int nn = 0; nn < nvalid; ++nn) acc = fma_(dz[nn], row < H ? in[nn] : 1.0f, acc);
      } else {
        const int q = e - g.offD, row = q / g.OPD, o = q % g.OPD;
        if (o >= L || row > H) continue;
        const float* dz = s.dzs + o * LNB;
        const float* in = s.h1 + (2 * H + row) * LNB;
        for (int nn = 0; nn < nvalid; ++nn) acc = fma_(dz[nn], row < H ? in[nn] : 1.0f, acc);
      }
      part[e] = acc;
    }
    __syncthreads();
    float* tmp = dY; dY = dYn; dYn = tmp;
  }
}

// ---- decode + loss ----
struct LatDecArgs {
  const float *series, *pg, *data, *mask, *mu, *lv;
  int T, B, I, N;
  float w_kl, two_sig2, sig2, log_sig, half_log_2pi;
  float *ll, *kl, *dseries, *dmu, *dlv;
  float *dpred, *gpart;   // workspaces: (B, T, I) and (B, I*N + I)
};
struct LatDecOut { double loss; double nll; double klm; };

constexpr int LDT = 256;

__global__ __launch_bounds__(LDT) void k_lat_dec(LatDecArgs a) {
  using lrnde::fma_;
  extern __shared__ __attribute__((aligned(16))) char lat_smem[];
  double* red = reinterpret_cast<double*>(lat_smem);
  float* W = reinterpret_cast<float*>(red + LDT);
  const int tid = threadIdx.x, b = blockIdx.x, T = a.T, B = a.B, I = a.I, N = a.N;
  const int PG = I * N + I;
  for (int e = tid; e < PG; e += LDT) W[e] = a.pg[e];
  // sum(mask; dims=(1, 2)) of the column (utils.jl:97)
  double ms = 0.0;
  for (int e = tid; e < T * I; e += LDT) ms += (double)a.mask[(size_t)b * T * I + e];
  red[tid] = ms;
  __syncthreads();
  for (int st = LDT / 2; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  const float msum = (float)red[0];
  __syncthreads();
  // d loss / d (pred .* mask - data .* mask) = d / (sigma^2 * B * msum)
  const float inv = 1.0f / ((a.sig2 * (float)B) * msum);
  double acc_ll = 0.0;
  for (int e = tid; e < T * I; e += LDT) {
    const int t = e / I, i = e % I;
    const float* z = a.series + ((size_t)t * B + b) * N;
    float p = 0.f;
    for (int k = 0; k < N; ++k) p = fma_(W[i + k * I], z[k], p);
    p = p + W[I * N + i];
    const float mk = a.mask[(size_t)b * T * I + e];
    const float d = p * mk - a.data[(size_t)b * T * I + e] * mk;
    const float term = (-(d * d) / a.two_sig2 - a.log_sig) - a.half_log_2pi;   // utils.jl:96
    acc_ll += (double)term;
    a.dpred[(size_t)b * T * I + e] = (d * inv) * mk;
  }
  red[tid] = acc_ll;
  __syncthreads();
  for (int st = LDT / 2; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    a.ll[b] = (float)red[0] / msum;
    // kl_divergence (utils.jl:101): mean over the rows of exp(logvar) + mu^2 - 1 - logvar, halved
    float sk = 0.f;
    for (int k = 0; k < N; ++k) {
      const float mu = a.mu[(size_t)b * N + k], lv = a.lv[(size_t)b * N + k];
      sk = sk + (((lrnde::expf_c(lv) + mu * mu) - 1.0f) - lv);
    }
    a.kl[b] = (sk / (float)N) / 2.0f;
  }
  for (int k = tid; k < N; k += LDT) {
    const float mu = a.mu[(size_t)b * N + k], lv = a.lv[(size_t)b * N + k];
    const float c = a.w_kl / (float)B;
    if (a.dmu) a.dmu[(size_t)b * N + k] = c * (mu / (float)N);
    if (a.dlv) a.dlv[(size_t)b * N + k] = c * ((lrnde::expf_c(lv) - 1.0f) / (2.0f * (float)N));
  }
  __syncthreads();   // dpred of this column is complete (written and read by this workgroup only)
  const float* dp = a.dpred + (size_t)b * T * I;
  if (a.dseries)
    for (int e = tid; e < T * N; e += LDT) {
      const int t = e / N, k = e % N;
      float acc = 0.f;
      for (int i = 0; i < I; ++i) acc = fma_(W[i + k * I], dp[t * I + i], acc);
      a.dseries[((size_t)t * B + b) * N + k] = acc;
    }
  if (a.gpart)
    for (int e = tid; e < PG; e += LDT) {
      const int i = e < I * N ? e % I : e - I * N, k = e < I * N ? e / I : N;
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc = fma_(dp[t * I + i], k < N ? a.series[((size_t)t * B + b) * N + k] : 1.0f, acc);
      a.gpart[(size_t)b * PG + e] = acc;
    }
}

// gen_to_data alone: y[b][t][i] for every saved state (construct.jl:250)
__global__ void k_lat_pred(const float* series, const float* pg, int T, int B, int I, int N, float* pred) {
  const size_t total = (size_t)B * T * I;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e % I), t = (int)((e / I) % T), b = (int)(e / ((size_t)I * T));
    const float* z = series + ((size_t)t * B + b) * N;
    float p = 0.f;
    for (int k = 0; k < N; ++k) p = lrnde::fma_(pg[i + k * I], z[k], p);
    pred[e] = p + pg[I * N + i];
  }
}

// loss = -mean(ll - w_kl * kl) (construct.jl:50), the stats' means, and gen_to_data's cotangent: columns in column order
__global__ void k_lat_dec_sum(int B, int PG, float w_kl, const float* ll, const float* kl, const float* gpart, float* dpg,
                              LatDecOut* out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < PG && dpg) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = acc + gpart[(size_t)b * PG + e];
    dpg[e] = acc;
  }
  if (e == 0) {
    double s = 0.0, sl = 0.0, sk = 0.0;
    for (int b = 0; b < B; ++b) {
      s += (double)(ll[b] - w_kl * kl[b]);
      sl += (double)ll[b];
      sk += (double)kl[b];
    }
    out->loss = -s / (double)B;
    out->nll = -sl / (double)B;
    out->klm = sk / (double)B;
  }
}

}  // namespace

// ---- the handle ----
struct lrnde_latent {
  int device = 0;
  hipStream_t stream = nullptr;
  lrnde_latent_desc desc{};
  LatGeom g{};
  int max_lds = 0;
  bool have_params = false;
  DevBuf<float> img, pg, rec, trec, part, dpred, gpart, llkl;
  DevBuf<LatDecOut> dec_out;
  PinBuf<LatDecOut> dec_host;
  size_t lds_set_fwd = 0, lds_set_bwd = 0;
  bool rec_valid = false;
  uint64_t rec_gen = 0;
  int rec_B = 0, rec_T = 0, rec_training = 0;
  int launches_fwd = 0, launches_bwd = 0;
  std::string err;
};

namespace {
thread_local std::string g_lat_create_err;

// this handle's names for the library's formatter and HIP check (lrnde_fail.hpp); without a handle (a refused create)
// the message goes to the thread's create-error string
inline std::string* lat_err(lrnde_latent* h) { return h ? &h->err : &g_lat_create_err; }
#define lat_fail(h, ...) lrnde::failf(lat_err(h), __VA_ARGS__)
#define LATCHK(h, x) LRNDE_HIPCHK(lat_err(h), x)

bool lat_desc_ok(const lrnde_latent_desc* d) {
  return d && d->in_dims >= 1 && d->hidden_dims >= 1 && d->latent_dims >= 1 && d->node_dims >= 1 && d->in_dims <= (1 << 14) &&
         d->hidden_dims <= (1 << 14) && d->latent_dims <= (1 << 14) && d->node_dims <= (1 << 14);
}
}  // namespace

extern "C" {

size_t lrnde_latent_param_count(const lrnde_latent_desc* d) {
  if (!lat_desc_ok(d)) return 0;
  const size_t I = d->in_dims, H = d->hidden_dims, L = d->latent_dims, N = d->node_dims, K = 2 * L + 2 * I + 1;
  return 3 * (H * K + H) + 2 * (L * H + L) + (2 * L * H + 2 * L) + (L * 2 * L + L) + (2 * N * L + 2 * N) + (I * N + I);
}

const char* lrnde_latent_last_error(const lrnde_latent* h) {
  if (h) return h->err.c_str();
  return g_lat_create_err.empty() ? "null latent handle" : g_lat_create_err.c_str();
}

int lrnde_latent_create(lrnde_latent** out, const lrnde_latent_desc* d, int device, void* stream) {
  g_lat_create_err.clear();
  if (!out) return lat_fail(nullptr, LRNDE_BADARG, "null pointer");
  *out = nullptr;
  if (!lat_desc_ok(d)) return lat_fail(nullptr, LRNDE_BADARG, "every dimension of a latent descriptor must be in 1..16384");
  if (3 * d->hidden_dims > 2 * LNJ)
    return lat_fail(nullptr, LRNDE_UNSUPPORTED, "hidden_dims = %d: the three first layers side by side hold at most %d rows (hidden_dims <= %d)",
                    d->hidden_dims, 2 * LNJ, 2 * LNJ / 3);
  const LatGeom g = lat_geom(*d);
  if (hipSetDevice(device) != hipSuccess) return lat_fail(nullptr, LRNDE_HIP_ERROR, "hipSetDevice(%d) failed", device);
  const int max_lds = 160 * 1024;   // LDS of a gfx950 CU (set_smem_attr in lrnde_kernels.hip uses the same figure)
  const size_t need = lat_smem_bytes(g, true, 1);
  if (need > (size_t)max_lds)
    return lat_fail(nullptr, LRNDE_UNSUPPORTED,
                    "in/hidden/latent/node = %d/%d/%d/%d: the gates' weight image (%d bytes) and the backward's activations need %zu bytes "
                    "of LDS, the device has %d", d->in_dims, d->hidden_dims, d->latent_dims, d->node_dims, g.ldsw * 4, need, max_lds);
  lrnde_latent* h = new lrnde_latent();
  h->device = device; h->stream = (hipStream_t)stream; h->desc = *d; h->g = g; h->max_lds = max_lds;
  *out = h;
  return LRNDE_OK;
}

int lrnde_latent_destroy(lrnde_latent* h) {
  if (!h) return LRNDE_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  delete h;   // (the buffers are DevBuf / PinBuf members)
  return LRNDE_OK;
}

int lrnde_latent_set_params(lrnde_latent* h, const float* p, size_t n) {
  if (!h) return LRNDE_BADARG;
  if (!p || n != lrnde_latent_param_count(&h->desc))
    return lat_fail(h, LRNDE_BADARG, "the parameter vector has %zu entries, the descriptor needs %zu", n, lrnde_latent_param_count(&h->desc));
  LATCHK(h, hipSetDevice(h->device));
  const LatGeom& g = h->g;
  const size_t PG = (size_t)g.I * g.N + g.I;
  LATCHK(h, h->img.once(g.wimg));
  LATCHK(h, h->pg.once(PG));
  hipLaunchKernelGGL(k_lat_pack, dim3((g.wimg + 255) / 256), dim3(256), 0, h->stream, g, p, h->img.get());
  LATCHK(h, hipGetLastError());
  LATCHK(h, hipMemcpyAsync(h->pg.get(), p + g.P, sizeof(float) * PG, hipMemcpyDeviceToDevice, h->stream));
  h->have_params = true;
  h->rec_valid = false;
  return LRNDE_OK;
}

int lrnde_latent_encode(lrnde_latent* h, const float* x, int32_t B, int32_t T, int32_t training, const float* eps, float* y, float* mu,
                        float* logvar, float* z0) {
  if (!h) return LRNDE_BADARG;
  if (!h->have_params) return lat_fail(h, LRNDE_BADARG, "lrnde_latent_set_params has not been called");
  if (!x || B <= 0 || T <= 0 || (training && !eps)) return lat_fail(h, LRNDE_BADARG, "bad argument (x, B >= 1, T >= 1; eps in training mode)");
  const LatGeom& g = h->g;
  const size_t lds = lat_smem_bytes(g, false, T), lds_b = lat_smem_bytes(g, true, T);
  if (T > LAT_MAX_T || lds_b > (size_t)h->max_lds)
    return lat_fail(h, LRNDE_UNSUPPORTED, "T = %d: the mask table of the steps does not fit LDS next to the weights (%zu of %d bytes)", T, lds_b,
                    h->max_lds);
  LATCHK(h, hipSetDevice(h->device));
  h->rec_valid = false;
  const int nwg = (B + LNB - 1) / LNB;
  LATCHK(h, h->rec.grow((size_t)nwg * T * g.RW * LNB));
  LATCHK(h, h->trec.grow((size_t)nwg * g.TW * LNB));
  if (lds > h->lds_set_fwd) {
    LATCHK(h, hipFuncSetAttribute((const void*)k_lat_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->lds_set_fwd = lds;
  }
  LatFwdArgs a{};
  a.x = x; a.eps = eps; a.img = h->img.get(); a.B = B; a.T = T; a.training = training ? 1 : 0;
  a.y = y; a.mu = mu; a.lv = logvar; a.z0 = z0; a.rec = h->rec.get(); a.trec = h->trec.get();
  hipLaunchKernelGGL(k_lat_fwd, dim3(nwg), dim3(LNT), lds, h->stream, g, a);
  LATCHK(h, hipGetLastError());
  h->launches_fwd = 1;
  h->rec_valid = true; h->rec_gen += 1; h->rec_B = B; h->rec_T = T; h->rec_training = a.training;
  return LRNDE_OK;
}

int lrnde_latent_encode_backward(lrnde_latent* h, const float* x, int32_t B, int32_t T, const float* dy, const float* dz0,
                                 const float* dmu, const float* dlogvar, float* dx, float* dp) {
  if (!h) return LRNDE_BADARG;
  if (!h->rec_valid) return lat_fail(h, LRNDE_BADARG, "no recorded encode to differentiate (none yet, consumed, or the parameters changed)");
  if (!x || !dp || B != h->rec_B || T != h->rec_T)
    return lat_fail(h, LRNDE_BADARG, "bad argument: the record is of B = %d, T = %d", h->rec_B, h->rec_T);
  LATCHK(h, hipSetDevice(h->device));
  const LatGeom& g = h->g;
  const int nwg = (B + LNB - 1) / LNB;
  const size_t lds = lat_smem_bytes(g, true, T);
  LATCHK(h, h->part.grow((size_t)nwg * g.wimg));
  if (lds > h->lds_set_bwd) {
    LATCHK(h, hipFuncSetAttribute((const void*)k_lat_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->lds_set_bwd = lds;
  }
  LatBwdArgs a{};
  a.x = x; a.img = h->img.get(); a.dy = dy; a.dz0 = dz0; a.dmu = dmu; a.dlv = dlogvar; a.B = B; a.T = T; a.training = h->rec_training;
  a.rec = h->rec.get(); a.trec = h->trec.get(); a.part = h->part.get(); a.dx = dx;
  h->rec_valid = false;   // one backward per record
  hipLaunchKernelGGL(k_lat_bwd, dim3(nwg), dim3(LNT), lds, h->stream, g, a);
  const int ne = g.wimg + g.L * g.H + g.L;
  hipLaunchKernelGGL(k_lat_pgsum, dim3((ne + 255) / 256), dim3(256), 0, h->stream, g, (const float*)h->part.get(), nwg, dp);
  LATCHK(h, hipGetLastError());
  h->launches_bwd = 2;
  return LRNDE_OK;
}

int lrnde_latent_decode_loss(lrnde_latent* h, const float* series, int32_t T, int32_t B, const float* data, const float* mask, const float* mu,
                             const float* logvar, float w_kl, float* loss_host, float* ll, float* kl, float* dseries, float* dmu,
                             float* dlogvar, float* dpg) {
  if (!h) return LRNDE_BADARG;
  if (!h->have_params) return lat_fail(h, LRNDE_BADARG, "lrnde_latent_set_params has not been called");
  if (!series || !data || !mask || !mu || !logvar || !loss_host || T <= 0 || B <= 0) return lat_fail(h, LRNDE_BADARG, "bad argument");
  LATCHK(h, hipSetDevice(h->device));
  const LatGeom& g = h->g;
  const int PG = g.I * g.N + g.I;
  const size_t lds = sizeof(double) * LDT + sizeof(float) * PG;
  if (lds > 60 * 1024) return lat_fail(h, LRNDE_UNSUPPORTED, "gen_to_data's %d parameters do not fit the decode kernel's LDS", PG);
  LATCHK(h, h->dpred.grow((size_t)B * T * g.I));
  LATCHK(h, h->gpart.grow((size_t)B * PG));
  LATCHK(h, h->llkl.grow((size_t)2 * B));
  LATCHK(h, h->dec_out.once(1));
  LATCHK(h, h->dec_host.once(1));
  LatDecArgs a{};
  a.series = series; a.pg = h->pg.get(); a.data = data; a.mask = mask; a.mu = mu; a.lv = logvar;
  a.T = T; a.B = B; a.I = g.I; a.N = g.N; a.w_kl = w_kl;
  const float sig = 0.01f;                        // utils.jl:95
  a.sig2 = sig * sig; a.two_sig2 = 2.0f * (sig * sig); a.log_sig = logf(sig); a.half_log_2pi = logf((float)(2.0 * M_PI)) / 2.0f;
  a.ll = ll ? ll : h->llkl.get(); a.kl = kl ? kl : h->llkl.get() + B;
  a.dseries = dseries; a.dmu = dmu; a.dlv = dlogvar; a.dpred = h->dpred.get(); a.gpart = dpg ? h->gpart.get() : nullptr;
  hipLaunchKernelGGL(k_lat_dec, dim3(B), dim3(LDT), lds, h->stream, a);
  hipLaunchKernelGGL(k_lat_dec_sum, dim3((PG + 255) / 256), dim3(256), 0, h->stream, (int)B, PG, w_kl, (const float*)a.ll, (const float*)a.kl,
                     (const float*)h->gpart.get(), dpg, h->dec_out.get());
  LATCHK(h, hipGetLastError());
  LATCHK(h, hipMemcpyAsync(h->dec_host.get(), h->dec_out.get(), sizeof(LatDecOut), hipMemcpyDeviceToHost, h->stream));
  LATCHK(h, hipStreamSynchronize(h->stream));
  loss_host[0] = (float)h->dec_host.get()->loss;
  loss_host[1] = (float)h->dec_host.get()->nll;
  loss_host[2] = (float)h->dec_host.get()->klm;
  return LRNDE_OK;
}

int lrnde_latent_decode(lrnde_latent* h, const float* series, int32_t T, int32_t B, float* pred) {
  if (!h) return LRNDE_BADARG;
  if (!h->have_params) return lat_fail(h, LRNDE_BADARG, "lrnde_latent_set_params has not been called");
  if (!series || !pred || T <= 0 || B <= 0) return lat_fail(h, LRNDE_BADARG, "bad argument");
  LATCHK(h, hipSetDevice(h->device));
  const LatGeom& g = h->g;
  const size_t total = (size_t)B * T * g.I;
  int nb = (int)((total + 255) / 256); if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(k_lat_pred, dim3(nb), dim3(256), 0, h->stream, series, (const float*)h->pg.get(), (int)T, (int)B, g.I, g.N, pred);
  LATCHK(h, hipGetLastError());
  return LRNDE_OK;
}

int lrnde_latent_record_generation(lrnde_latent* h, uint64_t* gen_host) {
  if (!h || !gen_host) return LRNDE_BADARG;
  *gen_host = h->rec_valid ? h->rec_gen : 0;
  return LRNDE_OK;
}

int lrnde_latent_last_launches(lrnde_latent* h, int32_t* encode_host, int32_t* backward_host) {
  if (!h || !encode_host || !backward_host) return LRNDE_BADARG;
  *encode_host = h->launches_fwd; *backward_host = h->launches_bwd;
  return LRNDE_OK;
}

}  // extern "C"
