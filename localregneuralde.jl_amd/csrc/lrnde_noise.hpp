// lrnde_noise.hpp — Gaussian noise for the SDE layers, drawn on the handle's device from a seed.
// Included by lrnde_kernels.hip after lrnde_sde_node.hpp.
//
// Counter-based: normal j (step index) of column c = b*D + d in stream s comes from the Philox-4x32-10 block (Salmon et
// al., SC'11) with counter (j >> 2, c, s, 0) and key (seed & 0xffffffff, seed >> 32); the block's words x0..x3 give
// normals 4q..4q+3 by Box-Muller on the pairs (x0, x1) and (x2, x3).  A column's noise thus depends on (seed, s, b, d, j)
// alone — not on B, on nsteps or on the launch shape.  Uniforms u = ((x >> 8) + 0.5) * 2^-24 are exact in float64 and lie
// in (0, 1); Box-Muller runs in float64 and rounds once to float32, so a float64 restatement (tests/philox_np.py) agrees
// to within one float32 ulp and almost always bit for bit.  The scale and the path's running sum are single fp32
// operations in sequential order: exactly np.cumsum(z.astype(f32) * f32(scale), dtype=f32).
// Also here: the C entry points of the virtual path tree (lrnde_sde_tree_path, lrnde_sde_set_path_tree; lrnde_sde_tree.hpp).

namespace {

constexpr int NZ_COLS = 64;    // columns of one workgroup (one wave wide)
constexpr int NZ_ROWS = 128;   // steps generated into LDS per pass (32 KB)
constexpr int NZ_NT = 256;

// (philox4x32_10, noise_u01 and box_muller: lrnde_sde_tree.hpp, which draws the same normals)

// One workgroup per 64 columns.  Per pass of NZ_ROWS steps its four waves generate the standard normals into LDS (a wave
// covers the 64 columns of one counter block: conflict-free LDS rows), then either every thread writes scale * z row by
// row (increments), or wave 0 runs the sequential sum of its column (path).  Rows are written 64 columns wide (coalesced).
// out: (nsteps + cumulative) x ncols, row-major, 64-bit indexing.
__global__ __launch_bounds__(NZ_NT) void k_sde_noise(uint32_t k0, uint32_t k1, uint32_t s, int32_t nsteps, uint32_t ncols,
                                                     float scale, int32_t cumulative, float* __restrict__ out) {
  __shared__ float z[NZ_ROWS][NZ_COLS];
  const uint32_t col0 = blockIdx.x * (uint32_t)NZ_COLS;
  const int lc = threadIdx.x & (NZ_COLS - 1);
  const uint32_t c = col0 + lc;
  const bool scan = cumulative && threadIdx.x < NZ_COLS && c < ncols;
  float acc = 0.f;
  if (scan) out[c] = 0.f;
  for (int j0 = 0; j0 < nsteps; j0 += NZ_ROWS) {
    const int rows = min(NZ_ROWS, nsteps - j0);
    const int nq = (rows + 3) >> 2;
    if (c < ncols) {
      for (int qq = threadIdx.x / NZ_COLS; qq < nq; qq += NZ_NT / NZ_COLS) {
        uint32_t x[4];
        philox4x32_10((uint32_t)(j0 >> 2) + qq, c, s, 0u, k0, k1, x);
        float z0, z1, z2, z3;
        box_muller(x[0], x[1], z0, z1);
        box_muller(x[2], x[3], z2, z3);
        z[4 * qq + 0][lc] = z0; z[4 * qq + 1][lc] = z1; z[4 * qq + 2][lc] = z2; z[4 * qq + 3][lc] = z3;
      }
    }
    __syncthreads();
    if (cumulative) {
      if (scan)
        for (int r = 0; r < rows; ++r) {
          acc = __fadd_rn(acc, __fmul_rn(z[r][lc], scale));
          out[(size_t)(j0 + r + 1) * ncols + c] = acc;
        }
    } else {
      for (int i = threadIdx.x; i < rows * NZ_COLS; i += NZ_NT) {
        const int r = i / NZ_COLS, cl = i & (NZ_COLS - 1);
        if (col0 + cl < ncols) out[(size_t)(j0 + r) * ncols + col0 + cl] = __fmul_rn(z[r][cl], scale);
      }
    }
    __syncthreads();
  }
}

__global__ void k_philox_hook(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) philox4x32_10(c0, c1, c2, c3, k0, k1, out);
}

}  // namespace

extern "C" {

int lrnde_sde_draw_noise(lrnde_sde* s, uint64_t seed, uint32_t stream, int32_t nsteps, int32_t B, float scale,
                         int32_t cumulative, float* out) {
  if (!s) return LRNDE_BADARG;
  lrnde_ctx* c = s->drift;
  if (nsteps < 0) return fail(c, LRNDE_BADARG, "nsteps must be non-negative (got %d)", nsteps);
  if (B <= 0) return fail(c, LRNDE_BADARG, "batch must be positive (got %d)", B);
  if (!out) return fail(c, LRNDE_BADARG, "null output pointer");
  if (!isfinite(scale)) return fail(c, LRNDE_BADARG, "scale must be finite (got %g)", (double)scale);
  if (cumulative != 0 && cumulative != 1) return fail(c, LRNDE_BADARG, "cumulative must be 0 (increments) or 1 (path)");
  const uint64_t ncols = (uint64_t)B * (uint64_t)c->desc.state_dim;
  if (ncols > (1ull << 30)) return fail(c, LRNDE_BADARG, "B x D = %llu columns: at most 2^30", (unsigned long long)ncols);
  if (nsteps + cumulative == 0) return LRNDE_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const unsigned nwg = (unsigned)((ncols + NZ_COLS - 1) / NZ_COLS);
  hipLaunchKernelGGL(k_sde_noise, dim3(nwg), dim3(NZ_NT), 0, c->stream, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
                     stream, nsteps, (uint32_t)ncols, scale, cumulative, out);
  HIPCHK(c, hipGetLastError());
  return LRNDE_OK;
}

// the virtual path tree (lrnde_sde_tree.hpp) as an array: what every tree-mode solve queries, for callers that want to look at it
int lrnde_sde_tree_path(lrnde_sde* s, uint64_t seed, uint32_t stream, int32_t levels, int32_t B, float t0, float t2, float* out) {
  if (!s) return LRNDE_BADARG;
  lrnde_ctx* c = s->drift;
  if (levels < 0 || levels > TREE_MAXL) return fail(c, LRNDE_BADARG, "levels must lie in 0..%d (got %d)", TREE_MAXL, levels);
  if (B <= 0) return fail(c, LRNDE_BADARG, "batch must be positive (got %d)", B);
  if (!out) return fail(c, LRNDE_BADARG, "null output pointer");
  if (!(t2 > t0) || !isfinite(t2 - t0)) return fail(c, LRNDE_BADARG, "t2 must lie after t0");
  const uint64_t ncols = (uint64_t)B * (uint64_t)c->desc.state_dim;
  if (ncols > (1ull << 30)) return fail(c, LRNDE_BADARG, "B x D = %llu columns: at most 2^30", (unsigned long long)ncols);
  HIPCHK(c, hipSetDevice(c->device));
  SdeTree T{};
  T.on = 1; T.k0 = (uint32_t)(seed & 0xffffffffu); T.k1 = (uint32_t)(seed >> 32); T.L = levels;
  sde_tree_scales(T, t2 - t0);
  hipLaunchKernelGGL(k_sde_tree_path, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, c->stream, T, stream, (uint32_t)ncols, out);
  HIPCHK(c, hipGetLastError());
  return LRNDE_OK;
}

int lrnde_sde_set_path_tree(lrnde_sde* s, int32_t enable, uint64_t seed) {
  if (!s) return LRNDE_BADARG;
  if (enable != 0 && enable != 1) return fail(s->drift, LRNDE_BADARG, "enable must be 0 or 1 (got %d)", enable);
  s->tree_on = enable != 0;
  s->tree_seed = enable ? seed : 0;
  return LRNDE_OK;
}

int lrnde_hook_sde_drift_ctx(lrnde_sde* s, lrnde_ctx** out) {
  if (!s || !out) return LRNDE_BADARG;
  *out = s->drift;
  return LRNDE_OK;
}

int lrnde_hook_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  if (!ctr || !key || !out) return LRNDE_BADARG;
  DevBuf<uint32_t> d;
  if (d.once(4) != hipSuccess) return LRNDE_HIP_ERROR;
  hipLaunchKernelGGL(k_philox_hook, dim3(1), dim3(64), 0, 0, ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], d.get());
  return hipGetLastError() == hipSuccess && hipMemcpy(out, d, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess
             ? LRNDE_OK : LRNDE_HIP_ERROR;
}

}  // extern "C"
