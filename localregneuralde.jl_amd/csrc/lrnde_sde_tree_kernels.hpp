// lrnde_sde_tree_kernels.hpp — the virtual Brownian tree (lrnde_sde_tree.hpp) as arrays, for the host-controlled loops and for
// callers that want to look at the path.  Included by lrnde_kernels.hip inside its anonymous namespace: these two kernels are
// compiled once, there.

// dW[e] = W[i + m] - W[i] of element e = column e of a (B, D) array (k_sde_dw's subtraction): the host-controlled loops' increment
__global__ __launch_bounds__(256) void k_sde_dw_tree(size_t n, SdeTree T, uint32_t stream, int i, int m, float* __restrict__ dW) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t c[1] = {(uint32_t)e};
    float hi[1], lo[1];
    tree_query<1>(T, stream, c, i + m, hi);
    tree_query<1>(T, stream, c, i, lo);
    dW[e] = hi[0] - lo[0];
  }
}

// The whole array the definition gives, out (nfine + 1) x ncols row-major: one thread per column walks the nodes in heap order
// (parents before children), four normals per Philox block; rows are written one column per thread (coalesced), a node's
// two ends are this thread's own earlier stores.  64-bit indexing.
__global__ __launch_bounds__(256) void k_sde_tree_path(SdeTree T, uint32_t stream, uint32_t ncols, float* __restrict__ out) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= ncols) return;
  const uint32_t nfine = 1u << T.L;
  volatile float* o = out;   // (read back below: no value is kept across the stores)
  o[c] = 0.f;
  for (uint32_t q = 0; q < (nfine + 3u) >> 2; ++q) {
    uint32_t x[4];
    philox4x32_10(q, c, stream, 0u, T.k0, T.k1, x);
    float z[4];
    box_muller(x[0], x[1], z[0], z[1]);
    box_muller(x[2], x[3], z[2], z[3]);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t n = 4u * q + (uint32_t)w;
      if (n >= nfine) break;
      if (n == 0u) { o[(size_t)nfine * ncols + c] = __fmul_rn(T.sT, z[0]); continue; }
      const int l = 32 - __clz((int)n);                 // level: 2^(l-1) <= n < 2^l
      const uint32_t j = n - (1u << (l - 1));
      const uint32_t half = nfine >> l, a = j * (2u * half), mid = a + half, b = mid + half;
      const float sl = ldexpf((l & 1) ? T.s1 : T.s2, -((l - 1) >> 1));
      const float wa = o[(size_t)a * ncols + c], wb = o[(size_t)b * ncols + c];
      o[(size_t)mid * ncols + c] = __fadd_rn(__fmul_rn(0.5f, __fadd_rn(wa, wb)), __fmul_rn(sl, z[w]));
    }
  }
}
