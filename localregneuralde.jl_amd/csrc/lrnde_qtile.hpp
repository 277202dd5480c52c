// lrnde_qtile.hpp — the small-batch kernel family: 4 batch columns per workgroup.
// Included by lrnde_kernels.hip inside its anonymous namespace (shares StepArgs, Ctrl, the device
// prologue, the partial-sum protocol and the canonical arithmetic).
//
// Why a second tile shape: the vector field is per-sample independent, so the batch is the only
// inter-workgroup parallelism.  With 16 columns per workgroup MNIST-ODE B=512 gives 32 workgroups
// on a 256-CU chip.  v_mfma_f32_4x4x1_16B_f32 multiplies 16 independent 4x4 blocks per
// instruction; mapping block b to rows 4b..4b+3 of a 64-row group and the 4 columns to 4 samples
// gives a 64x4 output tile per instruction with K = 1 — still one fp32 fma per product in
// increasing k (measured: tools/mfma_probe.hip), i.e. the same canonical dot product, on a
// 4-column tile: 128 workgroups at B=512.  A workgroup is 4 waves, ONE per SIMD (512 VGPRs
// each): weights stream from L2 with buffer loads one block ahead, the first block of each
// GEMM phase stays resident in registers for the whole launch.
//
// Lane roles (lane l): sample s = l & 3, row quad q = l >> 2.  A operand: W[row 64*rg + l][k];
// B operand: x[k][s]; D register r: out[row 64*rg + 4q + r][s].

constexpr int QNB = 4;    // batch columns per workgroup
constexpr int QNW = 7;    // waves per workgroup: one per canonical K-segment of Dense-1 (784 rows = 7 segments).  With 8,
                          // the eighth wave's 56 Dense-1 loads per f-eval and the second Dense-2 row group of waves 5..7
                          // were out-of-range loads (they return 0 without touching memory), and those still take the
                          // CU's address-issue slot of a real 1-KiB wave-load (tools/oor_probe.hip): 59.9 -> 56.5 us.
constexpr int QNT = QNW * 64;
constexpr int QB1 = 7;    // k-quads per Dense-1 block (a canonical segment = 28 quads = 4 blocks)
constexpr int QSEG = 28;  // k-quads per canonical segment (112 rows)
constexpr int QB2 = 4;    // k-quads per Dense-2 block
constexpr int QRGC = 4;   // Dense-2 row groups run concurrently by one wave

struct SmemQ {
  f32x4* xl;   // x tile: [KQ1p][4 samples] quads (4 consecutive rows of one sample)
  f32x4* hl;   // h tile: [KQ2p][4]
  f32x4* pl;   // Dense-1 segment partials [nseg1][RG1][64 lanes]
  float* bias; // w1t[64*RG1] b1[64*RG1] w2t[64*RG2] b2[64*RG2]
  double* red;
  Bcast* bc;
};

__device__ __forceinline__ int q_nseg1(const ModelDev& m) { return (m.KQ1p + QSEG - 1) / QSEG; }
// Dense-2 row ownership: wave w produces the rows of its own Dense-1 segment, [112w, 112w + 112), as two 64-row groups
// starting at 112w and 112w + 64 (packed groups 2w and 2w + 1 of W2q); rows 112w + 112 .. + 127 of the second group are
// the next wave's.  So the x rows a wave writes in a stage epilogue are the ones it reads in the next Dense-1.
__host__ __device__ __forceinline__ int q_w2_groups(int KQ1p) { return 2 * ((KQ1p + QSEG - 1) / QSEG); }

// sum of the nseg (<= QNW) K-segment partials of C-fragment element e, in segment order (the canonical order), with all
// LDS reads issued before the first add: a loop with the runtime trip count read, waited and added one segment at a time
__device__ __forceinline__ float q_segment_sum(const float* plf, int ne, int e, int nseg) {
  float vals[QNW];
#pragma unroll
  for (int sgi = 0; sgi < QNW; ++sgi) vals[sgi] = plf[(size_t)(sgi < nseg ? sgi : nseg - 1) * ne + e];
  float v = vals[0];
#pragma unroll
  for (int sgi = 1; sgi < QNW; ++sgi) v = sgi < nseg ? v + vals[sgi] : v;
  return v;
}

// Epilogue 1 (segment sum, time column, bias, activation of the Dense-1 rows) as straight-line code.  A thread owns the
// C-fragment element e = threadIdx.x of the RG1 * 256 (r = e & 3, lane l = (e >> 2) & 63, row group e >> 8: row
// o = 64 rg + 4 (l >> 2) + r of sample l & 3), and what it needs besides the partials depends on the launch alone:
struct Epi1Q {
  const float* p0;  // its element of segment 0's partial (LDS); element 0 for a thread that owns none
  int seg[QNW];     // float offset of segment s's partial from p0, the segments past nseg1 clamped to the last (wave-uniform)
  unsigned add;     // bit s: segment s exists and is added (wave-uniform)
  float* h;         // its h slot
  float w1, b1;     // time column and bias of its row
  bool valid;       // it owns an element, and the row lies in a Dense-2 quad (o >= H inside the padded quads included)
  bool two;         // wave-uniform: the wave's threads own a second element, threadIdx.x + QNT, that can hold such a row
};
// row of element e / float index of its h slot
__device__ __forceinline__ int q_epi1_row(int e) { return (e >> 8) * 64 + (((e >> 2) & 63) >> 2) * 4 + (e & 3); }
__device__ __forceinline__ int q_epi1_slot(int e) { return ((q_epi1_row(e) >> 2) * 4 + ((e >> 2) & 3)) * 4 + (e & 3); }
// (reads the staged bias vectors: after the barrier that orders smem_init_q / bias_write_q)
__device__ __forceinline__ Epi1Q q_epi1_make(const ModelDev& m, const SmemQ& sm) {
  static_assert(2 * QNT >= 512, "two elements per thread cover the 512 of RG1 = 2, the family's limit");
  const int ne = m.RG1 * 256, nseg1 = q_nseg1(m), h64 = m.RG1 * 64;
  const bool has = (int)threadIdx.x < ne;
  const int e = has ? (int)threadIdx.x : 0, o = q_epi1_row(e);
  Epi1Q ep;
  ep.p0 = reinterpret_cast<const float*>(sm.pl) + e;
#pragma unroll
  for (int sgi = 0; sgi < QNW; ++sgi) ep.seg[sgi] = (sgi < nseg1 ? sgi : nseg1 - 1) * ne;
  ep.add = (1u << nseg1) - 1u;
  ep.h = reinterpret_cast<float*>(sm.hl) + q_epi1_slot(e);
  ep.w1 = sm.bias[o]; ep.b1 = sm.bias[h64 + o];
  ep.valid = has && (o >> 2) < m.KQ2p;
  // the second elements are QNT .. ne - 1, all in wave 0, and their rows ascend from q_epi1_row(QNT): with RG1 = 2 and
  // KQ2p = 28 (every shape of the family today) that row is 112 = 4 KQ2p and no second element is real
  ep.two = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0 && ne > QNT && (q_epi1_row(QNT) >> 2) < m.KQ2p;
  return ep;
}
// the h value of one element: the K-segment partials summed in segment order, all reads issued before the first add
// (q_segment_sum), then the same expression as ever; the activation in its select form (lrnde_math.hpp: the same bits)
__device__ __forceinline__ float q_epi1_value(const ModelDev& m, const float* p0, const int (&seg)[QNW], unsigned add,
                                              float w1, float b1, float ts) {
  float vals[QNW];
#pragma unroll
  for (int sgi = 0; sgi < QNW; ++sgi) vals[sgi] = p0[seg[sgi]];
  float v = vals[0];
#pragma unroll
  for (int sgi = 1; sgi < QNW; ++sgi) v = ((add >> sgi) & 1u) ? v + vals[sgi] : v;
  float pre = m.td ? fma_(w1, ts, v) : v;
  pre = pre + b1;
  return act_apply_sel(m.act, pre);
}
__device__ __forceinline__ void q_epilogue1(const ModelDev& m, const SmemQ& sm, const Epi1Q& ep, float ts) {
  const float hv = q_epi1_value(m, ep.p0, ep.seg, ep.add, ep.w1, ep.b1, ts);
  if (ep.valid) *ep.h = hv;
  if (ep.two) {  // (nothing of it is kept from the head: no shape takes this today)
    const int e = (int)threadIdx.x + QNT, o = q_epi1_row(e);
    const bool ok = e < m.RG1 * 256 && (o >> 2) < m.KQ2p;
    const int e2 = ok ? e : 0, o2 = ok ? o : 0;
    const float hv2 = q_epi1_value(m, reinterpret_cast<const float*>(sm.pl) + e2, ep.seg, ep.add, sm.bias[o2],
                                   sm.bias[m.RG1 * 64 + o2], ts);
    if (ok) reinterpret_cast<float*>(sm.hl)[q_epi1_slot(e2)] = hv2;
  }
}


__device__ __forceinline__ SmemQ carve_q(const ModelDev& m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  SmemQ s;
  s.xl = reinterpret_cast<f32x4*>(smem);
  s.hl = s.xl + (size_t)m.KQ1p * 4;
  s.pl = s.hl + (size_t)m.KQ2p * 4;
  s.bias = reinterpret_cast<float*>(s.pl + (size_t)q_nseg1(m) * m.RG1 * 64);
  s.red = reinterpret_cast<double*>(s.bias + 128 * (size_t)(m.RG1 + m.RG2));
  s.bc = reinterpret_cast<Bcast*>(s.red + QNW * 3);
  return s;
}
// first 16-byte aligned LDS address behind the forward layout, as an LDS pointer.  (Rounding the address up through
// uintptr_t loses the address space: every access through the result was a FLAT instruction, which counts in vmcnt
// and lgkmcnt at once and can only be waited for with vmcnt(0) — it drained the weight stream at every stage epilogue.)
__device__ __forceinline__ f32x4* q_extra_smem(const SmemQ& s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned off = (unsigned)(reinterpret_cast<const char*>(s.bc + 1) - smem);
  return reinterpret_cast<f32x4*>(smem + ((off + 15u) & ~15u));
}
static constexpr size_t smem_bytes_q(int KQ1p, int KQ2p, int RG1, int RG2) {
  const size_t nseg1 = (size_t)((KQ1p + QSEG - 1) / QSEG);
  return ((size_t)KQ1p * 4 + (size_t)KQ2p * 4 + nseg1 * RG1 * 64) * 16 + 128 * (size_t)(RG1 + RG2) * 4 +
         QNW * 3 * sizeof(double) + sizeof(Bcast) + 16;
}
// SKIP0 = true: wave 0 takes no part (it runs the device prologue meanwhile, k_step_q); the other waves cover everything
template <bool SKIP0 = false>
__device__ __forceinline__ void smem_init_q(const ModelDev& m, const SmemQ& s) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  constexpr int NTH = SKIP0 ? QNT - 64 : QNT;
  const int tid = SKIP0 ? (int)threadIdx.x - 64 : (int)threadIdx.x;
  if (SKIP0 && tid < 0) return;
  for (int i = tid; i < (m.KQ1p + m.KQ2p) * 4; i += NTH) s.xl[i] = z;  // xl and hl are adjacent
  const int h64 = m.RG1 * 64, d64 = m.RG2 * 64;
  for (int i = tid; i < h64; i += NTH) {
    s.bias[i] = (i < m.Hp) ? m.w1t[i] : 0.f;
    s.bias[h64 + i] = (i < m.Hp) ? m.b1[i] : 0.f;
  }
  for (int i = tid; i < d64; i += NTH) {
    s.bias[2 * h64 + i] = (i < m.Dp) ? m.w2t[i] : 0.f;
    s.bias[2 * h64 + d64 + i] = (i < m.Dp) ? m.b2[i] : 0.f;
  }
}

// ---- per-lane access to the state workspace for this tile shape ----------------------------
struct TileIOQ {
  __amdgpu_buffer_rsrc_t rs;
  int voff;  // ((b0 + s) * D + 4q) * 4, or out of range for columns beyond the batch
};
__device__ __forceinline__ TileIOQ make_tile_io_q(const StepArgs& a, int b0, int nvalid) {
  const int lane = threadIdx.x & 63, sidx = lane & 3, q = lane >> 2;
  TileIOQ io;
  io.rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.state, 0, (int)(a.n_local * 40), 0x00020000);
  io.voff = (sidx < nvalid) ? ((b0 + sidx) * a.m.D + q * 4) * 4 : 0x7ffffff0;
  return io;
}
// offset of the Dense-2 row group starting at row rb for this lane (out of range when the lane's rows are not its wave's:
// beyond D, or the 16 rows of the next wave's segment in a wave's second group)
__device__ __forceinline__ int q_voff(const TileIOQ& io, int rb, bool own) {
  return own ? io.voff + rb * 4 : 0x7ffffff0;
}
__device__ __forceinline__ f32x4 qload(const TileIOQ& io, int voff_rg, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(io.rs, voff_rg, soff, 0));
}
__device__ __forceinline__ void qstore(const TileIOQ& io, int voff_rg, int soff, const f32x4& v) {
  // literal soffset: see the store-data hazard note at sstore()
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), io.rs, voff_rg + soff, 0, 0);
}

// ---- Dense-2 epilogue policies (same contract as the 16-column ones; tile index = first row rb of the 64-row group,
// own = this lane's row quad belongs to the wave: below D, and not one of the 16 rows of the next wave's segment that a
// wave's second group covers — those lanes compute a discarded value and write nothing) ----
struct EpiStoreKQ {
  static constexpr int NPRE = 1;
  const ModelDev* m; float* kout; int b0, nvalid;
  template <class G> __device__ __forceinline__ void pre(G, int, bool, f32x4 (&)[NPRE]) const {}
  template <class G> __device__ __forceinline__ void post(G, int rb, bool own, const f32x4& kv, f32x4 (&)[NPRE]) const {
    const int lane = threadIdx.x & 63, sidx = lane & 3, q = lane >> 2;
    const int row0 = rb + q * 4;
    if (sidx < nvalid && own) *reinterpret_cast<f32x4*>(kout + (size_t)(b0 + sidx) * m->D + row0) = kv;
  }
};

// The stage operands (uprev, k1 .. k6) of a lane's two Dense-2 row groups stay in registers for the whole launch, in the
// D-fragment layout of the MFMA: element r of group G = row 112w + 64G + 4q + r of sample s.  A row's operands are written
// (post) and read (the next stages' post) by the same lane, so they never leave it; through an LDS buffer they cost 2 x S
// ds_read_b128 and 2 ds_write_b128 per lane and stage, 113 KB of LDS, and a cross-wave preload and x2 pass with a workgroup
// barrier each at the head of the launch.  The k vectors are still stored to global memory for the next launch and the
// dense record.  Lanes that are not `own` carry values that are discarded.
// Which k_step_q<SPEC, KT> keep them there: the specialised Dense-2 tail (KT < 4, MNIST-ODE's H = 100), whose last stream
// block leaves ring registers free; the generic form (KT = 4) keeps the LDS buffer (EpiStageQL / EpiFinalQL below)
__host__ __device__ constexpr bool q_regops(int KT) { return KT < 4; }
struct RegOpsQ {
  f32x4 up[2];    // uprev
  f32x4 k[6][2];  // k1 .. k6
};
// (the group index G of pre / post is a type, IC<0> or IC<1>: every register of RegOpsQ is addressed at compile time)
template <int S> struct EpiStageQ {
  static constexpr int NPRE = 1;
  TileIOQ io;
  int off_out, off_x;
  float dt;
  f32x4* xl;
  RegOpsQ* R;
  int store_k;  // Bcast::store_k: 0 = k_S stays in registers only (its global store gets an out-of-range offset and is dropped)
  template <class G> __device__ __forceinline__ void pre(G, int, bool, f32x4 (&)[NPRE]) const {}
  template <class G> __device__ __forceinline__ void post(G, int rb, bool own, const f32x4& kv, f32x4 (&)[NPRE]) const {
    constexpr int g = G::value;
    const int lane = threadIdx.x & 63, sidx = lane & 3, q = lane >> 2;
    constexpr int off = (S - 1) * S / 2;
    const int vo = q_voff(io, rb, own);
    qstore(io, store_k ? vo : 0x7ffffff0, off_out, kv);
    R->k[S - 1][g] = kv;
    f32x4 x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float o[S];
#pragma unroll
      for (int j = 0; j < S - 1; ++j) o[j] = R->k[j][g][r];
      o[S - 1] = kv[r];
      float sum = (float)Tsit5::A[off] * o[0] + (float)Tsit5::A[off + 1] * o[1];
#pragma unroll
      for (int j = 2; j < S; ++j) sum = sum + (float)Tsit5::A[off + j] * o[j];
      x[r] = R->up[g][r] + dt * sum;
    }
    if (off_x >= 0) qstore(io, vo, off_x, x);
    if (own) xl[(rb / 4 + q) * 4 + sidx] = x;  // one quad = the B operand of 4 Dense-1 k-steps, in this wave's own segment
  }
};

struct EpiFinalQ {
  static constexpr int NPRE = 2;  // u (the x tile of this, the last, f-eval: the wave's own xl rows) and g6
  TileIOQ io;
  int off_g6, off_out;
  float dt, abstol, reltol;
  int want_stiff, nvalid;
  double *aerr, *anum, *aden;
  const f32x4* xl;
  const RegOpsQ* R;  // uprev, k1..k6 as in EpiStageQ
  // dense record written by the step itself (StepArgs::dense_direct): descriptor over the slot [uprev,k1,P2,P3,P4] of this
  // attempt, voff out of range when there is none
  __amdgpu_buffer_rsrc_t rsD; int nstB; bool rec;
  // (lanes that are not `own` read another wave's x quads or, in the last group, up to 15 quads past the tile — inside the
  //  h tile behind it: the value is discarded)
  template <class G> __device__ __forceinline__ void pre(G, int rb, bool own, f32x4 (&pb)[NPRE]) const {
    pb[0] = xl[rb + (threadIdx.x & 63)];
    if (want_stiff) pb[1] = qload(io, q_voff(io, rb, own), off_g6);
  }
  template <class G> __device__ __forceinline__ void post(G, int rb, bool own, const f32x4& kv, f32x4 (&pb)[NPRE]) const {
    constexpr int g = G::value;
    const int lane = threadIdx.x & 63, sidx = lane & 3;
    const int vo = q_voff(io, rb, own);
    const f32x4 up = R->up[g];
    const f32x4 k1 = R->k[0][g], k2 = R->k[1][g], k3 = R->k[2][g], k4 = R->k[3][g], k5 = R->k[4][g], k6 = R->k[5][g];
    qstore(io, vo, off_out, kv);
    if (rec) {
      // the attempt's record slot, straight from the operands this lane already holds: uprev, k1..k6, k7 (kv) — instead
      // of a 25-MB copy through global memory in the next prologue
      // (polynomial form, lrnde_math.hpp tsit5_rec_poly: [uprev, k1, P2, P3, P4] — five stores, were eight)
      const int vd = vo;  // the slot's arrays have the state arrays' (column, row) layout
      f32x4 P2, P3, P4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float kk[6] = {k2[r], k3[r], k4[r], k5[r], k6[r], kv[r]};
        float P[3];
        tsit5_rec_poly(k1[r], kk, P);
        P2[r] = P[0]; P3[r] = P[1]; P4[r] = P[2];
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, up), rsD, vd, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, k1), rsD, vd + nstB, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, P2), rsD, vd + 2 * nstB, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, P3), rsD, vd + 3 * nstB, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, P4), rsD, vd + 4 * nstB, 0, 0);
    }
    if (sidx >= nvalid || !own) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sum = (float)Tsit5::BT[0] * k1[r] + (float)Tsit5::BT[1] * k2[r];
      sum = sum + (float)Tsit5::BT[2] * k3[r];
      sum = sum + (float)Tsit5::BT[3] * k4[r];
      sum = sum + (float)Tsit5::BT[4] * k5[r];
      sum = sum + (float)Tsit5::BT[5] * k6[r];
      sum = sum + (float)Tsit5::BT[6] * kv[r];
      const float utilde = dt * sum;
      const float sc = abstol + fmaxf_(__builtin_fabsf(up[r]), __builtin_fabsf(pb[0][r])) * reltol;
      const float rr = utilde / sc;
      const float sq = rr * rr;
      *aerr += (double)sq;
      if (want_stiff) {
        const float d1 = pb[0][r] - pb[1][r];
        const float d2 = kv[r] - k6[r];
        const float q1 = d1 * d1, q2 = d2 * d2;
        *aden += (double)q1; *anum += (double)q2;
      }
    }
  }
};

// The LDS form of the same epilogues, for the generic Dense-2 tail (KT = 4, q_regops): there the last stream block keeps
// all of its 24 ring registers to the end of the f-eval and the register form does not fit 256 VGPRs (it spilled 12).
// The stage operands (uprev, k1 .. k_{S-1}) of a workgroup's tile stay in LDS for the whole launch: kl[slot][quad*4+sample],
// slot 0 = uprev, slot j = k_j.  Slots 4.. are written and read only by the Dense-2 wave that owns the rows (the rows of its
// Dense-1 segment); the preloaded pairs are ordered by the __syncthreads() ahead of the x2 pass.  Re-reading them from
// global memory went through the same L2->L1 path as the weight stream (Dense-2 streamed at 36 B/clk against
// Dense-1's 56); the k vectors are still stored to global memory for the next launch and the dense record.
template <int S> struct EpiStageQL {
  static constexpr int NPRE = S;
  TileIOQ io;
  int off_up, off_k[6], off_out, off_x;
  float dt;
  f32x4* xl;
  f32x4* kl; int KL;
  const f32x4* klu; const f32x4* klk;  // uprev / k1 of THIS step (one of the two preloaded candidate pairs, k_step_q)
  int store_k;  // Bcast::store_k: 0 = k_S stays in LDS (its global store gets an out-of-range offset and is dropped)
  // (lanes that are not `own` read another wave's quads or, in the last group, up to 15 quads past the slot — inside the
  //  launch's slack: the value is discarded)
  template <class G> __device__ __forceinline__ void pre(G, int rb, bool, f32x4 (&pb)[NPRE]) const {
    const int li = rb + (threadIdx.x & 63);
    pb[0] = klu[li];
    if (S > 1) pb[S > 1 ? 1 : 0] = klk[li];
#pragma unroll
    for (int j = 2; j < S; ++j) pb[j] = kl[(size_t)(j + 2) * KL + li];
  }
  template <class G> __device__ __forceinline__ void post(G, int rb, bool own, const f32x4& kv, f32x4 (&pb)[NPRE]) const {
    const int lane = threadIdx.x & 63, sidx = lane & 3, q = lane >> 2;
    constexpr int off = (S - 1) * S / 2;
    const int vo = q_voff(io, rb, own);
    qstore(io, store_k ? vo : 0x7ffffff0, off_out, kv);
    if (own) kl[(size_t)(S + 2) * KL + rb + lane] = kv;
    f32x4 x;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float o[S];
#pragma unroll
      for (int j = 0; j < S - 1; ++j) o[j] = pb[1 + j][r];
      o[S - 1] = kv[r];
      float sum = (float)Tsit5::A[off] * o[0] + (float)Tsit5::A[off + 1] * o[1];
#pragma unroll
      for (int j = 2; j < S; ++j) sum = sum + (float)Tsit5::A[off + j] * o[j];
      x[r] = pb[0][r] + dt * sum;
    }
    if (off_x >= 0) qstore(io, vo, off_x, x);
    if (own) xl[(rb / 4 + q) * 4 + sidx] = x;  // one quad = the B operand of 4 Dense-1 k-steps, in this wave's own segment
  }
};

struct EpiFinalQL {
  static constexpr int NPRE = 9;
  TileIOQ io;
  int off_up, off_u, off_k[6], off_g6, off_out;
  float dt, abstol, reltol;
  int want_stiff, nvalid, D;
  double *aerr, *anum, *aden;
  const f32x4* xl; const f32x4* kl; int KL;  // u is the x tile of this (last) f-eval; uprev, k1..k6 as in EpiStageQ
  const f32x4* klu; const f32x4* klk;
  // dense record written by the step itself (StepArgs::dense_direct): descriptor over the slot [uprev,k1,P2,P3,P4] of this
  // attempt, voff out of range when there is none
  __amdgpu_buffer_rsrc_t rsD; int nstB; bool rec;
  template <class G> __device__ __forceinline__ void pre(G, int rb, bool own, f32x4 (&pb)[NPRE]) const {
    const int li = rb + (threadIdx.x & 63);
    pb[0] = klu[li];
    pb[1] = xl[li];
    pb[2] = klk[li];
#pragma unroll
    for (int j = 1; j < 6; ++j) pb[2 + j] = kl[(size_t)(3 + j) * KL + li];
    if (want_stiff) pb[8] = qload(io, q_voff(io, rb, own), off_g6);
  }
  template <class G> __device__ __forceinline__ void post(G, int rb, bool own, const f32x4& kv, f32x4 (&pb)[NPRE]) const {
    const int lane = threadIdx.x & 63, sidx = lane & 3;
    const int vo = q_voff(io, rb, own);
    qstore(io, vo, off_out, kv);
    if (rec) {
      // the attempt's record slot, straight from the operands this lane already holds: uprev (pb[0]), k1..k6 (pb[2..7]),
      // k7 (kv) — instead of a 25-MB copy through global memory in the next prologue
      // (polynomial form, lrnde_math.hpp tsit5_rec_poly: [uprev, k1, P2, P3, P4] — five stores, were eight)
      const int vd = vo;  // the slot's arrays have the state arrays' (column, row) layout
      f32x4 P2, P3, P4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float kk[6] = {pb[3][r], pb[4][r], pb[5][r], pb[6][r], pb[7][r], kv[r]};
        float P[3];
        tsit5_rec_poly(pb[2][r], kk, P);
        P2[r] = P[0]; P3[r] = P[1]; P4[r] = P[2];
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pb[0]), rsD, vd, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pb[2]), rsD, vd + nstB, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, P2), rsD, vd + 2 * nstB, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, P3), rsD, vd + 3 * nstB, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, P4), rsD, vd + 4 * nstB, 0, 0);
    }
    if (sidx >= nvalid || !own) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sum = (float)Tsit5::BT[0] * pb[2][r] + (float)Tsit5::BT[1] * pb[3][r];
      sum = sum + (float)Tsit5::BT[2] * pb[4][r];
      sum = sum + (float)Tsit5::BT[3] * pb[5][r];
      sum = sum + (float)Tsit5::BT[4] * pb[6][r];
      sum = sum + (float)Tsit5::BT[5] * pb[7][r];
      sum = sum + (float)Tsit5::BT[6] * kv[r];
      const float utilde = dt * sum;
      const float sc = abstol + fmaxf_(__builtin_fabsf(pb[0][r]), __builtin_fabsf(pb[1][r])) * reltol;
      const float rr = utilde / sc;
      const float sq = rr * rr;
      *aerr += (double)sq;
      if (want_stiff) {
        const float d1 = pb[1][r] - pb[8][r];
        const float d2 = kv[r] - pb[7][r];
        const float q1 = d1 * d1, q2 = d2 * d2;
        *aden += (double)q1; *anum += (double)q2;
      }
    }
  }
};

// W1q: [RG1][KQ1p][64][4]   element (rg,kq,l,j) = W1[row 64rg+l][k 4kq+j],  KQ1p = 28 * nseg1
// W2q: [2*nseg1][KQ2p][64][4]   KQ2p = 28; group 2w+c holds rows 112w + 64c + l (l < 48 when c = 1), zero elsewhere
// Loads for row groups beyond RG1 / 2*nseg1, and lanes whose weight row is beyond the real matrix (or another wave's),
// are outside the descriptor's range: they return 0 without touching memory.

// ===========================================================================================
// Streaming fast path (nseg1 <= QNW, RG1 <= 2, RG2 <= 2*QNW: one work item per GEMM phase per
// wave — MNIST-ODE).  A wave's weights for one f-eval are ONE fixed stream of QSB blocks
// (7 Dense-1 + 7 Dense-2) of 8 one-KiB buffer loads (4 k-quads x 2 row groups).  The blocks
// rotate through a 3-slot register ring that has two blocks in flight or, in the register form of
// k_step_q, as many quads as its issue schedule finds dead registers for (QSchedEarly): the stream is
// carried across the GEMM phases, across the barriers (raw s_barrier + lgkmcnt(0): a
// __syncthreads() would drain vmcnt) and across f-evals (the next f-eval streams the same
// addresses), so the L2 -> CU pipe does not idle at phase boundaries.  Everything is straight
// line code with compile-time slots, so hipcc emits counted vmcnt waits.
// ===========================================================================================
constexpr int QSQ = 4;            // k-quads per stream block
constexpr int QSB1 = QSEG / QSQ;  // 7 Dense-1 blocks (one canonical segment)
constexpr int QSB2 = 7;           // Dense-2 blocks (KQ2p = 28 k-quads)
constexpr int QSB = QSB1 + QSB2;
#ifndef LRNDE_QRING
#define LRNDE_QRING 3
#endif
constexpr int QRING = LRNDE_QRING;   // ring slots; QRING - 1 blocks are in flight
constexpr int QAHEAD = QRING - 1;
constexpr int VRING = 3;             // ring of the VJP kernel's stream (lrnde_backward.hpp)
// Parked stream blocks: bit B of the mask = the 8 fragments of stream block B (0..QSB-1) of every wave stay in LDS for the
// whole launch of the register form of k_step_q (q_regops), filled once at its head (q_park_fill) and read back with
// ds_read_b128 by all six f-evals, instead of six buffer loads through the CU's vector-memory address path.  The form
// has the room since its stage operands left LDS: 16 KiB per wave (two blocks) behind the forward layout.  0 = nothing
// is parked, the kernels are instruction for instruction the ones without the switch.
// Default: the last Dense-1 block (6) and the last full Dense-2 block (12), the blocks whose MFMAs the late wave of each
// SIMD waits for before the two barriers (DESIGN.md 4.1 "parked weight blocks", profiles/qpark; 0x81u, the first block
// of each phase, was measured slower with the first form of the fill).  Under the issue schedule (QSchedEarly) the blocks a
// wave waits for first behind a barrier were measured as well: {9, 10} slower in every run, {9, 12} inside the default's
// range (profiles/qsched/bench_ab.txt).
#ifndef LRNDE_QPARK
#define LRNDE_QPARK qsched::DEFAULT_PARK  // 0x1040u
#endif
constexpr unsigned QPARK = LRNDE_QPARK;
__host__ __device__ constexpr int q_popcount(unsigned v) { int n = 0; for (; v; v &= v - 1) ++n; return n; }
__host__ __device__ constexpr int q_park_nb(unsigned mask) { return q_popcount(mask & ((1u << QSB) - 1)); }
// index of parked block B among the parked blocks / the P-th parked block
__host__ __device__ constexpr int q_park_index(unsigned mask, int B) { return q_popcount(mask & ((1u << B) - 1)); }
__host__ __device__ constexpr int q_park_block(unsigned mask, int P) {
  for (int B = 0; B < QSB; ++B) if ((mask >> B) & 1u) { if (P == 0) return B; --P; }
  return -1;
}
constexpr int QPARK_FRAG = QSQ * 2;  // fragments (one-KiB wave-loads) per block
__host__ __device__ constexpr size_t q_park_bytes(unsigned mask) { return (size_t)QNW * q_park_nb(mask) * QPARK_FRAG * 1024; }
static_assert((QPARK >> QSB) == 0, "LRNDE_QPARK is a mask over the QSB stream blocks of an f-eval");
// the family's largest shape (D = 784: KQ1p = 196, KQ2p = 28, RG1 = 2, RG2 = 13) with the park region behind it
static_assert(smem_bytes_q(7 * QSEG, QSEG, 2, 13) + q_park_bytes(QPARK) <= 160 * 1024,
              "forward layout + park region exceed the 160 KiB of LDS of a CU: park fewer blocks");

// Register-parked stream block: bit B of the mask = the 8 fragments of stream block B of every wave stay in 32 VGPRs of
// the wave (StreamQ::rpark) for the whole launch of the register form of k_step_q, loaded once at its head and taken
// by the block's MFMAs as operands where they lie: no load, no LDS traffic and no copy into the ring in any f-eval.
// The registers are the ones the stream's addresses held before they moved into the loads' immediate offsets
// (q_stream_fetch_quad).  At most one block, disjoint from LRNDE_QPARK, not the (partial) last one; 0 = none, the
// kernels are the ones of the immediate-offset stream alone.  Default: block 5, just ahead of the LDS-parked last
// Dense-1 block (DESIGN.md 4.1 "Register-parked block / immediate-offset stream", profiles/rpark).
#ifndef LRNDE_QRPARK
#define LRNDE_QRPARK qsched::DEFAULT_RPARK  // 0x20u
#endif
constexpr unsigned QRPARK = LRNDE_QRPARK;
static_assert((QRPARK >> (QSB - 1)) == 0 && q_popcount(QRPARK) <= 1, "LRNDE_QRPARK names at most one of the stream blocks 0..QSB-2");
static_assert((QRPARK & QPARK) == 0, "a block is parked in LDS (LRNDE_QPARK) or in registers (LRNDE_QRPARK), not both");
__host__ __device__ constexpr bool q_parked(unsigned mask, int B) { return ((mask >> B) & 1u) != 0; }

// The issue schedule of an f-eval: which quad of which block is requested at which of its 56 points, and the slot each
// block's MFMAs read, as a compile-time table (lrnde_qsched.hpp).  QSchedLegacy<SLOT0> is the closed form every kernel of
// the family had (block B + QAHEAD into slot (SLOT0 + B + QAHEAD) % QRING at block B) and all but one still have.
// QSchedEarly<F> is f-eval F (0..5) of the register form of k_step_q: a quad is requested as soon as the registers that
// receive it are dead, the parked blocks hold no slot of their own, and the last f-eval requests nothing for a seventh.
// -DLRNDE_QSCHED=0 builds the closed form there too (so do the burst form and every ring size but three);
// -DLRNDE_QLEAD=n reads an LDS-parked quad n points (1..4) ahead of its MFMAs, -DLRNDE_QWRAP=n lets n blocks of the
// next f-eval be requested before the stage epilogue.
#ifndef LRNDE_QSCHED
#define LRNDE_QSCHED 1
#endif
#ifndef LRNDE_QLEAD
#define LRNDE_QLEAD 2
#endif
// LRNDE_QCAP and LRNDE_QWRAP are what ONE compiler's register allocation leaves (253 of 256 VGPRs, profiles/qsched/
// resource_usage.txt); tests/test_host_qstep_resources.py reads the built kernels' metadata and fails on a spill or a
// private segment: re-derive the caps then, the late f-evals first.
#ifndef LRNDE_QCAP   // busy slot quads allowed in each of the six f-evals (qsched::Params::cap)
#define LRNDE_QCAP LRNDE_QSCHED_DEFAULT_CAP
#endif
#ifndef LRNDE_QWRAP  // blocks of the next f-eval requested across a stage epilogue (qsched::Params::wrap)
#define LRNDE_QWRAP 2
#endif
static_assert(QSB == qsched::NB && QSQ == qsched::NQ && QRING <= qsched::MAXSLOT && qsched::NFEVAL == 6, "lrnde_qsched.hpp describes this stream");
static_assert(LRNDE_QLEAD >= 1 && LRNDE_QLEAD <= QSQ, "LRNDE_QLEAD is a number of points, at most one block");
#ifdef LRNDE_QBURST  // (the burst form takes its slots from the closed form's origin, qsched::Table::slot0)
constexpr bool QEARLY = false;
#else
constexpr bool QEARLY = LRNDE_QSCHED != 0 && QRING == 3;
#endif
template <int SLOT0, int KT = 4, unsigned PARK = 0, unsigned RPARK = 0> struct QSchedLegacy {
  static constexpr qsched::Table tab = qsched::legacy_table_at(qsched::Params{PARK, RPARK, KT, QRING, qsched::LEGACY, 0, 0, {}}, SLOT0);
};
template <int F, int KT, unsigned PARK, unsigned RPARK> struct QSchedEarly {
  static constexpr qsched::Params par = qsched::Params{PARK, RPARK, KT, QRING, qsched::EARLY, LRNDE_QLEAD, LRNDE_QWRAP, LRNDE_QCAP};
  static_assert(qsched::check_launch(par, qsched::EPI_INFLIGHT) == 0, "the issue schedule of these masks breaks an invariant (lrnde_qsched.hpp check_launch)");
  static constexpr qsched::Table tab = qsched::launch_table(par, F);
};
// f-eval F of a step launch (stage F + 2)
template <int F, int KT, unsigned PARK, unsigned RPARK>
using QSchedStep = std::conditional_t<QEARLY, QSchedEarly<F, KT, PARK, RPARK>, QSchedLegacy<(QSB * F) % QRING, KT, PARK, RPARK>>;

template <int I> struct IC { static constexpr int value = I; };
template <int I0, int I1, class F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I0 < I1) { f(IC<I0>{}); static_for<I0 + 1, I1>(f); }
}

struct StreamQ {
  __amdgpu_buffer_rsrc_t rs1[2], rs2[2];  // descriptors of the wave's Dense-1 / Dense-2 row groups: they begin at the group's
                             // first quad of this wave (q_stream_rsrc), so a fragment's offset is a compile-time constant
  int v1[2], v2[2];          // per-lane offsets of those row groups (or out of range)
  int kq2_real;              // ceil(H/4): Dense-2 quads at/after it are not fetched
  f32x4 ring[QRING][QSQ][2];
  f32x4 rpark[QSQ][2];       // the register-parked block (QRPARK).  Set by k_step_q only
  const f32x4* park;         // parked blocks (QPARK): this lane's quad of the wave's own fragment 0, in LDS; fragment f is
                             // 64 quads (1 KiB) further on each.  Set by k_step_q only
};

__device__ __forceinline__ void q_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Addressing of the stream.  Fragment (block B, quad J, row group c) lies (B' * QSQ + J) * 1024 bytes behind the first
// quad of its row group, B' = the block's index inside its layer, and the row group's descriptor begins at that first
// quad.  The load takes the fragment as
//   vector offset  v[c] + J * 1024    the lane's offset, the quad in the instruction's 12-bit immediate (at most 3072;
//                                     the sum is unsigned: an out-of-range 0x7ffffff0 becomes 0x800003f0 .. 0x80000bf0,
//                                     out of range as well, and does not wrap)
//   scalar offset  B' * 4096          one of six constants, the same for both layers and row groups,
// so no address lives in a register of its own.  Written as rs + v[c] + (s[c] + constant) with s[c] the wave's runtime
// offset, the 90 offsets of an f-eval were launch invariants that hipcc kept in registers: 45 SGPRs (spilled into VGPR
// lanes and read back ahead of each load) and, for Dense-2, whose select below it folded the constant into, 42 VGPRs.
//
// lane offset + quad, as an unsigned sum (0x7ffffff0 + 3072 overflows an int)
__device__ __forceinline__ int q_lane_off(int v, int quad_bytes) { return (int)((unsigned)v + (unsigned)quad_bytes); }
// descriptor of `bytes` of weights from byte `first` on (on = false: a row group or a wave that has none, every lane of
// it is out of range: any valid descriptor)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t q_stream_rsrc(const float* W, int bytes, int first, bool on) {
  const int f = on ? first : 0;
  return __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const char*>(W) + f), 0, bytes - f, 0x00020000);
}
// the two loads (row groups 0 and 1) of quad J of stream block B.
// KT = number of k-quads of the LAST Dense-2 block that exist.  launch_step instantiates two values: KT = 1 exactly when
// ceil(H/4) == 25 (kq2_real = 25: the callers emit quads 0..24 and every emitted Dense-2 load is real, which is the only
// reason the KT < 4 branch below may drop the test), and KT = 4 otherwise, the generic form: quads at or after kq2_real
// are fetched with an out-of-range offset and return 0 without touching memory.  KT = 2, 3 are never instantiated, and
// would need a launch rule of the same kind (KT = kq2_real - 24) before they could be.
template <int B, int J, int KT>
__device__ __forceinline__ void q_stream_fetch_quad(const StreamQ& st, f32x4& r0, f32x4& r1) {
#ifdef LRNDE_QABL_NOLOAD  // diagnostic ablation: no weight stream (results are meaningless)
  r0 = f32x4{0.f, 0.f, 0.f, 0.f}; r1 = f32x4{0.f, 0.f, 0.f, 0.f};
  asm volatile("" : "+v"(r0), "+v"(r1));
  return;
#endif
  // (the generic form keeps the quad in the scalar constant: the 12 sums v[c] + J * 1024, which hipcc forms once per
  //  launch where a load sits in another basic block than the first one, are VGPRs k_step_q<*, 4> does not have)
  constexpr int BL = B < QSB1 ? B : B - QSB1;
  constexpr int voff = KT < 4 ? J * 1024 : 0, soff = KT < 4 ? BL * (QSQ * 1024) : (BL * QSQ + J) * 1024;
  if constexpr (B < QSB1) {
    r0 = wload(st.rs1[0], q_lane_off(st.v1[0], voff), soff);
    r1 = wload(st.rs1[1], q_lane_off(st.v1[1], voff), soff);
  } else if constexpr (KT < 4) {
    r0 = wload(st.rs2[0], q_lane_off(st.v2[0], voff), soff);
    r1 = wload(st.rs2[1], q_lane_off(st.v2[1], voff), soff);
  } else {
    // wave-uniform; as an OR with a scalar (v2 is lane * 16 < 1024 or 0x7ffffff0 itself: the OR is 0x7ffffff0 exactly)
    const int oor = (BL * QSQ + J) < st.kq2_real ? 0 : 0x7ffffff0;
    r0 = wload(st.rs2[0], st.v2[0] | oor, soff);
    r1 = wload(st.rs2[1], st.v2[1] | oor, soff);
  }
}

// issue the 8 loads of stream block B (0..QSB-1) into ring slot SLOT
template <int B, int SLOT>
__device__ __forceinline__ void q_stream_load(StreamQ& st) {
  static_for<0, QSQ>([&](auto Jc) {
    constexpr int J = decltype(Jc)::value;
    q_stream_fetch_quad<B, J, 4>(st, st.ring[SLOT][J][0], st.ring[SLOT][J][1]);
  });
  __builtin_amdgcn_sched_barrier(0);
}

// the two loads of quad J of stream block B into ring slot SLOT: the pieces of q_stream_load, for interleaving with
// MFMAs.
// With KT < 4 the missing quads of the last Dense-2 block are neither loaded nor multiplied: an out-of-range load still
// costs its slot in the SIMD's return path (tools/oor_probe.hip), and for H = 100 (25 real quads) 3 of the 28 loads of
// every Dense-2 row group were of that kind.
// PARK = the mask of LDS-parked blocks (QPARK; 0 in every kernel but the register form of k_step_q): the two fragments
// of a parked block come from the wave's own LDS region — what q_park_fill's same two buffer loads returned, lane for
// lane — into the same ring registers at the same point of the interleave.
// RPARK = the mask of the register-parked block (QRPARK, likewise): nothing is issued for it, its MFMAs read StreamQ::rpark
template <int B, int SLOT, int J, int KT = 4, unsigned PARK = 0, unsigned RPARK = 0>
__device__ __forceinline__ void q_stream_load_quad(StreamQ& st) {
  if constexpr (q_parked(RPARK, B)) {
  } else if constexpr (q_parked(PARK, B)) {
    if constexpr (B < QSB - 1 || J < KT) {
      constexpr int f = (q_park_index(PARK, B) * QSQ + J) * 2;
      st.ring[SLOT][J][0] = st.park[f * 64];
      st.ring[SLOT][J][1] = st.park[(f + 1) * 64];
    }
  } else if constexpr (B < QSB - 1 || J < KT) {
    q_stream_fetch_quad<B, J, KT>(st, st.ring[SLOT][J][0], st.ring[SLOT][J][1]);
  }
}

__device__ __forceinline__ void stream_init_q(const ModelDev& m, StreamQ& st) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int voff = lane * 16;
  const bool has1 = wave < q_nseg1(m);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    // the wave's K-segment of W1q's row group c / its packed group 2w + c of W2q
    st.rs1[c] = q_stream_rsrc(m.W1q, m.RG1 * m.KQ1p * 1024, (c * m.KQ1p + wave * QSEG) * 1024, has1 && c < m.RG1);
    st.rs2[c] = q_stream_rsrc(m.W2q, q_w2_groups(m.KQ1p) * m.KQ2p * 1024, (2 * wave + c) * m.KQ2p * 1024, has1);
#ifdef LRNDE_X_FULLROWS  // experiment: rows H..64*RG1-1 of W1q are real (zero) memory instead of out-of-range lanes
    st.v1[c] = (has1 && c < m.RG1) ? voff : 0x7ffffff0;
#else
    st.v1[c] = (has1 && c < m.RG1 && c * 64 + lane < m.H) ? voff : 0x7ffffff0;
#endif
    // Dense-2: packed groups 2w, 2w+1 = rows 112w + 64c + lane (q_w2_row); the second group's last 16 rows are the next
    // wave's, packed as zeros and out of range here as well
    const int rb = wave * (QSEG * 4) + c * 64;
    st.v2[c] = (has1 && (c == 0 || lane < QSEG * 4 - 64) && rb + lane < m.D) ? voff : 0x7ffffff0;
  }
  st.kq2_real = (m.H + 3) / 4;
  static_for<0, QAHEAD>([&](auto Bc) { constexpr int B = decltype(Bc)::value; q_stream_load<B, B>(st); });
}

// The loads the schedule asks for are issued two at a time between the quads' MFMAs (eight MFMAs per pair of loads),
// pinned by sched_barriers: as a burst of eight ahead of the block's 32 MFMAs a wave sat in the CU's address-issue
// queue behind the other waves' bursts before it could start its MFMAs (56.5 -> 53.0 us per step).  -DLRNDE_QBURST
// builds the burst form.
// (what is requested at a point, in front of its MFMAs and behind them, is the schedule's: q_sched_issue)
template <class SCH, int PT, bool POST, int KT, unsigned PARK, unsigned RPARK>
__device__ __forceinline__ void q_sched_issue(StreamQ& st) {
  constexpr int src = POST ? SCH::tab.post[PT].src : SCH::tab.pre[PT].src;
  if constexpr (src != qsched::SRC_NONE) {
    constexpr int B = (POST ? SCH::tab.post[PT].block : SCH::tab.pre[PT].block) % QSB;
    constexpr int SLOT = POST ? SCH::tab.post[PT].slot : SCH::tab.pre[PT].slot;
    constexpr int J = POST ? SCH::tab.post[PT].quad : SCH::tab.pre[PT].quad;
    static_assert((src == qsched::SRC_LDS) == q_parked(PARK, B) && !q_parked(RPARK, B), "the schedule and q_stream_load_quad agree on the source");
    q_stream_load_quad<B, SLOT, J, KT, PARK, RPARK>(st);
  }
}
#ifndef LRNDE_QBURST
#define LRNDE_QISSUE(PT, POST) q_sched_issue<SCH, PT, POST, KT, PARK, RPARK>(st)
#define LRNDE_QPIN() __builtin_amdgcn_sched_barrier(0)
#else
#define LRNDE_QISSUE(PT, POST) do {} while (0)
#define LRNDE_QPIN() do {} while (0)
#endif
// diagnostic ablation (-DLRNDE_QABL_NOMFMA): the MFMAs of feval_qs are replaced by an empty asm that keeps their
// operands live, so the launch time is that of the weight stream, the LDS traffic and the epilogues alone
#ifdef LRNDE_QABL_NOMFMA
__device__ __forceinline__ f32x4 qmfma(float a, float b, f32x4 c) { asm volatile("" : "+v"(c) : "v"(a), "v"(b)); return c; }
#else
__device__ __forceinline__ f32x4 qmfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }
#endif
// ep1 = epilogue 1's invariants where the caller made them once for all the f-evals of its launch (k_step_q's register
// form); nullptr (a constant at every call): they are made here, behind the first barrier
// RPARK: the MFMAs of the register-parked block take StreamQ::rpark where those of the others take their ring slot
// SCH: the issue schedule (QSchedLegacy / QSchedEarly)
template <class Epi, class SCH, int KT = 4, unsigned PARK = 0, unsigned RPARK = 0>
__device__ __forceinline__ void feval_qs(const ModelDev& m, const SmemQ& sm, StreamQ& st, float ts, const Epi& epi,
                                         const Epi1Q* ep1 = nullptr) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sidx = lane & 3, q = lane >> 2;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int h64 = m.RG1 * 64, d64 = m.RG2 * 64;
  const float* w2t = sm.bias + 2 * h64; const float* b2 = w2t + d64;
  const int nseg1 = q_nseg1(m);
  f32x4 acc0 = zero4, acc1 = zero4;
  STAMP(1); STAMPW(0);
  // ---- Dense 1: stream blocks 0..6 (segment = wave, row groups 0 and 1) ----
  {
    const f32x4* xp = sm.xl + (size_t)((wave < nseg1 ? wave : 0) * QSEG) * 4 + sidx;
    // the B operands (x quads from LDS) are read one block ahead of their MFMAs: read at the top of their own block,
    // every block exposed the LDS round trip (~230 cycles x 14 blocks per f-eval)
    f32x4 bq[2][QSQ];
#pragma unroll
    for (int j = 0; j < QSQ; ++j) bq[0][j] = xp[j * 4];
    static_for<0, QSB1>([&](auto Bc) {
      constexpr int B = decltype(Bc)::value;
      constexpr int SL = q_parked(RPARK, B) ? 0 : SCH::tab.slot_of[B];
#ifdef LRNDE_QBURST
      q_stream_load<(B + QAHEAD) % QSB, (SCH::tab.slot0 + B + QAHEAD) % QRING>(st);  // (the burst form is LEGACY's)
#endif
      if constexpr (B + 1 < QSB1) {
#pragma unroll
        for (int j = 0; j < QSQ; ++j) bq[(B + 1) & 1][j] = xp[((B + 1) * QSQ + j) * 4];
      }
      const f32x4 (&b_)[QSQ] = bq[B & 1];
      const f32x4 (&w_)[QSQ][2] = q_parked(RPARK, B) ? st.rpark : st.ring[SL];
      static_for<0, QSQ>([&](auto Jc) {
        constexpr int j = decltype(Jc)::value;
        LRNDE_QISSUE(B * QSQ + j, false);
        acc0 = qmfma(w_[j][0].x, b_[j].x, acc0);
        acc1 = qmfma(w_[j][1].x, b_[j].x, acc1);
        acc0 = qmfma(w_[j][0].y, b_[j].y, acc0);
        acc1 = qmfma(w_[j][1].y, b_[j].y, acc1);
        acc0 = qmfma(w_[j][0].z, b_[j].z, acc0);
        acc1 = qmfma(w_[j][1].z, b_[j].z, acc1);
        acc0 = qmfma(w_[j][0].w, b_[j].w, acc0);
        acc1 = qmfma(w_[j][1].w, b_[j].w, acc1);
        LRNDE_QISSUE(B * QSQ + j, true);
        LRNDE_QPIN();
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    if (wave < nseg1) {
      f32x4* pp = sm.pl + ((size_t)wave * m.RG1) * 64 + lane;
      pp[0] = acc0;
      if (m.RG1 > 1) pp[64] = acc1;
    }
  }
  STAMP(2); STAMPW(1);
  q_barrier();
  STAMP(3);
  // epilogue 1 (one C-fragment element per thread, Epi1Q)
  if (ep1) q_epilogue1(m, sm, *ep1, ts);
  else q_epilogue1(m, sm, q_epi1_make(m, sm), ts);
  STAMPW(2);
  q_barrier();
  STAMP(4); STAMPW(3);
  // ---- Dense 2: stream blocks 7..13 (the rows of the wave's Dense-1 segment as two 64-row groups, q_w2_groups; one
  // chain over K = H) ----
  {
    const f32x4* hp = sm.hl + sidx;
    acc0 = zero4; acc1 = zero4;
    const int g0 = wave * (QSEG * 4), g1 = g0 + 64;  // first rows of the two groups
    const bool own0 = g0 + q * 4 < m.D, own1 = q < (QSEG * 4 - 64) / 4 && g1 + q * 4 < m.D;
    f32x4 pb0[Epi::NPRE], pb1[Epi::NPRE];
    f32x4 bq[2][QSQ];
#pragma unroll
    for (int j = 0; j < QSQ; ++j) bq[0][j] = hp[j * 4];
    static_for<0, QSB2>([&](auto Bc) {
      constexpr int B = decltype(Bc)::value;
      constexpr int SL = q_parked(RPARK, QSB1 + B) ? 0 : SCH::tab.slot_of[QSB1 + B];
#ifdef LRNDE_QBURST
      q_stream_load<(QSB1 + B + QAHEAD) % QSB, (SCH::tab.slot0 + QSB1 + B + QAHEAD) % QRING>(st);  // wraps into the next f-eval's Dense-1 blocks
#endif
      if constexpr (B == QSB2 - 3) {  // epilogue operands: issued ~3 blocks before they are needed
        if (g0 < m.D) epi.pre(IC<0>{}, g0, own0, pb0);
        if (g1 < m.D) epi.pre(IC<1>{}, g1, own1, pb1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (B + 1 < QSB2) {
#pragma unroll
        for (int j = 0; j < QSQ; ++j) bq[(B + 1) & 1][j] = hp[((B + 1) * QSQ + j) * 4];
      }
      const f32x4 (&b_)[QSQ] = bq[B & 1];
      const f32x4 (&w_)[QSQ][2] = q_parked(RPARK, QSB1 + B) ? st.rpark : st.ring[SL];
      static_for<0, QSQ>([&](auto Jc) {
        constexpr int j = decltype(Jc)::value;
        LRNDE_QISSUE((QSB1 + B) * QSQ + j, false);
        if constexpr (B < QSB2 - 1 || j < KT) {
          acc0 = qmfma(w_[j][0].x, b_[j].x, acc0);
          acc1 = qmfma(w_[j][1].x, b_[j].x, acc1);
          acc0 = qmfma(w_[j][0].y, b_[j].y, acc0);
          acc1 = qmfma(w_[j][1].y, b_[j].y, acc1);
          acc0 = qmfma(w_[j][0].z, b_[j].z, acc0);
          acc1 = qmfma(w_[j][1].z, b_[j].z, acc1);
          acc0 = qmfma(w_[j][0].w, b_[j].w, acc0);
          acc1 = qmfma(w_[j][1].w, b_[j].w, acc1);
        }
        LRNDE_QISSUE((QSB1 + B) * QSQ + j, true);
        LRNDE_QPIN();
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    auto finish = [&](int rb, bool own, const f32x4& tot) {
      const int row0 = own ? rb + q * 4 : 0;  // (other lanes' rows may lie past the bias vectors; their value is discarded)
      const f32x4 wt = *reinterpret_cast<const f32x4*>(w2t + row0);
      const f32x4 bb = *reinterpret_cast<const f32x4*>(b2 + row0);
      f32x4 kv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pre = m.td ? fma_(wt[r], ts, tot[r]) : tot[r];
        kv[r] = pre + bb[r];
      }
      return kv;
    };
    if (g0 < m.D) epi.post(IC<0>{}, g0, own0, finish(g0, own0, acc0), pb0);
    if (g1 < m.D) epi.post(IC<1>{}, g1, own1, finish(g1, own1, acc1), pb1);
  }
  STAMP(5); STAMPW(4);
  // No workgroup barrier here: the x quads a wave has just written are its own Dense-1 segment, read next by the same
  // wave, and a wavefront's LDS accesses are performed in program order — only the compiler must not move the next
  // f-eval's reads above these stores.  Every other LDS region keeps its order through the two barriers inside the
  // f-eval: h and the Dense-1 partials are rewritten only after every wave has passed the next barrier, i.e. after
  // every wave's reads of them; the stage operands are in the lanes' registers (RegOpsQ).
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  STAMP(6);
}

template <class F>
__device__ __forceinline__ void q_tile_foreach(const ModelDev& m, int b0, int nvalid, int KQ1, F&& fn) {
  // quads of the tile: sample fastest (4), then k-quad: 256 B contiguous per sample per wave
  for (int i = threadIdx.x; i < KQ1 * 4; i += QNT) {
    const int sidx = i & 3, kq = i >> 2;
    fn(kq, sidx, sidx < nvalid, (size_t)(b0 + sidx) * m.D + kq * 4);
  }
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }

// `three` (workgroup-uniform) = false: b and c are known to be zero everywhere (no stiffness sums wanted) and their
// shuffle reductions — 12 dependent ds_bpermute round trips each — are skipped; the sums are the same zeros
__device__ __forceinline__ void block_sum3_q(double* red, double& a, double& b, double& c, bool three = true) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  a = wave_sum_dpp(a);
  if (three) { b = wave_sum_dpp(b); c = wave_sum_dpp(c); }
  if (lane == 0) { red[wave * 3 + 0] = a; red[wave * 3 + 1] = b; red[wave * 3 + 2] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0.0, sb = 0.0, sc = 0.0;
    for (int w = 0; w < QNW; ++w) { sa += red[w * 3]; sb += red[w * 3 + 1]; sc += red[w * 3 + 2]; }
    a = sa; b = sb; c = sc;
  }
  // (no second barrier: `red` is not written again in this launch, and the callers only use thread 0's totals)
}

__device__ __forceinline__ void q_feval_store(const ModelDev& m, const SmemQ& sm, StreamQ& fc, float ts,
                                              float* kout, int b0, int nvalid) {
  EpiStoreKQ e;
  e.m = &m; e.kout = kout; e.b0 = b0; e.nvalid = nvalid;
  feval_qs<EpiStoreKQ, QSchedLegacy<0>>(m, sm, fc, ts, e);
  __syncthreads();  // full barrier: the k stores are read back through other lanes by the caller
}

__global__ __launch_bounds__(QNT) void k_rhs_q(StepArgs a, const float* u, float t, float* du) {
  STAMP(0);
  const SmemQ s = carve_q(a.m);
  smem_init_q(a.m, s);
  StreamQ fc;
  stream_init_q(a.m, fc);
  const int b0 = blockIdx.x * QNB, nvalid = min(QNB, a.B - b0);
  const int KQ1 = a.m.D / 4;
  __syncthreads();
  q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int kq, int sidx, bool valid, size_t g) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    s.xl[kq * 4 + sidx] = valid ? ld4(u + g) : z;
  });
  __syncthreads();
  q_feval_store(a.m, s, fc, t, du, b0, nvalid);
}

__global__ __launch_bounds__(QNT) void k_init1_q(StepArgs a) {
  const SmemQ s = carve_q(a.m);
  smem_init_q(a.m, s);
  StreamQ fc;
  stream_init_q(a.m, fc);
  const int b0 = blockIdx.x * QNB, nvalid = min(QNB, a.B - b0);
  const int KQ1 = a.m.D / 4;
  int cur0; float tinit;
  if (a.init_fresh) {  // first launch of a solve: the control blocks are written here (StepArgs::init_fresh)
    cur0 = 0; tinit = a.t0;
    if (blockIdx.x == 0 && threadIdx.x == 0) solve_init_body(a.ctrl, a.t0, a.init_nsaved, a.init_si);
  } else {
    const Ctrl c = a.ctrl[0];
    cur0 = c.cur; tinit = c.t;
  }
  const float* u0 = a.init_u0 ? a.init_u0 : ubuf_at(a, cur0);
  float* ucopy = a.init_u0 ? ubuf_at(a, cur0) : nullptr;
  float* f0 = kfsal_at(a, cur0);
  __syncthreads();
  q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int kq, int sidx, bool valid, size_t g) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 v = valid ? ld4(u0 + g) : z;
    s.xl[kq * 4 + sidx] = v;
    if (valid && ucopy) st4(ucopy + g, v);
  });
  __syncthreads();
  q_feval_store(a.m, s, fc, tinit, f0, b0, nvalid);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int, int, bool valid, size_t g) {
    if (!valid) return;
    const f32x4 u = ld4(u0 + g), f = ld4(f0 + g);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float sk = a.abstol + __builtin_fabsf(u[h]) * a.reltol;
      const float r0 = u[h] / sk, r1 = f[h] / sk;
      const float q0 = r0 * r0, q1 = r1 * r1;
      a0 += (double)q0; a1 += (double)q1;
    }
  });
  block_sum3_q(s.red, a0, a1, a2);
  publish_partial(a, 2, a0, a1, 0.0);
}

__global__ __launch_bounds__(QNT) void k_init2_q(StepArgs a) {
  const SmemQ s = carve_q(a.m);
  smem_init_q(a.m, s);
  StreamQ fc;
  stream_init_q(a.m, fc);
  const int b0 = blockIdx.x * QNB, nvalid = min(QNB, a.B - b0);
  const int KQ1 = a.m.D / 4;
  const Ctrl c = a.ctrl[0];
  if (threadIdx.x < 64) {
    double s1[3];
    reduce_partials(a.pinit_recv, a.nwg_global, s1);
    if (threadIdx.x == 0) s.bc->dt0 = init_dt0(s1, a.n_global, a.t1 - a.t0);
  }
  __syncthreads();
  const float dt0 = s.bc->dt0;
  const float* u0 = ubuf_at(a, c.cur);
  const float* f0 = kfsal_at(a, c.cur);
  float* f1 = a.ks[0];
  q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int kq, int sidx, bool valid, size_t g) {
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
      const f32x4 u = ld4(u0 + g), f = ld4(f0 + g);
#pragma unroll
      for (int h = 0; h < 4; ++h) x[h] = u[h] + dt0 * f[h];
    }
    s.xl[kq * 4 + sidx] = x;
  });
  __syncthreads();
  q_feval_store(a.m, s, fc, c.t + dt0, f1, b0, nvalid);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int, int, bool valid, size_t g) {
    if (!valid) return;
    const f32x4 u = ld4(u0 + g), f = ld4(f0 + g), ff = ld4(f1 + g);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float sk = a.abstol + __builtin_fabsf(u[h]) * a.reltol;
      const float r2 = (ff[h] - f[h]) / sk;
      const float q2 = r2 * r2;
      a0 += (double)q2;
    }
  });
  block_sum3_q(s.red, a0, a1, a2);
  publish_partial(a, 3, a0, 0.0, 0.0);
}

// stream_init_q's per-lane offset (or out of range) and scalar byte offset of the first quad of row group c of the Dense-1
// and Dense-2 streams, for any wave: the park fill (q_park_fill) issues other waves' loads.  (Its own function and not
// a part of stream_init_q: hipcc compiled the shared form of it to other code in every kernel of the family, and the
// kernels without a park stay instruction for instruction what they were.)
struct QRowOff { int v1, s1, v2, s2; };
// ... through descriptors of the whole matrices (the stream's own begin at the issuing wave's rows, StreamQ)
struct QParkSrc { __amdgpu_buffer_rsrc_t rs1, rs2; int kq2_real; };
__device__ __forceinline__ QRowOff q_row_off(const ModelDev& m, int wave, int lane, int c) {
  const int voff = lane * 16;
  const bool has1 = wave < q_nseg1(m);
  QRowOff r;
#ifdef LRNDE_X_FULLROWS
  r.v1 = (has1 && c < m.RG1) ? voff : 0x7ffffff0;
#else
  r.v1 = (has1 && c < m.RG1 && c * 64 + lane < m.H) ? voff : 0x7ffffff0;
#endif
  r.s1 = (c * m.KQ1p + (has1 ? wave * QSEG : 0)) * 1024;
  const int rb = wave * (QSEG * 4) + c * 64;
  r.v2 = (has1 && (c == 0 || lane < QSEG * 4 - 64) && rb + lane < m.D) ? voff : 0x7ffffff0;
  r.s2 = (has1 ? 2 * wave + c : 0) * m.KQ2p * 1024;
  return r;
}

// The fill of the park region, by waves 1..6 at the head of k_step_q (wave 0 runs the controller prologue and gets nothing
// added).  Fragment (P * QSQ + J) * 2 + c of a wave — quad J, row group c of its P-th parked block — lies at
// park[(wave * NF + fragment) * 64 + lane].  A filling wave parks its own fragments with the very loads of its stream
// (q_stream_load_quad into the ring slot that is still free at the head) and, per block, one or two of wave 0's eight
// with wave 0's offsets (q_row_off): an out-of-range lane parks the zero the stream load returns.  Ten loads are in
// flight per block; the addresses of the own fragments cost nothing, which matters: a first form that gave every load a
// runtime (wave, fragment) spent 60 scalar instructions per load and 10 k cycles in the head.  The __syncthreads() at
// the end of the head orders the writes before any parked read.
//
// fragment e (= quad e / 2, row group e % 2) of stream block B of wave 0, whose row offsets are ra (group 0), rb (group 1)
template <int B>
__device__ __forceinline__ f32x4 q_park_load0(const QParkSrc& st, const QRowOff& ra, const QRowOff& rb, int e, bool on) {
  const int J = e >> 1;
  const bool c1 = (e & 1) != 0;
  if constexpr (B < QSB1) {
    return wload(st.rs1, on ? (c1 ? rb.v1 : ra.v1) : 0x7ffffff0, (c1 ? rb.s1 : ra.s1) + (B * QSQ + J) * 1024);
  } else {
    const int kq = (B - QSB1) * QSQ + J;
    return wload(st.rs2, on && kq < st.kq2_real ? (c1 ? rb.v2 : ra.v2) : 0x7ffffff0, (c1 ? rb.s2 : ra.s2) + kq * 1024);
  }
}
template <unsigned PARK, int KT, int P>
__device__ __forceinline__ void q_park_fill_block(StreamQ& st, const QParkSrc& src, const QRowOff& ra, const QRowOff& rb, int fw,
                                                  f32x4* own, f32x4* w0) {
  if constexpr (P < q_park_nb(PARK)) {
    constexpr int B = q_park_block(PARK, P), FREE = QRING - 1;
    // wave 0's fragment e of this block: e = fw for every wave, and e = 6, 7 for two waves that rotate with P
    const int e2 = QNW - 1 + fw - 2 * (P % 3);
    const bool on2 = e2 >= QNW - 1 && e2 < QPARK_FRAG;
    static_for<0, QSQ>([&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      if constexpr (B < QSB - 1 || J < KT) q_stream_fetch_quad<B, J, KT>(st, st.ring[FREE][J][0], st.ring[FREE][J][1]);
    });
    const f32x4 va = q_park_load0<B>(src, ra, rb, fw, true), vb = q_park_load0<B>(src, ra, rb, on2 ? e2 : 0, on2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int J = 0; J < QSQ; ++J) {
      if (B < QSB - 1 || J < KT) {  // (the quads the stream itself never loads stay unwritten and unread)
        own[((P * QSQ + J) * 2) * 64] = st.ring[FREE][J][0];
        own[((P * QSQ + J) * 2 + 1) * 64] = st.ring[FREE][J][1];
      }
    }
    w0[(P * QPARK_FRAG + fw) * 64] = va;
    if (on2) w0[(P * QPARK_FRAG + e2) * 64] = vb;
    __builtin_amdgcn_sched_barrier(0);
    q_park_fill_block<PARK, KT, P + 1>(st, src, ra, rb, fw, own, w0);
  }
}
template <unsigned PARK, int KT>
__device__ __forceinline__ void q_park_fill(const ModelDev& m, StreamQ& st, f32x4* park) {
  constexpr int NF = q_park_nb(PARK) * QPARK_FRAG;
  const int lane = threadIdx.x & 63;
  const int fw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) - 1;  // 0..5
  const QRowOff ra = q_row_off(m, 0, lane, 0), rb = q_row_off(m, 0, lane, 1);
  QParkSrc src;
  src.rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)m.W1q, 0, m.RG1 * m.KQ1p * 1024, 0x00020000);
  src.rs2 = __builtin_amdgcn_make_buffer_rsrc((void*)m.W2q, 0, q_w2_groups(m.KQ1p) * m.KQ2p * 1024, 0x00020000);
  src.kq2_real = st.kq2_real;
  q_park_fill_block<PARK, KT, 0>(st, src, ra, rb, fw, park + (size_t)(fw + 1) * (NF * 64) + lane, park + lane);
}

// the eight loads of the register-parked block, at the head of k_step_q: the stream's own loads of that block, into
// StreamQ::rpark.  An out-of-range lane (or a wave without rows) keeps the zeros the stream would have fed its MFMAs.
template <unsigned RPARK, int KT>
__device__ __forceinline__ void q_rpark_load(StreamQ& st) {
  if constexpr (RPARK != 0) {
    constexpr int B = q_park_block(RPARK, 0);
    static_for<0, QSQ>([&](auto Jc) {
      constexpr int J = decltype(Jc)::value;
      q_stream_fetch_quad<B, J, KT>(st, st.rpark[J][0], st.rpark[J][1]);
    });
  }
}

// one attempted Tsit5 step, 4 columns per workgroup (same flow as k_step's fused path)
template <bool SPEC, int KT> __global__ __launch_bounds__(QNT) void k_step_q(StepArgs a, int j) {
  STAMP(9);
  const SmemQ s = carve_q(a.m);
  StreamQ fc;
  stream_init_q(a.m, fc);   // the first two weight blocks are requested before anything waits
  const int b0 = blockIdx.x * QNB, nvalid = min(QNB, a.B - b0);
  const int KQ1 = a.m.D / 4;
  STAMP(10);
  // wave 0 runs the device prologue (a chain of dependent global loads: control block, partial sums) while the other
  // six waves clear the LDS tiles and stage the bias vectors: the two used to run one after the other
  // ... and every wave loads BOTH candidate pairs (ubuf[p], kfsal[p]), p = 0, 1, of its own Dense-2 rows into registers:
  // which pair is (uprev, k1) is what the prologue is deciding, and its round trip to memory plus the controller
  // arithmetic is time in which the tile would otherwise sit unread (then one more round trip, after the decision, at
  // the head of the step).  Columns past the batch and lanes that are not `own` load from an out-of-range offset: zeros.
  const TileIOQ io = make_tile_io_q(a, b0, nvalid);
  const int qlane = (threadIdx.x & 63) >> 2;
  const int g0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * (QSEG * 4), g1 = g0 + 64;  // as in feval_qs
  const bool own0 = g0 + qlane * 4 < a.m.D, own1 = qlane < (QSEG * 4 - 64) / 4 && g1 + qlane * 4 < a.m.D;
  const int vo0 = q_voff(io, g0, own0), vo1 = q_voff(io, g1, own1);
  RegOpsQ R;
#ifndef LRNDE_NO_PRELOAD  // (diagnostic builds: the pair is read after the decision)
  f32x4 cu[2][2], ck[2][2];  // [parity][row group]
  auto preload = [&]() {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      cu[p][0] = qload(io, vo0, arr_off(a, p)); cu[p][1] = qload(io, vo1, arr_off(a, p));
      ck[p][0] = qload(io, vo0, arr_off(a, 2 + p)); ck[p][1] = qload(io, vo1, arr_off(a, 2 + p));
    }
  };
#else
  auto preload = [&]() {};
#endif
  constexpr bool REGS = q_regops(KT);
  f32x4* kl = REGS ? nullptr : q_extra_smem(s);  // LDS form: [9][KL]: 0,1 = pair 0; 2,3 = pair 1; 4..8 = k2..k6
  const int KL = a.m.KQ1p * 4;
  constexpr bool PARKED = REGS && QPARK != 0;
  constexpr unsigned RPARK = REGS ? QRPARK : 0u;
  if constexpr (PARKED) {  // the wave's own 16 KiB of the park region, behind the forward layout
    constexpr int NF = q_park_nb(QPARK) * QPARK_FRAG;
    fc.park = q_extra_smem(s) + (size_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * (NF * 64) + (threadIdx.x & 63);
  }
  if (threadIdx.x < 64) {
    if constexpr (REGS) { preload(); q_rpark_load<RPARK, KT>(fc); }  // in flight while the wave decides
    step_prologue(a, j, s.bc);
  } else {
    // (LDS init first: the prologue's own loads are already on their way when these 48 (LDS form: 72) wave-loads reach
    //  the CU's address path, which takes them one every ~16 cycles)
    smem_init_q<true>(a.m, s);
    if constexpr (REGS) {
      preload();
      q_rpark_load<RPARK, KT>(fc);
      if constexpr (PARKED) q_park_fill<QPARK, KT>(a.m, fc, q_extra_smem(s));
    } else {  // LDS form: the six waves load both pairs of the whole tile into kl, ordered by the barrier below
#ifndef LRNDE_NO_PRELOAD
    constexpr int NTH = QNT - 64;
    const int tid = (int)threadIdx.x - 64;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 v[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {  // KQ1 * 4 <= 784 quads (shape limit of this kernel) = at most three per thread
      const int i = tid + r * NTH;
      const int sidx = i & 3, kq = i >> 2;
      const bool ok = i < KQ1 * 4 && sidx < nvalid;
      const size_t g = ok ? (size_t)(b0 + sidx) * a.m.D + kq * 4 : 0;
      v[r][0] = ld4(a.ubuf[0] + g); v[r][1] = ld4(a.kfsal[0] + g);
      v[r][2] = ld4(a.ubuf[1] + g); v[r][3] = ld4(a.kfsal[1] + g);
      if (!ok) { v[r][0] = z; v[r][1] = z; v[r][2] = z; v[r][3] = z; }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int i = tid + r * NTH;
      if (i < KQ1 * 4) { kl[i] = v[r][0]; kl[KL + i] = v[r][1]; kl[2 * KL + i] = v[r][2]; kl[3 * KL + i] = v[r][3]; }
    }
#endif
    }
  }
  __syncthreads();  // Bcast is written, the LDS tiles are clear, the biases staged (register form: the only barrier of the head)
  STAMP(11);
  const Bcast bc = *s.bc;

  if (bc.accepted_prev) {  // savevalues! of the step accepted by the prologue
    const float* up = ubuf_at(a, bc.cur_prev);
    const float* un = ubuf_at(a, bc.cur_prev ^ 1);
    const float* k1 = kfsal_at(a, bc.cur_prev);
    const float* k7 = kfsal_at(a, bc.cur_prev ^ 1);
    int slot = bc.nsaved0;
    for (int is = bc.isave0; is < bc.isave1; ++is, ++slot) {
      const float ts = a.saveat[is];
      float* dst = a.u_saved + (size_t)slot * a.B * a.m.D;
      float* dst2 = slot == a.also_slot ? a.also_dst : nullptr;
      if (ts != bc.t_new) {
        const float theta = (ts - bc.tprev) / bc.dt_prev;
        float bw[7];
        tsit5_bweights(theta, bw);
        q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int, int, bool valid, size_t g) {
          if (!valid) return;
          const f32x4 y0 = ld4(up + g), v1 = ld4(k1 + g), v2 = ld4(a.ks[0] + g), v3 = ld4(a.ks[1] + g),
                      v4 = ld4(a.ks[2] + g), v5 = ld4(a.ks[3] + g), v6 = ld4(a.ks[4] + g), v7 = ld4(k7 + g);
          f32x4 o;
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            float sum = v1[h] * bw[0] + v2[h] * bw[1];
            sum = sum + v3[h] * bw[2];
            sum = sum + v4[h] * bw[3];
            sum = sum + v5[h] * bw[4];
            sum = sum + v6[h] * bw[5];
            sum = sum + v7[h] * bw[6];
            o[h] = y0[h] + bc.dt_prev * sum;
          }
          st4(dst + g, o);
          if (dst2) st4(dst2 + g, o);
        });
      } else {
        q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int, int, bool valid, size_t g) {
          if (!valid) return;
          const f32x4 o = ld4(un + g);
          st4(dst + g, o);
          if (dst2) st4(dst2 + g, o);
        });
      }
      if (blockIdx.x == 0 && threadIdx.x == 0) a.t_saved[slot] = ts;
    }
    if (a.save_everystep) {
      float* dst = a.u_saved + (size_t)slot * a.B * a.m.D;
      q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int, int, bool valid, size_t g) {
        if (valid) st4(dst + g, ld4(un + g));
      });
      if (blockIdx.x == 0 && threadIdx.x == 0) a.t_saved[slot] = bc.t_new;
    }
    if (bc.dense_idx >= 0) {  // dense record of the accepted step for the adjoint
      const size_t nst = (size_t)a.n_local;
      float* dd = a.dense + (size_t)bc.dense_idx * REC_ARRAYS * nst;
      const float* src[8] = {up, k1, a.ks[0], a.ks[1], a.ks[2], a.ks[3], a.ks[4], k7};
      if (!a.dense_direct)  // (direct mode: the step wrote this slot itself at its end, EpiFinalQ)
      q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int, int, bool valid, size_t g) {
        if (!valid) return;
        f32x4 v[8], P2, P3, P4;
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) v[qq] = ld4(src[qq] + g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float kk[6] = {v[2][r], v[3][r], v[4][r], v[5][r], v[6][r], v[7][r]};
          float P[3];
          tsit5_rec_poly(v[1][r], kk, P);
          P2[r] = P[0]; P3[r] = P[1]; P4[r] = P[2];
        }
        st4(dd + g, v[0]); st4(dd + nst + g, v[1]); st4(dd + 2 * nst + g, P2); st4(dd + 3 * nst + g, P3); st4(dd + 4 * nst + g, P4);
      });
      if (blockIdx.x == 0 && threadIdx.x == 0) { a.dense_t[bc.dense_idx] = bc.tprev; a.dense_dt[bc.dense_idx] = bc.dt_prev; }
    }
  }
  if (!bc.do_step) return;

  // register form: epilogue 1's invariants once for the six f-evals (the bias vectors are staged: the head's barrier).
  // The LDS form makes them in each f-eval (feval_qs): it has no registers to keep them in
  const Epi1Q ep1v = REGS ? q_epi1_make(a.m, s) : Epi1Q{};
  const Epi1Q* ep1 = REGS ? &ep1v : nullptr;
  const float t = bc.t, dt = bc.dt;
  const float c1 = (float)Tsit5::C[0], c2 = (float)Tsit5::C[1], c3 = (float)Tsit5::C[2],
              c4 = (float)Tsit5::C[3];
  double aerr = 0.0, anum = 0.0, aden = 0.0;
  const int o_un = arr_off(a, bc.cur ^ 1), o_k7 = arr_off(a, 2 + (bc.cur ^ 1));
  const int o_g6 = arr_off(a, 9);
  const int o_up = arr_off(a, bc.cur), o_k1 = arr_off(a, 2 + bc.cur);
  const f32x4* klu = nullptr; const f32x4* klk = nullptr;
  if constexpr (REGS) {
#ifndef LRNDE_NO_PRELOAD
    {  // the pair the prologue chose (bc.cur is workgroup-uniform); the other one is dropped
      const bool odd = bc.cur != 0;
      R.up[0] = odd ? cu[1][0] : cu[0][0]; R.up[1] = odd ? cu[1][1] : cu[0][1];
      R.k[0][0] = odd ? ck[1][0] : ck[0][0]; R.k[0][1] = odd ? ck[1][1] : ck[0][1];
    }
#else
    R.up[0] = qload(io, vo0, o_up); R.up[1] = qload(io, vo1, o_up);
    R.k[0][0] = qload(io, vo0, o_k1); R.k[0][1] = qload(io, vo1, o_k1);
#endif
    {  // x2 = uprev + (dt*a21)*k1   (src/perform_step.jl:11-12): each lane forms the quads of its own rows and writes them
       // to its wave's own segment of the x tile, which only this wave reads (Dense-1 of stage 2) — no workgroup barrier,
       // the wavefront-scope fence keeps the compiler from moving those reads above the stores (see the end of feval_qs)
      const float a21dt = dt * (float)Tsit5::A[0];
      const int sidx = threadIdx.x & 3;
      f32x4 x0, x1;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        x0[h] = R.up[0][h] + a21dt * R.k[0][0][h];
        x1[h] = R.up[1][h] + a21dt * R.k[0][1][h];
      }
      if (own0) s.xl[(g0 / 4 + qlane) * 4 + sidx] = x0;  // (zeros in the columns past the batch)
      if (own1) s.xl[(g1 / 4 + qlane) * 4 + sidx] = x1;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  } else {  // LDS form: a cross-wave pass over the tile between two workgroup barriers
    klu = kl + (bc.cur ? 2 : 0) * KL;  // the pair the prologue chose
    klk = kl + (bc.cur ? 3 : 1) * KL;
    __syncthreads();  // smem_init_q is complete before the x tile is written
    {  // x2 = uprev + (dt*a21)*k1   (src/perform_step.jl:11-12)
      const float a21dt = dt * (float)Tsit5::A[0];
      q_tile_foreach(a.m, b0, nvalid, KQ1, [&](int kq, int sidx, bool valid, size_t g) {
#ifdef LRNDE_NO_PRELOAD
        {
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          const_cast<f32x4*>(klu)[kq * 4 + sidx] = valid ? ld4(ubuf_at(a, bc.cur) + g) : z;
          const_cast<f32x4*>(klk)[kq * 4 + sidx] = valid ? ld4(kfsal_at(a, bc.cur) + g) : z;
        }
#endif
        const f32x4 u = klu[kq * 4 + sidx], f = klk[kq * 4 + sidx];  // (zeros in the columns past the batch)
        f32x4 x;
#pragma unroll
        for (int h = 0; h < 4; ++h) x[h] = u[h] + a21dt * f[h];
        s.xl[kq * 4 + sidx] = x;
      });
    }
    __syncthreads();
  }
  STAMP(12);
#define LRNDE_QSTAGE(S, TS)                                                             \
  do {                                                                                  \
    const int off_out = arr_off(a, 4 + (S - 2));                                        \
    const int off_x = (S == 6) ? o_un : ((S == 5 && a.want_stiff) ? o_g6 : -1);         \
    if constexpr (REGS) {                                                               \
      EpiStageQ<S> e;                                                                   \
      e.io = io; e.off_out = off_out; e.off_x = off_x;                                  \
      e.dt = dt; e.xl = s.xl; e.R = &R; e.store_k = bc.store_k;                         \
      feval_qs<EpiStageQ<S>, QSchedStep<S - 2, KT, QPARK, RPARK>, KT, QPARK, RPARK>(a.m, s, fc, (TS), e, ep1); \
    } else {                                                                            \
      EpiStageQL<S> e;                                                                  \
      e.io = io; e.off_up = o_up; e.off_k[0] = o_k1;                                    \
      _Pragma("unroll") for (int qq = 0; qq < 5; ++qq) e.off_k[1 + qq] = arr_off(a, 4 + qq); \
      e.off_out = off_out; e.off_x = off_x;                                             \
      e.dt = dt; e.xl = s.xl; e.kl = kl; e.KL = KL; e.klu = klu; e.klk = klk; e.store_k = bc.store_k; \
      feval_qs<EpiStageQL<S>, QSchedLegacy<(QSB * (S - 2)) % QRING, KT>, KT>(a.m, s, fc, (TS), e); \
    }                                                                                   \
    STAMP(11 + S);                                                                      \
  } while (0)
  LRNDE_QSTAGE(2, t + c1 * dt);
  LRNDE_QSTAGE(3, t + c2 * dt);
  LRNDE_QSTAGE(4, t + c3 * dt);
  LRNDE_QSTAGE(5, t + c4 * dt);
  LRNDE_QSTAGE(6, t + dt);
#undef LRNDE_QSTAGE
  const bool rec = a.dense != nullptr && a.dense_direct && bc.dense_slot >= 0;
  const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.dense + (size_t)(rec ? bc.dense_slot : 0) * REC_ARRAYS * (size_t)a.n_local), 0, (int)(a.n_local * 4 * REC_ARRAYS), 0x00020000);
  if constexpr (REGS) {
    EpiFinalQ ef;
    ef.io = io; ef.off_g6 = o_g6; ef.off_out = o_k7;
    ef.dt = dt; ef.abstol = a.abstol; ef.reltol = a.reltol; ef.want_stiff = a.want_stiff; ef.nvalid = nvalid;
    ef.aerr = &aerr; ef.anum = &anum; ef.aden = &aden;
    ef.xl = s.xl; ef.R = &R;
    ef.rec = rec; ef.nstB = (int)(a.n_local * 4); ef.rsD = rsD;
    feval_qs<EpiFinalQ, QSchedStep<5, KT, QPARK, RPARK>, KT, QPARK, RPARK>(a.m, s, fc, t + dt, ef, ep1);
  } else {
    EpiFinalQL ef;
    ef.io = io; ef.off_up = o_up; ef.off_u = o_un; ef.off_k[0] = o_k1;
#pragma unroll
    for (int qq = 0; qq < 5; ++qq) ef.off_k[1 + qq] = arr_off(a, 4 + qq);
    ef.off_g6 = o_g6; ef.off_out = o_k7;
    ef.dt = dt; ef.abstol = a.abstol; ef.reltol = a.reltol; ef.want_stiff = a.want_stiff; ef.nvalid = nvalid;
    ef.D = a.m.D;
    ef.aerr = &aerr; ef.anum = &anum; ef.aden = &aden;
    ef.xl = s.xl; ef.kl = kl; ef.KL = KL; ef.klu = klu; ef.klk = klk;
    ef.rec = rec; ef.nstB = (int)(a.n_local * 4); ef.rsD = rsD;
    feval_qs<EpiFinalQL, QSchedLegacy<(QSB * 5) % QRING, KT>, KT>(a.m, s, fc, t + dt, ef);
  }
  STAMP(18);
  block_sum3_q(s.red, aerr, anum, aden, a.want_stiff != 0);
  STAMP(19);
  publish_partial(a, (j + 1) & 1, aerr, anum, aden);
}

// smem_init_q in parts for kernels that have other work to put between them: the bias / time-column loads are issued at
// the head of the kernel (a round trip to memory), the tiles are cleared at once, and the values are written to LDS only
// where the kernel first has to wait anyway (they are not read before the first epilogue).  Shape limits of the 4-column family: RG1*64 <= QNT, RG2*64 <= 2*QNT.
struct BiasPreQ { float w1, b1, w2[2], b2[2]; };
__device__ __forceinline__ BiasPreQ bias_issue_q(const ModelDev& m) {
  BiasPreQ p;
  const int t = (int)threadIdx.x;
  p.w1 = (t < m.Hp) ? m.w1t[t] : 0.f;
  p.b1 = (t < m.Hp) ? m.b1[t] : 0.f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = t + r * QNT;
    p.w2[r] = (i < m.Dp) ? m.w2t[i] : 0.f;
    p.b2[r] = (i < m.Dp) ? m.b2[i] : 0.f;
  }
  return p;
}
__device__ __forceinline__ void smem_zero_q(const ModelDev& m, const SmemQ& s) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int i = (int)threadIdx.x; i < (m.KQ1p + m.KQ2p) * 4; i += QNT) s.xl[i] = z;  // xl and hl are adjacent
}
__device__ __forceinline__ void bias_write_q(const ModelDev& m, const SmemQ& s, const BiasPreQ& p) {
  const int t = (int)threadIdx.x;
  const int h64 = m.RG1 * 64, d64 = m.RG2 * 64;
  if (t < h64) { s.bias[t] = p.w1; s.bias[h64 + t] = p.b1; }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = t + r * QNT;
    if (i < d64) { s.bias[2 * h64 + i] = p.w2[r]; s.bias[2 * h64 + d64 + i] = p.b2[r]; }
  }
}

// flat Lux parameter vector -> quad-tile A layouts (zero padded in k; W1q row groups NOT padded; W2q in the groups of
// q_w2_groups, G2 = 2 * nseg1 of them)
__global__ void k_pack_q(const float* p, int D, int H, int td, int KQ1p, int KQ2p, int RG1, int G2,
                         float* W1q, float* W2q) {
  const size_t n1 = (size_t)RG1 * KQ1p * 256, n2 = (size_t)G2 * KQ2p * 256;
  const size_t base2 = (size_t)H * (D + td) + H;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n1 + n2; i += (size_t)gridDim.x * blockDim.x) {
    if (i < n1) {
      const int jj = i & 3, l = (i >> 2) & 63;
      const size_t blk = i >> 8;
      const int kq = blk % KQ1p, rg = blk / KQ1p;
      const int o = rg * 64 + l, k = kq * 4 + jj;
      W1q[i] = (o < H && k < D) ? p[(size_t)o + (size_t)H * k] : 0.f;
    } else {
      const size_t e = i - n1;
      const int jj = e & 3, l = (e >> 2) & 63;
      const size_t blk = e >> 8;
      const int kq = blk % KQ2p, g = blk / KQ2p;
      const int c = g & 1, o = (g >> 1) * (QSEG * 4) + c * 64 + l, k = kq * 4 + jj;
      const bool mine = c == 0 || l < QSEG * 4 - 64;  // the second group's last 16 rows belong to the next wave
      W2q[e] = (mine && o < D && k < H) ? p[base2 + (size_t)o + (size_t)D * k] : 0.f;
    }
  }
}
