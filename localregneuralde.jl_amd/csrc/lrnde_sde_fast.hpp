// lrnde_sde_fast.hpp — the seam between the library and the one-launch SDE step kernels: for every NeuralDSDE whose drift is
// Chain(Dense(D => H, act), Dense(H => D)) without a time input and whose diffusion is Dense(D => D)
// (src/layers/neural_sde.jl:50-72; experiments/src/construct.jl:204-205 is D = 32, H = 64) with D <= 64 and H <= 128, one
// attempted step is ONE launch.  Each kernel family is a translation unit of its own, compiled beside lrnde_kernels.hip:
//   lrnde_sde_eh_fast.hip    k_sde_eh_fast   (Lamba Euler-Heun; also the persistent whole-solve form)
//   lrnde_sde_mil_fast.hip   k_sde_mil_fast  (Milstein)
//   lrnde_sde_sri_fast.hip   k_sde_sri_fast  (four-stage SRI)
// on the workgroup frame of lrnde_sde_frame.hpp.  The library reaches them through the four launch functions below and the one
// argument struct, nothing else; the types are in namespace lrnde because a function whose parameter type is local to one
// translation unit cannot be declared in another.
#pragma once
#include <hip/hip_runtime.h>

#include "lrnde.h"
#include "lrnde_stepctl.hpp"
#include "lrnde_dev.hpp"
#include "lrnde_sde_tree.hpp"

namespace lrnde {

constexpr int SF_NT = 256;
constexpr int SF_MAXD = 64, SF_MAXH = 128;

struct SdeFastArgs {
  const f32x4* W1p; int KG1;         // drift Dense-1 fragments [MT1p][KG1][64]
  const f32x4* W2p; int KG2p;        // drift Dense-2 fragments [MT2][KG2p][64]
  const f32x4* Wgp; int KGgp;        // diffusion (second layer of the identity+Dense form) [MT2][KGgp][64]
  const float *b1, *b2, *bg;         // zero-padded to the tile sizes
  int act, D;
  const float* u; const float* dW; float* un;   // (B, D)
  int B;
  float dt, abstol, reltol, delta;
  const float* dt_dev;   // non-NULL: the single step's dt is read from here (a dt an earlier launch on the stream computed)
  float* dW_scaled;      // non-NULL: `dW` holds standard-normal draws z; the step uses sqrt(dt) * z and leaves it here (k_sde_scale's expression)
  // sde_determine_initdt on this kernel's tiles (idt_phase 1 / 2, lrnde_sde_node.hpp: sde_init_dt_dev): per-workgroup fp64
  // sums of the norms into idt_part (phase 1: d0, d1) / idt_part2 (phase 2: d2); phase 2 leaves {dt0, d1} in idt_scal
  int idt_phase; double* idt_part; double* idt_part2; float* idt_scal; float idt_dtmax;
  // fixed-grid solve as ONE launch (lrnde_sde_solve_fixed): march_n > 0 — the workgroup takes its columns through march_n steps,
  // step i with the increments dW + i * B * D, end state to un + i * B * D, and leaves its partial sum of step i in
  // march_part[(i * gridDim.x + workgroup) * PSTRIDE]: no step waits for another workgroup (nothing consumes EEst inside
  // the solve; k_sde_march_records forms every step's record afterwards, in the partial-vector order)
  int march_n; double* march_part;
  int dbg_stall;   // test hook (LRNDE_SDE_PERSIST_STALL): the persistent form waits for one workgroup more than there are — its barrier times out
  double* part;      // per-workgroup fp64 sums of the squared residual (PSTRIDE doubles each)
  int* arrive;       // fixed-grid solve: arrival counter of the step's footer, or NULL
  Ctrl* rec;         //   ... and the record slot the last workgroup fills (EEst, EEst*dt)
  double n_norm;     // elements of the norm (B * D)
  // adaptive solves: the controller lives on the device.  The launch reads the control block (grid position i, step
  // length m in grid intervals, which of the two state buffers is current), forms dW from the caller's path itself, and
  // its last workgroup runs the PI controller and writes the block for the next launch.
  SdeCtl* ctl; const float* Wpath; float* ua; float* ub; int nfine; float t0, h;
  float gamma, qmin, qmax, beta1, beta2; int maxiters;
  lrnde_trace_row* trace; int cap_trace;
  unsigned long long* prog;  // pinned host word: sde_report_pack(launches whose footer ran, status)
  int jlaunch;
  // the layer's recorded forward: end state of accepted step k -> rec_u[k] (slot = accepted steps so far; a rejected
  // attempt's slot is rewritten by the retry), its (i, m) -> rec_im[k]
  float* rec_u; int2* rec_im; int rec_cap;
  // persistent form (k_sde_eh_fast<DT, HT, true>, cooperative launch): the base of the TWO blocks of {partial sum, tag} slots the
  // steps alternate between (zero at launch: no slot carries a step's tag yet)
  double* part2;
  // the four-stage SRI step (k_sde_sri_fast, lrnde_sde_sri_fast.hip): the second Brownian path on W's grid and the caller's
  // tableau, by value (last: the other kernels' argument offsets are what they were)
  const float* Zpath; lrnde_sri_tableau tab;
  // the path source of the TREE instantiations (lrnde_sde_tree.hpp): W (and SRI's Z) by descent instead of Wpath / Zpath, the
  // accepted step's increments recorded beside rec_u.  Behind everything else: no other field moves
  SdeTree tree;
};

// the gate of the one-launch kernels
inline bool sde_fast_shape(int D, int H) { return D >= 1 && D <= SF_MAXD && H >= 1 && H <= SF_MAXH; }

// One launch of nwg workgroups of the shape's instantiation (f.tree.on picks the TREE one) on st; nothing is launched for a
// shape outside the gate.  Defined beside their kernels — a cooperative launch takes the kernel's address; hidden: the
// library's exports are its C ABI.  sde_persist_launch: the whole adaptive solve in one launch, returns the launch's hipError_t.
__attribute__((visibility("hidden"))) void sde_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f);
__attribute__((visibility("hidden"))) hipError_t sde_persist_launch(int D, int H, int nwg, hipStream_t st, SdeFastArgs& f, bool coop);
__attribute__((visibility("hidden"))) void sde_mil_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f);
__attribute__((visibility("hidden"))) void sde_sri_fast_launch(int D, int H, int nwg, hipStream_t st, const SdeFastArgs& f);

}  // namespace lrnde
