/*
 * lrnde.h — C ABI of liblrnde: the MI355X (gfx950) implementation of the
 * LocalRegNeuralDE.jl adaptive Tsit5 neural-ODE path.
 *
 * The reference has no FFI seam of its own (it is pure Julia); the seam this
 * library replaces is the Julia-level one listed in SURVEY.md §8(b).  Each
 * entry point names the reference interface it stands in for (paths relative
 * to the reference repository).  A Julia maintainer binds these with `ccall`
 * (see INTEGRATION.md); this repo's host mirror binds them with ctypes.
 *
 * Conventions
 *   - opaque handle, one per (device, stream); not thread-safe; distinct
 *     handles are independent;
 *   - every array pointer is a DEVICE pointer (hipMalloc'd / torch.cuda) unless
 *     the name ends in _host; the caller owns all buffers;
 *   - states are fp32, column-major (D x B) "batch last" exactly as the Julia
 *     arrays are laid out, i.e. sample-major contiguous rows of D floats;
 *   - parameters are the flat Lux/ComponentArray vector
 *     [vec(W1) (H x (D+td)); b1 (H); vec(W2) (D x (H+td)); b2 (D)];
 *   - every call returns an lrnde_status (0 = ok) and never throws; the text of
 *     the last error is available from lrnde_last_error();
 *   - calls are stream-ordered on the handle's HIP stream; calls that return
 *     host-side results (stats, scalars) synchronise that stream.
 */
#ifndef LRNDE_H
#define LRNDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrnde_ctx lrnde_ctx;

typedef enum {
  LRNDE_OK = 0,
  LRNDE_MAXITERS = 1,          /* ReturnCode.MaxIters  (iter > maxiters)            */
  LRNDE_DT_LESS_THAN_MIN = 2,  /* ReturnCode.DtLessThanMin                          */
  LRNDE_DT_NAN = 3,            /* ReturnCode.DtNaN / Unstable (NaN reached the norm) */
  LRNDE_BADARG = 4,            /* ArgumentError (src/utils.jl:53-58 and shape checks) */
  LRNDE_CAPACITY = 5,          /* caller's save buffer too small                     */
  LRNDE_HIP_ERROR = 6,
  LRNDE_NCCL_ERROR = 7,
  LRNDE_UNSUPPORTED = 8
} lrnde_status;

enum { LRNDE_ACT_IDENTITY = 0, LRNDE_ACT_TANH = 1, LRNDE_ACT_GELU = 2 };
enum { LRNDE_REG_ERROR_ESTIMATE = 0, LRNDE_REG_STIFFNESS_ESTIMATE = 1 };
enum { LRNDE_MODE_NONE = 0, LRNDE_MODE_UNBIASED = 1, LRNDE_MODE_BIASED = 2 };

/* Vector field description.  Replaces the Lux model captured by the `dudt`
 * closure, src/layers/neural_ode.jl:45-48, for the field the MNIST experiment
 * builds: TDChain(Dense(D+td => H, act), Dense(H+td => D)),
 * experiments/src/construct.jl:180-189 and src/layers/common.jl:10-40. */
typedef struct {
  int32_t state_dim;   /* D: rows of the state per sample (784 for MNIST)        */
  int32_t hidden_dim;  /* H (100)                                               */
  int32_t time_dep;    /* 1: TDChain appends t as the last input row of each Dense */
  int32_t act;         /* LRNDE_ACT_* applied after the first Dense              */
} lrnde_model_desc;

/* Solver options.  Replaces the kwargs NeuralODE forwards to `solve`,
 * src/layers/neural_ode.jl:10-13,51 and experiments/src/construct.jl:192-197. */
typedef struct {
  float abstol, reltol;
  int32_t maxiters;
  int32_t save_start;      /* Julia kwarg save_start (experiments pass false)     */
  int32_t save_everystep;  /* saveat == [] (the :biased mode)                     */
  int32_t exact_pow;       /* 0: DiffEqBase fastpow in the PI controller; 1: pow  */
} lrnde_solve_opts;

/* sol.destats / retcode / the last attempted step (src/utils.jl:7-9). */
typedef struct {
  int32_t retcode;  /* lrnde_status of the solve itself */
  int32_t nf, naccept, nreject, iters;
  int32_t nsaved;
  float t_final, dt_final, eest_last, dt_init;
} lrnde_stats;

typedef struct { /* one row per attempted step (diagnostics / parity tests) */
  float t, dt, eest;
  int32_t accepted;
} lrnde_trace_row;

/* lifecycle.  `stream` is a hipStream_t (NULL = the null stream). */
int lrnde_create(lrnde_ctx** out, const lrnde_model_desc* desc, int device, void* stream);
int lrnde_destroy(lrnde_ctx* ctx);
const char* lrnde_last_error(const lrnde_ctx* ctx);
size_t lrnde_param_count(const lrnde_model_desc* desc);
const char* lrnde_version(void);

/* Small Dense-chain vector field: any `Chain` / `TDChain` of `Dense` layers, optionally led by an input activation
 * `Base.Fix1(broadcast, act)` / `WrappedFunction` (the PhysioNet latent ODE's gen_dynamics,
 * experiments/src/construct.jl:236-244: Chain(tanh.(u), Dense(20=>40, tanh), Dense(40=>20, tanh), ...)).
 *   nlayers    1..LRNDE_CHAIN_MAX_LAYERS Dense layers;
 *   time_dep   1: TDChain, t is appended as the last input row of EVERY Dense;
 *   input_act  LRNDE_ACT_* applied to u before the first Dense (identity: none);
 *   dims       the state widths, dims[0] == dims[nlayers] == D, every entry <= LRNDE_CHAIN_MAX_WIDTH
 *              (the input of a TDChain layer is dims[l] + 1);
 *   act        LRNDE_ACT_* after each Dense (the output layer may have one too).
 * Parameters: the flat Lux ComponentArray in layer order, per layer vec(W) (out x (in+td), column-major, the t column
 * last) followed by b.  The input activation has none.
 * Limits (checked by lrnde_create_chain, LRNDE_UNSUPPORTED with a message from lrnde_last_error(NULL)): the widths above
 * and the forward weight image, sum over layers of (in + td + 1) * (out rounded up to even) fp32 (rounded up to a
 * multiple of 4), at most LRNDE_CHAIN_MAX_WEIGHT_BYTES: the step kernel keeps it in LDS for the whole launch.
 * lrnde_chain_param_count applies no limits (0 for a malformed desc).
 * A chain handle is accepted by lrnde_set_params, lrnde_rhs, lrnde_init_dt, lrnde_perform_step, lrnde_solve,
 * lrnde_node_forward, lrnde_vjp, lrnde_step_reg_grad, lrnde_node_forward_record(_ts), lrnde_node_backward_recorded(_ts),
 * lrnde_node_backward, lrnde_record_generation and lrnde_destroy.  It is refused with LRNDE_UNSUPPORTED by the
 * communicator entry points (lrnde_comm_init, lrnde_comm_init_local: chain handles are one rank) and by the hooks
 * lrnde_set_overlap, lrnde_bench_step and lrnde_bench_exchange.  lrnde_set_solver accepts VCAB3 / VCABM3 (see there). */
#define LRNDE_CHAIN_MAX_LAYERS 16
#define LRNDE_CHAIN_MAX_WIDTH 128
#define LRNDE_CHAIN_MAX_WEIGHT_BYTES (128 * 1024)
typedef struct {
  int32_t nlayers;
  int32_t time_dep;
  int32_t input_act;
  int32_t dims[LRNDE_CHAIN_MAX_LAYERS + 1];
  int32_t act[LRNDE_CHAIN_MAX_LAYERS];
} lrnde_chain_desc;   /* 144 bytes */
int lrnde_create_chain(lrnde_ctx** out, const lrnde_chain_desc* desc, int device, void* stream);
size_t lrnde_chain_param_count(const lrnde_chain_desc* desc);

/* Wide Dense-chain vector field: the same descriptor and parameter layout as the small chain, for chains it refuses —
 * every width in 1..LRNDE_WIDE_CHAIN_MAX_WIDTH, any weight size (the MNIST field with mlp_num_hidden_layers > 1,
 * experiments/src/construct.jl:183-189: TDChain(Dense(785=>100,tanh), Dense(101=>100,tanh), Dense(101=>784))).  The
 * weights are streamed from L2 as MFMA operands, 16 batch columns per workgroup; every dot product is
 * the canonical one of the MLP handle (fp32 fma chains over 112-row segments, partials added left to right), so a
 * two-layer chain gives the MLP handle's lrnde_rhs bits and a chain of widths <= 112 the small chain handle's.
 * Checked here (LRNDE_BADARG / LRNDE_UNSUPPORTED with a message from lrnde_last_error(NULL)): nlayers in
 * 1..LRNDE_CHAIN_MAX_LAYERS, dims[0] == dims[nlayers], every width in 1..LRNDE_WIDE_CHAIN_MAX_WIDTH, activations
 * LRNDE_ACT_*; a chain whose parameter vector plus one workgroup's activation record exceed 256 MiB is refused (the
 * VJP's scratch is bounded by that figure: larger batches run as several launches).
 * A wide-chain handle is accepted by every entry point listed above for a chain handle, and by
 * lrnde_node_forward_record_ce and lrnde_classifier_ce; it is refused with LRNDE_UNSUPPORTED by the same calls that refuse
 * a chain handle (communicator entry points, lrnde_set_overlap, lrnde_bench_step, lrnde_bench_exchange) and by
 * lrnde_set_solver with VCAB3 / VCABM3 (Tsit5 only).  Its continuous adjoint runs the host-controlled loop by default and, after
 * lrnde_set_adjoint_loop(ctx, LRNDE_ADJ_LOOP_DEVICE), the device-controlled loop of two launches per attempted step. */
#define LRNDE_WIDE_CHAIN_MAX_WIDTH 1024
int lrnde_create_wide_chain(lrnde_ctx** out, const lrnde_chain_desc* desc, int device, void* stream);

/* Which loop runs the reversed solve of lrnde_node_backward_recorded(_ts) / lrnde_node_backward on this handle.
 * LRNDE_ADJ_LOOP_AUTO (the default): every handle's own routing; a wide-chain handle takes the host-controlled loop.
 * LRNDE_ADJ_LOOP_DEVICE: a wide-chain handle takes its device-controlled loop (same bits as the host loop); a backward
 * call whose batch is outside that loop's gate (LDS, workgroups, 256 MiB of stage records) returns LRNDE_UNSUPPORTED with
 * a message naming the limit and leaves the handle and its forward record usable.  On a handle whose AUTO routing already
 * is a device loop it is accepted and changes nothing.  The diagnostic switch LRNDE_ADJ_HOST=1 still forces the host loop.
 * LRNDE_ADJ_LOOP_DISCRETE: a wide-chain handle takes the discrete adjoint of its recorded Tsit5 solve: what the comment
 * of lrnde_set_sensealg below states for LRNDE_SENSE_DISCRETE, computed for the wide handle by two launches per recorded
 * step, newest first, all enqueued up front with no host wait (csrc/lrnde_wide_discrete.hpp: the kernels and their fixed
 * order of summation; two calls give the same bits).  lrnde_stats of the backward: naccept = iters = the record's steps,
 * nreject = 0, nf = 6 * steps + 1; the adjoint-info hook (lrnde_hooks.h) reports kind 5 and no host wait.  A backward call whose batch is
 * outside the gate (160 KiB of LDS, 4096 tiles of 16 columns, 256 MiB of stage records and sweep vectors) returns
 * LRNDE_UNSUPPORTED with a message naming the limit, touches nothing and leaves the record usable; it never runs the other
 * method instead, and LRNDE_ADJ_HOST=1 does not override it.  On a handle that is not an unsharded wide-chain handle the
 * setter returns LRNDE_UNSUPPORTED (a small Dense-chain handle selects its discrete adjoint with lrnde_set_sensealg, which
 * in turn stays closed for the wide handle) and the handle stays usable.  Any other code: LRNDE_BADARG. */
enum { LRNDE_ADJ_LOOP_AUTO = 0, LRNDE_ADJ_LOOP_DEVICE = 1 };
enum { LRNDE_ADJ_LOOP_DISCRETE = 2 };
int lrnde_set_adjoint_loop(lrnde_ctx* ctx, int32_t loop);

/* The `sensealg` field of NeuralODE (src/layers/neural_ode.jl:1-23): the method of lrnde_node_backward_recorded(_ts) and
 * lrnde_node_backward on this handle.
 * LRNDE_SENSE_INTERPOLATING (the default): the continuous adjoint, the InterpolatingAdjoint restatement described below.
 * LRNDE_SENSE_DISCRETE: the discrete adjoint of the recorded Tsit5 solve, what a tape (TrackerAdjoint / ReverseDiffAdjoint)
 * gives upstream — UPSTREAM-RECALL (frozen grid): DiffEqBase's norm of tracked arrays works on values, so a tape does not
 * differentiate the step-size controller.  loss = <cotangents, saved states> + w_reg * reg_val; the gradient is the exact
 * derivative of the discrete forward map over the accepted steps of the record, their times and step sizes constants.
 * Rejected attempts do not appear; the first-same-as-last derivative is differentiated (k1 of step n+1 is k7 of step n); a
 * state saved inside a step is that step's Tsit5 interpolant, whose cotangent flows into the step's uprev and k1..k7 with the
 * weights dt * b_i(theta), theta = (ts - t_n) / dt_n in fp32 as the forward forms it; a state saved at a step's end is a
 * copy of u; sol(t1) of the local step stays a constant and the regulariser's gradient is unchanged.  One launch walks
 * the record (csrc/lrnde_chain_discrete.hpp: the sweep, its fixed order of summation, its gate); two calls give the same
 * bits.  lrnde_stats of the backward: naccept = iters = the record's steps, nreject = 0, nf = 6 * steps + 1.
 * Returns LRNDE_BADARG for any other code and LRNDE_UNSUPPORTED for DISCRETE on a handle that is not an unsharded small
 * Dense-chain handle (lrnde_create_chain); the handle stays usable after either.  A backward call whose batch is outside
 * the sweep's gate (160 KiB of LDS, 4096 workgroups, 256 MiB of parameter partials) returns LRNDE_UNSUPPORTED with a
 * message naming the limit, touches nothing and leaves the record usable; it never runs the other method instead. */
enum { LRNDE_SENSE_INTERPOLATING = 0, LRNDE_SENSE_DISCRETE = 1 };
int lrnde_set_sensealg(lrnde_ctx* ctx, int32_t sensealg);

/* Hands the flat parameter vector `ps` (what ODEProblem(dudt, x, tspan, ps)
 * carries, src/layers/neural_ode.jl:50) to the library; repacked on device
 * into the MFMA operand layout.  Call again whenever ps changes. */
int lrnde_set_params(lrnde_ctx* ctx, const float* p, size_t n);

/* The `solver` field of NeuralODE (src/layers/neural_ode.jl:4,51: `solve(prob, n.solver; ...)`) for the choices the
 * experiments offer (experiments/src/construct.jl:154-164 `_ode_solver`): 0 = Tsit5 (default), 1 = VCAB3, 2 = VCABM3.
 * It selects the method of the layer's GLOBAL solve in lrnde_solve / lrnde_node_forward* / lrnde_node_backward*; the
 * local regularisation step stays Tsit5, as in the reference (neural_ode.jl:75,93 build that integrator with Tsit5()).
 * VCAB3 / VCABM3: restated from the published algorithm, UPSTREAM-RECALL (csrc/lrnde_adams.hpp says what is recalled);
 * the backward pass of a recorded Adams forward interpolates its Hermite record and integrates the adjoint with Tsit5.
 * Which handles, which loop: the MLP handle runs the host-driven loop of csrc/lrnde_adams.hpp (3-4 launches and a read-back
 * per attempted step); an unsharded small Dense-chain handle runs one launch per attempted step with the controller on the
 * device (csrc/lrnde_chain_adams.hpp, k_adams_chain; same bits as the host loop, which the diagnostic switch
 * LRNDE_ADAMS_HOST=1 selects there too).  A wide Dense-chain handle refuses alg != 0 with LRNDE_UNSUPPORTED (Tsit5 only).
 * The conv handle has a setter of its own, lrnde_conv_set_solver (host-driven loop with fused 16-byte elementwise kernels,
 * csrc/lrnde_conv_adams.hpp).
 * The small chain's discrete adjoint walks a Tsit5 stage record: alg != 0 on a handle whose lrnde_set_sensealg choice is
 * DISCRETE returns LRNDE_UNSUPPORTED, and so does lrnde_set_sensealg(DISCRETE) on a handle whose solver is not Tsit5 —
 * whichever is set second is refused, with a message, and the handle stays usable.  Any other code: LRNDE_BADARG. */
enum { LRNDE_ALG_TSIT5 = 0, LRNDE_ALG_VCAB3 = 1, LRNDE_ALG_VCABM3 = 2 };
int lrnde_set_solver(lrnde_ctx* ctx, int32_t alg);

/* du = dudt(u, p, t)  — src/layers/neural_ode.jl:45-48, src/layers/common.jl:10-40. */
int lrnde_rhs(lrnde_ctx* ctx, const float* u, float t, int32_t B, float* du);

/* `init(prob, Tsit5(); ...)` as used by _get_ode_integrator,
 * src/layers/neural_ode.jl:33-38: the automatic initial dt (2 f-evals) and
 * fsalfirst = f(u0, t0).  dt_host receives integrator.dt. */
int lrnde_init_dt(lrnde_ctx* ctx, const float* u0, int32_t B, float t0, float tend, float abstol,
                  float reltol, float* k1, float* dt_host);

/* `_perform_step(integrator, cache::Tsit5ConstantCache, p, Val(reg_type))`,
 * src/perform_step.jl:3-47.  Reads uprev, k1 (= integrator.fsalfirst), t, dt;
 * writes u and k7 (= integrator.fsallast); returns EEst and both regularisation
 * values on the host (reg_error = EEst*dt, :34-38; reg_stiff, :40-47).  The
 * reference's tuple (u, reg_val, 6 + sol.destats.nf, dt), :31, is these plus two
 * constants of the call: the step costs 6 f-evals and does not change dt
 * (julia/LRNDEBackend.jl `_perform_step`; lrnde_node_forward adds the 6 + 3 itself). */
int lrnde_perform_step(lrnde_ctx* ctx, const float* uprev, const float* k1, int32_t B, float t,
                       float dt, float abstol, float reltol, float* u, float* k7,
                       float* eest_host, float* reg_error_host, float* reg_stiff_host);

/* `solve(ODEProblem(dudt, x, tspan, ps), Tsit5(); maxiters, saveat, reltol,
 * abstol, save_start)`, src/layers/neural_ode.jl:50-51.  saveat_host: nsave
 * ascending times (may be NULL/0 with save_everystep).  u_saved: device buffer
 * of cap_saved states; t_saved_host: cap_saved floats (sol.t).  trace_host may be
 * NULL. */
int lrnde_solve(lrnde_ctx* ctx, const float* u0, int32_t B, float t0, float t1,
                const lrnde_solve_opts* opts, const float* saveat_host, int32_t nsave,
                float* u_saved, float* t_saved_host, int32_t cap_saved, lrnde_stats* stats_host,
                lrnde_trace_row* trace_host, int32_t cap_trace);

/* `(n::NeuralODE{regularize, regularize_type})(x, ps, st)`,
 * src/layers/neural_ode.jl:56-100: solve on (t0,t2), pick t1 (mode unbiased:
 * t1_or_rand is t1 itself, drawn by the host RNG as :71; mode biased: a uniform
 * [0,1) draw used as an index into sol.t[1:end-1], :92), fresh init at
 * (sol(t1), t1), one local _perform_step, nfe = sol.destats.nf + 6 + 3.
 * u_end receives sol.u[end] (diffeqsol_to_array, src/utils.jl:37). */
int lrnde_node_forward(lrnde_ctx* ctx, const float* x, int32_t B, float t0, float t2,
                       const lrnde_solve_opts* opts, int32_t mode, int32_t reg_type,
                       float t1_or_rand, float* u_end, float* reg_val_host, int32_t* nfe_host,
                       lrnde_stats* stats_host, float* t1_used_host);

/* Batch sharding across GPUs (one process per GPU).  Not in the reference
 * (SURVEY.md §2 rows 16-17): each rank owns B columns of a global batch of
 * nranks*B; the only exchange is one RCCL all-reduce of the per-tile fp64
 * partial sums of the error norm per attempted step (plus two at init).
 * Backward pass on a sharded handle: the parameter cotangent (gp of lrnde_vjp,
 * dp of lrnde_node_backward*) is all-reduced over the ranks — it is a sum over
 * all samples — and comes out replicated; dx stays sharded; the adjoint's error
 * norm runs over [lambda of all ranks; mu once].
 * unique_id: the 128 bytes of an ncclUniqueId made by lrnde_comm_unique_id on
 * rank 0 and broadcast by the host (torch.distributed). */
int lrnde_comm_unique_id(void* unique_id_128_host);
int lrnde_comm_init(lrnde_ctx* ctx, const void* unique_id_128_host, int32_t rank, int32_t nranks);
int lrnde_comm_destroy(lrnde_ctx* ctx);
/* The size of the communicator the handle actually holds (ncclCommCount; 1 for an unsharded handle) and, optionally, its
 * kind (0 none, 1 RCCL, 2 the in-process local communicator of lrnde_hooks.h): what a launcher checks against the number
 * of ranks it asked for. */
int lrnde_comm_count(lrnde_ctx* ctx, int32_t* nranks_host, int32_t* kind_host);

/* ---- SDE: `_perform_step(integrator, cache::LambaEulerHeunConstantCache, p)`,
 * src/perform_step.jl:172-206 (residual :214-216), as called by NeuralDSDE,
 * src/layers/neural_sde.jl:98,118.  drift: Chain(Dense(D=>H,act), Dense(H=>D)); diffusion:
 * Dense(D=>D) (experiments/src/construct.jl:204-205), diagonal noise; parameters are the two
 * halves of the ComponentArray (p.drift, p.diffusion = [vec(Wg); bg]).  dW (= W.dW) is supplied by
 * the caller, delta is integrator.opts.delta.  Returns u, EEst and the regularisation value
 * EEst*dt on the host.  3 drift + 3 diffusion evaluations per call. */
typedef struct lrnde_sde lrnde_sde;
int lrnde_sde_create(lrnde_sde** out, const lrnde_model_desc* drift, int32_t diffusion_bias, int device,
                     void* stream);
int lrnde_sde_destroy(lrnde_sde* sde);
const char* lrnde_sde_last_error(const lrnde_sde* sde);
int lrnde_sde_set_params(lrnde_sde* sde, const float* p_drift, size_t n_drift, const float* p_diffusion,
                         size_t n_diffusion);
int lrnde_sde_euler_heun_step(lrnde_sde* sde, const float* uprev, const float* dW, int32_t B, float t,
                              float dt, float abstol, float reltol, float delta, float* u,
                              float* eest_host, float* reg_val_host);

/* The same in two halves, for a training step that needs sol.u[end] before it can form du_end
 * (experiments/src/utils.jl:104-115: Zygote.pullback forward, then back(...)): the forward keeps the dense
 * record, the backward consumes it (one backward per record). */
int lrnde_node_forward_record(lrnde_ctx* ctx, const float* x, int32_t B, float t0, float t2,
                              const lrnde_solve_opts* opts, int32_t mode, int32_t reg_type, float t1_or_rand,
                              float* u_end, float* reg_val_host, int32_t* nfe_host, lrnde_stats* stats_host,
                              float* t1_used_host);
int lrnde_node_backward_recorded(lrnde_ctx* ctx, int32_t B, const float* du_end, float w_reg, float* dx, float* dp,
                                 lrnde_stats* stats_bwd_host);

/* The recorded forward with the layer's `saveat` kwarg, and its pullback for cotangents on EVERY state of the returned
 * solution — what the reference's time-series consumers differentiate (diffeqsol_to_timeseries, src/utils.jl:42-46;
 * experiments/src/construct.jl:244-249).  saveat_host: nsave ascending times (nsave = 0: the default of
 * src/layers/neural_ode.jl:102-116).  Mode unbiased appends t1 for the solve and drops every saved time equal to t1 from
 * the result again (_CorrectedDESolution, src/utils.jl:25-33); mode biased draws t1 among the saved times but the last.
 * u_series (device, cap_series x B x D) / t_series_host receive sol.u / sol.t as the caller of the layer sees them,
 * *nseries_host their count.  lrnde_node_backward_recorded_ts: du_series (device, nseries x B x D), one cotangent per
 * state of that series; each enters the reversed-time adjoint solve as an impulse on lambda at its time (SciMLSensitivity's
 * callbacks at the saved times, with the first-same-as-last derivative re-evaluated after each), the one at the end time is
 * lambda's start value. */
int lrnde_node_forward_record_ts(lrnde_ctx* ctx, const float* x, int32_t B, float t0, float t2, const lrnde_solve_opts* opts,
                                 int32_t mode, int32_t reg_type, float t1_or_rand, const float* saveat_host, int32_t nsave,
                                 float* u_series, float* t_series_host, int32_t cap_series, int32_t* nseries_host,
                                 float* reg_val_host, int32_t* nfe_host, lrnde_stats* stats_host, float* t1_used_host);
int lrnde_node_backward_recorded_ts(lrnde_ctx* ctx, int32_t B, const float* du_series, int32_t nseries, float w_reg,
                                    float* dx, float* dp, lrnde_stats* stats_bwd_host);

/* Classifier head + loss of the MNIST experiments: logits = Dense(D => K)(u) with flat Lux
 * parameters pc = [vec(W) (K x D, column-major); b] (experiments/src/construct.jl:199), loss =
 * logitcrossentropy(logits, onehot(labels)) = mean over the batch (experiments/src/utils.jl:88).  Returns the
 * loss on the host and, where the pointers are non-NULL, logits (B,K), du = d loss / d u (B,D) and
 * dpc = d loss / d pc (device).  labels: device int32 (B), 0-based.  D is the handle's state_dim. */
int lrnde_classifier_ce(lrnde_ctx* ctx, const float* u, int32_t B, const float* pc, int32_t K, const int32_t* labels,
                        float* loss_host, float* logits, float* du, float* dpc);

/* The forward half of the reference's training step in one call (experiments/src/utils.jl:104-115: model forward + loss inside
 * one timed pullback): lrnde_node_forward_record followed by lrnde_classifier_ce on its sol.u[end], same arguments and
 * results as the two calls, same bits.  The head's launches are enqueued when the solve's last report is in, ahead of the
 * solve's final synchronisation, so the call ends with ONE synchronisation and no host round trip between the layer and
 * the head (the two calls: two synchronisations and ~60 us of idle GPU between them). */
int lrnde_node_forward_record_ce(lrnde_ctx* ctx, const float* x, int32_t B, float t0, float t2, const lrnde_solve_opts* opts,
                                 int32_t mode, int32_t reg_type, float t1_or_rand, float* u_end, float* reg_val_host,
                                 int32_t* nfe_host, lrnde_stats* stats_host, float* t1_used_host, const float* pc, int32_t K,
                                 const int32_t* labels, float* loss_host, float* logits, float* du, float* dpc);

/* ---- conv vector field (experiments/src/construct.jl:213-218) ----
 * node_core = TDChain(Chain(Conv3x3(C+1=>Hc, no bias), BatchNorm(Hc, act)),
 *                     Chain(Conv3x3(Hc+1=>Hc), BatchNorm(Hc, act)), Conv3x3(Hc+1=>C))
 * on a (W x H x C x B) image state in the reference's own (Julia WHCN, w fastest) order — the same
 * (B, W*H*C) sample-major device array as everywhere else in this header.  Flat parameters in
 * Lux/ComponentArray order: conv1.weight (3x3x(C+1)xHc, column-major), bn1.scale, bn1.bias,
 * conv2.weight (3x3x(Hc+1)xHc), bn2.scale, bn2.bias, conv3.weight (3x3x(Hc+1)xC).
 * The t plane is concatenated as the last channel before every conv (src/layers/common.jl:10-45) and
 * is zero padded at the border like any other channel.  bn_train = 1: batch statistics (Lux training
 * mode); 0: the running statistics given to lrnde_conv_set_bn_state (default mean 0 / var 1).
 * compute_dtype LRNDE_F32: fp32 MFMA; LRNDE_BF16: bf16 MFMA operands, fp32 accumulation, fp32 state,
 * stage combination and error norm (BASELINE.json config 4); derivatives (lrnde_conv_vjp, _step_reg_grad, _node_backward) of a
 * bf16 handle are taken in fp32 at the states of its bf16 forward solve ("bf16 forward, fp32 adjoint").  LRNDE_F32_SPLIT: fp32 results for conv2 / conv3 on the fp16
 * MFMA pipe — operands written as hi + lo fp16 pairs (22 significant bits), products hi*hi + hi*lo + lo*hi accumulated in
 * fp32; the f-eval agrees with LRNDE_F32 to ~1e-6 of its scale and runs 1.6x faster, but its rounding errors are less
 * correlated between RK stages, so the embedded error estimate carries more noise when it is far below 1.
 * The solver entry points have the meaning of their lrnde_* namesakes above (same reference lines);
 * the adaptive loop's controller runs on the host for this field (an f-eval is 10^2..10^3 us). */
enum { LRNDE_F32 = 0, LRNDE_BF16 = 1, LRNDE_F32_SPLIT = 2 };
typedef struct {
  int32_t width, height, channels; /* state image W, H, C (CIFAR block: 32, 32, 8).  Supported: C = 8, Hc = 64, W % 4 == 0,
                                    * 4 <= W <= 128 (forward; the backward pass up to W = 124), H >= 2; otherwise
                                    * lrnde_conv_create / the call returns LRNDE_UNSUPPORTED */
  int32_t hidden;                  /* Hc (64) */
  int32_t act;                     /* LRNDE_ACT_*: activation inside the BatchNorm layers (gelu) */
  int32_t bn_train;
  int32_t compute_dtype;
  float bn_eps;                    /* Lux default 1e-5 */
} lrnde_conv_desc;
typedef struct lrnde_conv lrnde_conv;
size_t lrnde_conv_param_count(const lrnde_conv_desc* d);
int lrnde_conv_create(lrnde_conv** out, const lrnde_conv_desc* d, int device, void* stream);
int lrnde_conv_destroy(lrnde_conv* c);
const char* lrnde_conv_last_error(const lrnde_conv* c);
int lrnde_conv_set_params(lrnde_conv* c, const float* p, size_t n);               /* device pointer */
int lrnde_conv_set_bn_state(lrnde_conv* c, const float* mean_var, size_t n);      /* device, [mean1 var1 mean2 var2] */
/* The running statistics (st.model of the layer).  With bn_train = 1 every f-eval of rhs / solve / node_forward
 * advances them as Lux's training-mode BatchNorm does on each call (momentum 0.1, unbiased variance), which is
 * what the reference's dudt closure does to its captured st_ (src/layers/neural_ode.jl:44-48); the backward
 * pass's recomputations do not.  Initial value: mean 0, var 1 (Lux initialstates). */
int lrnde_conv_get_bn_state(lrnde_conv* c, float* mean_var, size_t n);            /* device */
/* Lux.trainmode / Lux.testmode for the field's BatchNorm layers after creation (overrides desc.bn_train) */
int lrnde_conv_set_bn_mode(lrnde_conv* c, int32_t bn_train);
/* lrnde_set_solver for the conv handle: the method of the GLOBAL solve in lrnde_conv_solve / lrnde_conv_node_forward* /
 * lrnde_conv_node_backward* (LRNDE_ALG_TSIT5 default, LRNDE_ALG_VCAB3, LRNDE_ALG_VCABM3; UPSTREAM-RECALL, parity unpinned:
 * csrc/lrnde_conv_adams.hpp).  The local regularisation step and the reversed solve of the pullback stay Tsit5; a recorded
 * Adams forward leaves a Hermite record [uprev, k1, P2, P3] per accepted step, which the pullback interpolates.  Every
 * f-eval of an Adams solve advances the running statistics once, as a Tsit5 solve's do.  Works on sharded handles (every
 * rank sets the same method).  Invalidates the forward record.  Any other code: LRNDE_BADARG, the handle stays usable. */
int lrnde_conv_set_solver(lrnde_conv* c, int32_t alg);
int lrnde_conv_rhs(lrnde_conv* c, const float* u, float t, int32_t B, float* du);
int lrnde_conv_init_dt(lrnde_conv* c, const float* u0, int32_t B, float t0, float t1, float abstol,
                       float reltol, float* k1, float* dt_host);
int lrnde_conv_perform_step(lrnde_conv* c, const float* uprev, const float* k1, int32_t B, float t, float dt,
                            float abstol, float reltol, float* u, float* k7, float* eest_host,
                            float* reg_error_host, float* reg_stiff_host);
int lrnde_conv_solve(lrnde_conv* c, const float* u0, int32_t B, float t0, float t1, const lrnde_solve_opts* o,
                     const float* saveat_host, int32_t nsave, float* u_saved, float* t_saved_host,
                     int32_t cap_saved, lrnde_stats* st, lrnde_trace_row* trace_host, int32_t cap_trace);
int lrnde_conv_node_forward(lrnde_conv* c, const float* x, int32_t B, float t0, float t2,
                            const lrnde_solve_opts* o, int32_t mode, int32_t reg_type, float t1_or_rand,
                            float* u_end, float* reg_val_host, int32_t* nfe_host, lrnde_stats* st,
                            float* t1_used_host);
/* Zygote.pullback(dudt, y, p, t) of the conv field (the adjoint RHS building block, as lrnde_vjp): dy = (df/dy)^T lam,
 * gp (device, flat parameter layout, may be NULL) = (df/dp)^T lam; train-mode BatchNorm is differentiated through its
 * batch statistics.  fp32 compute only. */
int lrnde_conv_vjp(lrnde_conv* c, const float* y, float t, const float* lam, int32_t B, float* dy, float* gp);
/* the conv-field instances of lrnde_step_reg_grad / lrnde_node_backward (same meaning, same reference lines) */
int lrnde_conv_step_reg_grad(lrnde_conv* c, const float* uprev, const float* k1, int32_t B, float t, float dt, float abstol,
                             float reltol, int32_t reg_type, float* gp, float* reg_val_host);
int lrnde_conv_node_backward(lrnde_conv* c, const float* x, int32_t B, float t0, float t2, const lrnde_solve_opts* o,
                             int32_t mode, int32_t reg_type, float t1_or_rand, const float* du_end, float w_reg,
                             float* dx, float* dp, lrnde_stats* st_fwd, lrnde_stats* st_bwd);
/* The same in two calls, for a training step that runs the forward once (experiments/src/utils.jl:104-123):
 * lrnde_conv_node_forward_record = lrnde_conv_node_forward that keeps the dense record of the main solve and u(t1);
 * lrnde_conv_node_backward_recorded = the backward pass from that record (invalidated by any later solve on the handle). */
int lrnde_conv_node_forward_record(lrnde_conv* c, const float* x, int32_t B, float t0, float t2, const lrnde_solve_opts* o,
                                   int32_t mode, int32_t reg_type, float t1_or_rand, float* u_end, float* reg_val_host,
                                   int32_t* nfe_host, lrnde_stats* st, float* t1_used_host);
int lrnde_conv_node_backward_recorded(lrnde_conv* c, int32_t B, const float* du_end, float w_reg, float* dx, float* dp,
                                      lrnde_stats* st_bwd);
/* lrnde_set_sensealg for the conv handle: the method of lrnde_conv_node_backward and lrnde_conv_node_backward_recorded.
 * LRNDE_SENSE_INTERPOLATING (the default): the reversed Tsit5 solve of [lambda; mu] over the interpolated record.
 * LRNDE_SENSE_DISCRETE: the discrete adjoint of the recorded Tsit5 solve with the meaning lrnde_set_sensealg states
 * (UPSTREAM-RECALL, frozen grid): loss = <du_end, sol.u[end]> + w_reg * reg_val, the exact derivative of the discrete
 * forward map over the accepted steps of the record, their times and step sizes constants, rejected attempts absent, the
 * first-same-as-last evaluation differentiated; u(t1) of the local step (every saved state of `unbiased` / `biased` mode)
 * stays a constant and the regulariser's gradient is the continuous method's, unchanged.  A reverse sweep over the record
 * (csrc/lrnde_conv_discrete.hpp: the sweep, its order of summation, its workspace): six VJPs per recorded step, no
 * controller, no norm; every launch goes to the handle's stream and the call waits once at the end.  Two calls give the same
 * bits.  lrnde_stats of the backward: naccept = iters = the record's steps, nreject = 0, nf = 6 * steps (the VJPs run).
 * The running statistics are left alone.  Sharded handles take the same method (every rank sets it): the sweep adds no
 * exchange to those of the VJPs; dx stays sharded, dp comes out replicated.
 * The setter does not invalidate the forward record: one record can be pulled back by either method.  It returns
 * LRNDE_BADARG for an unknown code and LRNDE_UNSUPPORTED for DISCRETE on a LRNDE_BF16 or LRNDE_F32_SPLIT handle; the handle
 * stays usable after either.  A backward call with DISCRETE set whose record (or, for the one-call form, whose solver) is
 * VCAB3 / VCABM3 returns LRNDE_UNSUPPORTED ("not a Tsit5 stage record"), touches nothing, never runs the continuous method
 * instead, and leaves the record usable once the setting is changed back. */
int lrnde_conv_set_sensealg(lrnde_conv* c, int32_t sensealg);
/* The accepted steps of the current forward record (lrnde_conv_node_forward_record, any solver): t_host[i], dt_host[i] of
 * step i, *n_host steps — the grid the discrete adjoint holds constant.  LRNDE_BADARG if there is no valid record or
 * cap < the step count (*n_host then holds the count, nothing else is written). */
int lrnde_conv_record_steps(lrnde_conv* c, float* t_host, float* dt_host, int32_t cap, int32_t* n_host);
/* ---- layers around the CIFAR10 NeuralODE (experiments/src/construct.jl:224-227) ----
 * stem: AugmenterLayer(Conv((3,3), 3=>5; pad=1), 3) (src/layers/common.jl:80-92: cat(x, conv(x); dims=3)) + BatchNorm(8);
 * ps (device, 156) = [conv.weight 3x3x3x5 column-major; conv.bias 5; bn.scale 8; bn.bias 8]; x (B,3,H,W) -> u0 (B,8,H,W).
 * BatchNorm(8) follows the handle's bn_train; in test mode bn_state (device, [mean 8; var 8], may be NULL = 0/1) is used.
 * In training mode bn_state_out (device, 16 floats, may be NULL) receives the running statistics Lux's BatchNorm
 * returns in its state: bn_state advanced by this batch (momentum 0.1, n/(n-1) variance correction, as the field's
 * layers, lrnde_conv_get_bn_state); in test mode it receives a copy of bn_state.
 * head: Chain(Conv((3,3), 8=>1, gelu; pad=1), FlattenLayer(), Dense(H*W=>K)) + logitcrossentropy
 * (experiments/src/utils.jl:88); ph (device) = [conv.weight 3x3x8x1; conv.bias 1; dense.weight K x H*W column-major;
 * dense.bias K]; returns the mean loss on the host and, where non-NULL, logits (B,K), du (B,8,H,W), dph.
 * H, W are the handle's image size.  labels: device int32 (B), 0-based; a label outside [0, K) fails the call with
 * LRNDE_BADARG ("a label is outside [0, K)" in lrnde_conv_last_error, as lrnde_classifier_ce) and *loss_host is left
 * alone: whatever the device arrays then hold is not a result.  Run once per batch: simple direct kernels. */
size_t lrnde_cifar_stem_param_count(void);
size_t lrnde_cifar_head_param_count(int32_t H, int32_t W, int32_t K);
int lrnde_cifar_stem_forward(lrnde_conv* c, const float* x, int32_t B, const float* ps, const float* bn_state, float* u0,
                             float* bn_state_out);
int lrnde_cifar_stem_backward(lrnde_conv* c, const float* x, int32_t B, const float* ps, const float* bn_state,
                              const float* du0, float* dps);
int lrnde_cifar_head_ce(lrnde_conv* c, const float* u, int32_t B, const float* ph, int32_t K, const int32_t* labels,
                        float* loss_host, float* logits, float* du, float* dph);

/* ---- batch-sharded conv handle: rank r owns images [r*B, (r+1)*B) of a global batch of nranks*B (the
 * same B on every rank), parameters and BatchNorm running statistics are replicated, and every rank calls the same
 * lrnde_conv_* / lrnde_cifar_* entry point concurrently.  A sharded handle computes what one handle on the global batch
 * computes: global batch statistics (training mode), global error norms and identical accept / reject decisions on
 * every rank; lrnde_cifar_head_ce returns the global mean loss.  gp of lrnde_conv_vjp, dp of lrnde_conv_node_backward*,
 * dps and dph come out summed over ranks and replicated; dy / dx / du stay sharded.  Every exchange is a stream-ordered
 * SUM all-reduce of per-rank slots; all argument checks precede a call's first exchange and every data-dependent
 * failure is decided from exchanged values, so no rank is left waiting.  Ranks called with different B all return
 * LRNDE_BADARG from any call that exchanges something (the check rides in the call's first exchange; a call that couples
 * nothing across ranks - a test-mode f-eval, a test-mode VJP without gp - exchanges nothing and is not checked).
 * nranks == 1 builds no communicator unless LRNDE_FORCE_COMM is set; LRNDE_GATHER_TILES (both read when
 * the communicator is made) exchanges the per-workgroup BatchNorm partials themselves, which reproduces the unsharded
 * statistics bit for bit.  uid: the 128 bytes of lrnde_comm_unique_id.  lrnde_conv_destroy leaves the communicator. */
int lrnde_conv_comm_init(lrnde_conv* c, const void* uid, int32_t rank, int32_t nranks);
int lrnde_conv_comm_destroy(lrnde_conv* c);
int lrnde_conv_comm_count(lrnde_conv* c, int32_t* nranks_host, int32_t* kind_host);      /* 0 none, 1 RCCL, 2 local */

/* `_perform_step(integrator, cache::RKMilCommuteConstantCache, p)`, src/perform_step.jl:108-170, diagonal noise,
 * Ito interpretation: u = K + L*dW + Dgj*J with J = dW^2/2 - |dt|/2, EEst from the 4-argument
 * _calculate_residuals (:218-220); returns u, EEst and EEst*dt.  The reference's du2/En are dead code there
 * (their `tmp` is overwritten at :166) and are not evaluated: 1 drift + 2 diffusion evaluations. */
int lrnde_sde_rkmil_step(lrnde_sde* sde, const float* uprev, const float* dW, int32_t B, float t, float dt,
                         float abstol, float reltol, float* u, float* eest_host, float* reg_val_host);

/* nsteps steps of size dt on a fixed grid, step i from t0 + i*dt with the increments dW[i] (device, nsteps x B x D):
 * the loop a NeuralDSDE forward (src/layers/neural_sde.jl:56-86) runs with a fixed-step solver, without a host round
 * trip per step (Euler-Heun at the one-launch step's shape: ONE launch marches the whole grid).  which: 0 Euler-Heun (src/perform_step.jl:172-206, delta used), 1 Milstein (:108-170).
 * u_traj (device, nsteps x B x D): every step's u; eest_host / reg_val_host (host, nsteps, may be NULL): every step's
 * EEst and EEst*dt.  Step i is bit-identical to the corresponding single-step call. */
int lrnde_sde_solve_fixed(lrnde_sde* sde, int32_t which, const float* u0, const float* dW, int32_t B, float t0, float dt,
                          int32_t nsteps, float abstol, float reltol, float delta, float* u_traj, float* eest_host,
                          float* reg_val_host);

/* Adaptive solve (Euler-Heun here; Milstein and the four-stage SRI step through lrnde_sde_solve_adaptive_alg below): the
 * loop that consumes the step's error estimate (src/perform_step.jl:200-205), which the
 * reference reaches through `solve(prob, solver; ...)` in src/layers/neural_sde.jl:60-72 (StochasticDiffEq, un-vendored).
 * The Brownian path is the CALLER's: W (device, (nfine+1) x B x D) holds it on a uniform grid of nfine intervals over
 * (t0, t1), W[0] = 0.  Steps are whole numbers of grid intervals, so every increment dW = W[j] - W[i] is the path's own
 * and a rejected step is retried over a shorter piece of the SAME path — what StochasticDiffEq's rejection sampling with
 * memory guarantees in distribution, made exact by fixing the path up front.  Step-size control: the PI form of the ODE
 * controller on EEst; StochasticDiffEq's own constants could not be read in this image, so they are
 * options (suggested: gamma 0.9, qmin 0.2, qmax 1.125, beta1 0.14, beta2 0.08).  u_end: the state at t1; the trace
 * (may be NULL) gets one row per attempted step.  On the MNIST-SDE shape (state 32, hidden 64, no time input, unsharded)
 * the controller runs on the device — in the footer of the one-launch step kernel; the host keeps launches enqueued and
 * watches a pinned progress word (12 us per attempted step) — elsewhere the loop is host-controlled, one stream sync per
 * attempted step.  The grid-quantised loop itself is UPSTREAM-RECALL, like the controller's constants. */
typedef struct {
  float abstol, reltol, delta;   /* integrator.opts.abstol / reltol / delta */
  float dt0;                     /* first step (rounded down to whole grid intervals, at least one) */
  float gamma, qmin, qmax, beta1, beta2;
  int32_t maxiters;
} lrnde_sde_adapt_opts;
int lrnde_sde_solve_adaptive(lrnde_sde* sde, const float* u0, const float* W, int32_t nfine, int32_t B, float t0, float t1,
                             const lrnde_sde_adapt_opts* opts, float* u_end, lrnde_stats* stats_host,
                             lrnde_trace_row* trace_host, int32_t cap_trace);

/* Gradient path of the NeuralDSDE layer.  The reference differentiates the SDE solve with TrackerAdjoint — a tape of the
 * solver's own arithmetic (src/layers/neural_sde.jl:12; test/runtests.jl:361-365,386-397) — and reg_val w.r.t. the
 * parameters only (the local step's integrator is built under CRC.@non_differentiable, neural_sde.jl:42).
 * lrnde_sde_solve_fixed_backward: pullback of lrnde_sde_solve_fixed (which = 0, Euler-Heun) for
 * loss = <du_end, u_traj[nsteps-1]>: the reverse sweep through the nsteps steps with the same increments dW
 * (discretise-then-differentiate); dx (B x D), dp_drift (flat drift parameters), dp_diff ([vec(Wg); bg]): device.
 * lrnde_sde_euler_heun_reg_grad: d (EEst*dt) / d (p_drift, p_diffusion) of one local Euler-Heun step
 * (src/perform_step.jl:172-206) with uprev, dW, dt constant; reg_val_host receives EEst*dt. */
int lrnde_sde_solve_fixed_backward(lrnde_sde* sde, const float* u0, const float* u_traj, const float* dW, int32_t B, float t0,
                                   float dt, int32_t nsteps, const float* du_end, float* dx, float* dp_drift, float* dp_diff);
int lrnde_sde_euler_heun_reg_grad(lrnde_sde* sde, const float* uprev, const float* dW, int32_t B, float t, float dt, float abstol,
                                  float reltol, float delta, float* dp_drift, float* dp_diff, float* reg_val_host);
/* The same two for the Milstein step (src/perform_step.jl:108-170; `solver = RKMilCommute()`): pullback of
 * lrnde_sde_solve_fixed(which = 1) and d (EEst*dt) / d parameters of one local step (EEst from the 4-argument residual). */
int lrnde_sde_solve_fixed_backward_rkmil(lrnde_sde* sde, const float* u0, const float* u_traj, const float* dW, int32_t B, float t0,
                                         float dt, int32_t nsteps, const float* du_end, float* dx, float* dp_drift, float* dp_diff);
int lrnde_sde_rkmil_reg_grad(lrnde_sde* sde, const float* uprev, const float* dW, int32_t B, float t, float dt, float abstol,
                             float reltol, float* dp_drift, float* dp_diff, float* reg_val_host);

/* The NeuralDSDE layer itself, forward and pullback: `(n::NeuralDSDE{R})(x, ps, st)` (src/layers/neural_sde.jl:74-123) =
 * `_solve_neuraldsde_generic` (:50-72: ADAPTIVE solve of drift / diffusion from x over tspan with the layer's saveat rules,
 * src/layers/neural_ode.jl:102-116) + for R = unbiased / biased in training mode the local step: a fresh integrator at
 * (sol(t1), t1) over (t1, t2) and one `_perform_step` (:94-98, :116-118; src/perform_step.jl:172-206) whose EEst*dt is
 * reg_val — and what `Zygote.gradient` of the reference's tests takes through it (test/runtests.jl:340-433: TrackerAdjoint
 * tapes the solve's own steps; reg_val w.r.t. the parameters only, neural_sde.jl:42).
 *   forward : x (B x D, device); W: the caller's Brownian path on a uniform grid of nfine intervals over (t0, t2), as for
 *     lrnde_sde_solve_adaptive (device, must stay alive until the backward call); opts: tolerances, delta and the
 *     controller's constants; opts->dt0 <= 0 selects the automatic initial dt (StochasticDiffEq's sde_determine_initdt
 *     restated, UPSTREAM-RECALL), for the main solve (rounded down to whole grid intervals) and for the local step.
 *     mode LRNDE_MODE_* (pass NONE for test mode); t1_or_rand: t1 itself (unbiased; the caller's host RNG draw
 *     rand*(t2-t0)+t0, :92) or the uniform draw r in [0,1) that picks sol.t[floor(r*(len-1))] (biased, :114).
 *     z_local (B x D, device, standard normal): the local step's increment is sqrt(dt_local) * z_local.
 *     save_start: 1 / 0, or -1 for DiffEq's default rule; saveat_host / nsave: the layer's `saveat` kwarg (ascending, may be
 *     empty).  Saved values between step ends come from the SDE solvers' linear interpolant.
 *     u_series (device, cap_series x B x D), t_series_host, nseries_host: sol.u / sol.t as the layer's caller sees them —
 *     after `_CorrectedDESolution` when the layer added t1 to a user saveat (the reference's own method is typed for
 *     ODESolution only, src/utils.jl:31; the behaviour here is the ODE layer's).  sol.u[end] is the last entry.
 *     nfe_drift_host / nfe_diffusion_host: the closures' call counts (:55-65).  stats: the main solve's.
 *   backward: du_series (device, nseries x B x D) = the cotangent of every state of that series; loss = sum_j <du_j, u_j> +
 *     w_reg * reg_val.  dx (B x D), dp_drift (flat drift parameters), dp_diff ([vec(Wg); bg]): device.  The reverse sweep walks
 *     the recorded accepted steps with their own dt and dW. */
int lrnde_sde_node_forward_record(lrnde_sde* sde, const float* x, const float* W, int32_t nfine, int32_t B, float t0, float t2,
                                  const lrnde_sde_adapt_opts* opts, int32_t mode, float t1_or_rand, const float* z_local,
                                  int32_t save_start, const float* saveat_host, int32_t nsave, float* u_series,
                                  float* t_series_host, int32_t cap_series, int32_t* nseries_host, float* reg_val_host,
                                  int32_t* nfe_drift_host, int32_t* nfe_diffusion_host, lrnde_stats* stats_host, float* t1_used_host);
int lrnde_sde_node_backward_recorded(lrnde_sde* sde, int32_t B, const float* du_series, int32_t nseries, float w_reg, float* dx,
                                     float* dp_drift, float* dp_diff);

/* Which recorded forward a handle's record belongs to: the count of successful lrnde_*_forward_record* calls on it (0 = no
 * usable record).  A binding's pullback closure keeps the value it saw after ITS forward and compares before calling
 * lrnde_*_backward_recorded*: a later forward on the same handle (an evaluation pass between forward and pullback, nested
 * AD) has replaced the record, and the backward would silently differentiate the other input.  julia/LRNDELayer.jl re-runs
 * its forward in that case. */
int lrnde_record_generation(lrnde_ctx* ctx, uint64_t* gen_host);
int lrnde_conv_record_generation(lrnde_conv* c, uint64_t* gen_host);
int lrnde_sde_record_generation(lrnde_sde* sde, uint64_t* gen_host);

/* Gaussian noise for the SDE layers, drawn on the handle's device and stream (no host sync).
 * out (device): cumulative = 1 -> (nsteps+1) x B x D, out[0] = 0, the Brownian path on a uniform grid;
 *               cumulative = 0 -> nsteps x B x D increments scale * z.  stream: 0 path W, 1 local-step z,
 *               2 fixed-grid dW, 3 fixed-grid dZ, 4 the adaptive SRI solve's second path Z, 5 its local-step z2
 *               (callers may use others).  scale = sqrt(h), computed by the caller.
 * Normal j of column c = b*D + d is Box-Muller (float64, rounded once) on Philox-4x32-10 at counter (j >> 2, c, stream, 0),
 * key (seed & 0xffffffff, seed >> 32): it depends on (seed, stream, b, d, j) only, not on B or nsteps.
 * The path is the sequential fp32 sum of the fp32 products scale * z.  B x D may not exceed 2^30. */
int lrnde_sde_draw_noise(lrnde_sde* sde, uint64_t seed, uint32_t stream, int32_t nsteps, int32_t B, float scale,
                         int32_t cumulative, float* out);

/* The Brownian path of the adaptive entry points as a VIRTUAL TREE: W at a grid index is a pure function of (seed, stream,
 * column, index) — a Levy / Brownian-bridge construction on lrnde_sde_draw_noise's normals — so a solve needs no
 * (nfine+1) x B x D array, its resolution is not tied to memory, and a rejected step re-queries the same path.
 * Definition (the kernels are held to it bit for bit; tests/brownian_tree_np.py restates it):  nfine = 2^L, 0 <= L <= 20;
 * span = t2 - t0 in float32; column c = b*D + d; z[n], n = 0 .. nfine-1, is standard normal n of column c in the stream exactly
 * as lrnde_sde_draw_noise(seed, stream, nfine, B, 1.0, increments) returns it (counter (n >> 2, c, stream, 0), word n & 3,
 * float64 Box-Muller rounded once).  Streams: 6 is the tree of W, 7 the tree of SRI's second path Z (0..5 keep their meaning).
 * Every operation is a single float32 operation, no contraction:
 *   W[0] = 0;  W[nfine] = sT * z[0], sT = (float)sqrt((double)span);
 *   for level l = 1 .. L and node j = 0 .. 2^(l-1) - 1:  a = j * 2^(L-l+1), b = a + 2^(L-l+1), mid = a + 2^(L-l), n = 2^(l-1) + j,
 *     W[mid] = (0.5 * (W[a] + W[b])) + (s_l * z[n]),  s_l = (float)(0.5 * sqrt((double)span * 2^-(l-1))).
 * A query for index k descends from (0, nfine) computing only the midpoints on its way: L - ctz(k) levels.  A column's path
 * depends on (seed, stream, b, d, k / nfine, span) only — not on B or the launch — and the tree is refinement-consistent:
 * W_L[k] == W_L'[k * 2^(L'-L)] bit for bit.
 * lrnde_sde_tree_path: the whole array of that definition, out (device, (2^levels + 1) x B x D), on the handle's stream (no host
 *   sync) — to look at a path, and the yardstick of the tests.
 * lrnde_sde_set_path_tree(enable = 1, seed): from then on lrnde_sde_solve_adaptive(_alg), lrnde_sde_node_forward_record(_alg)
 *   and lrnde_sde_model_forward_record_ce IGNORE their W and Z arguments (NULL is fine) and take the path from the tree of `seed`
 *   at L = log2(nfine) over the call's (t0, t2), stream 6 for W and 7 for Z.  nfine that is no power of two, or above 2^20, is
 *   LRNDE_BADARG with a message.  The recorded forward keeps the accepted steps' increments beside their end states (the record
 *   starts at 64 steps and is replaced by one four times as large, up to min(nfine, maxiters), when a solve ends with
 *   LRNDE_CAPACITY — the solve then runs again on the same path) and every backward route reads them from there: no backward call regenerates noise or reads a
 *   path.  enable = 0 (the default): the caller's arrays, as before — including the refusal of a NULL W.  A record remembers the
 *   source it was made with.  A sharded handle refuses the tree with LRNDE_BADARG: a shard numbers its columns from its own
 *   first sample, and the path of a sample must not depend on the sharding.
 * The grid-quantised adaptive loop that consumes the path is UPSTREAM-RECALL like its neighbours above (StochasticDiffEq's own
 * rejection sampling with memory is un-vendored and not restated). */
int lrnde_sde_tree_path(lrnde_sde* sde, uint64_t seed, uint32_t stream, int32_t levels, int32_t B, float t0, float t2, float* out);
int lrnde_sde_set_path_tree(lrnde_sde* sde, int32_t enable, uint64_t seed);

/* `_perform_step(integrator, cache::FourStageSRIConstantCache, p)`, src/perform_step.jl:49-106 — the step the
 * reference's default SDE solver SOSRI runs — diagonal noise: four drift and four diffusion evaluations, the
 * increments dW and dZ of the caller's noise process (device, B x D each), u, EEst from the 7-argument
 * _calculate_residuals (:214-216) and EEst*dt.  The tableau is NOT part of this library: SOSRI's coefficients live in
 * un-vendored StochasticDiffEq; the caller passes the cache's fields in the order the reference unpacks them (:51-55). */
typedef struct lrnde_sri_tableau {
  float a021, a031, a032, a041, a042, a043, a121, a131, a132, a141, a142, a143;
  float b021, b031, b032, b041, b042, b043, b121, b131, b132, b141, b142, b143;
  float c02, c03, c04, c11, c12, c13, c14, alpha1, alpha2, alpha3, alpha4;
  float beta11, beta12, beta13, beta14, beta21, beta22, beta23, beta24, beta31, beta32, beta33, beta34, beta41, beta42, beta43, beta44;
} lrnde_sri_tableau;
int lrnde_sde_sri_step(lrnde_sde* sde, const lrnde_sri_tableau* tab, const float* uprev, const float* dW, const float* dZ,
                       int32_t B, float t, float dt, float abstol, float reltol, float delta, float* u, float* eest_host,
                       float* reg_val_host);

/* The adaptive solve and the layer's recorded forward with the step as a parameter — the reference passes whatever n.solver
 * is to `solve` and to the local step (src/layers/neural_sde.jl:68-69,96,116).  The arguments of lrnde_sde_solve_adaptive /
 * lrnde_sde_node_forward_record, then:
 *   which    : 0 Euler-Heun (src/perform_step.jl:172-206), 1 Milstein (:108-170), 2 four-stage SRI (:49-106) — the codes of
 *              lrnde_sde_solve_fixed, extended by 2.  The two older entry points are these with which = 0: same launches, same bits.
 *   tab      : SRI only — the caller's tableau.
 *   Z        : SRI only — the second Brownian path on the same uniform grid, (nfine+1) x B x D, Z[0] = 0 (device, alive until
 *              the backward call); a step's dZ = Z[i+m] - Z[i].
 *   z2_local : SRI only, the recorded forward only — the local step's dZ = sqrt(dt_local) * z2_local (B x D, device).
 * SRI without tab or Z (or without z2_local when regularising) and which outside 0..2 return LRNDE_BADARG with a message.
 * Evaluations per attempted step, (drift, diffusion): Euler-Heun (3, 3), Milstein (1, 2), SRI (4, 4); the automatic initial dt
 * adds (2, 2).  lrnde_stats.nf is the drift count.
 * Where the controller runs: all three kinds at the one-launch kernels' shape (D <= 64, H <= 128, no time input,
 * unsharded) on the device — Milstein in the footer of k_sde_mil_fast, SRI in the footer of k_sde_sri_fast, one launch per
 * attempted step, no stream sync inside the solve.  Host-controlled, one stream sync per attempted step: Milstein and SRI
 * outside that shape (or with LRNDE_SDE_HOST_LOOP=1).
 * UPSTREAM-RECALL (StochasticDiffEq is not vendored; beside the controller's constants, which stay the caller's options):
 * the strong orders the automatic initial dt takes — 1/2 Euler-Heun, 1 Milstein, 3/2 SRI.
 * lrnde_sde_node_backward_recorded sweeps a record with the reverse kernels of the kind that made it: per recorded step the
 * kernels behind lrnde_sde_solve_fixed_backward_rkmil / lrnde_sde_sri_step_backward, one launch sequence per step; the
 * regulariser's parameter gradient from lrnde_sde_rkmil_reg_grad's kernels / the SRI reverse with du_new = NULL, dx = NULL. */
int lrnde_sde_solve_adaptive_alg(lrnde_sde* sde, const float* u0, const float* W, int32_t nfine, int32_t B, float t0, float t1,
                                 const lrnde_sde_adapt_opts* opts, float* u_end, lrnde_stats* stats_host,
                                 lrnde_trace_row* trace_host, int32_t cap_trace, int32_t which, const lrnde_sri_tableau* tab,
                                 const float* Z);
int lrnde_sde_node_forward_record_alg(lrnde_sde* sde, const float* x, const float* W, int32_t nfine, int32_t B, float t0, float t2,
                                      const lrnde_sde_adapt_opts* opts, int32_t mode, float t1_or_rand, const float* z_local,
                                      int32_t save_start, const float* saveat_host, int32_t nsave, float* u_series,
                                      float* t_series_host, int32_t cap_series, int32_t* nseries_host, float* reg_val_host,
                                      int32_t* nfe_drift_host, int32_t* nfe_diffusion_host, lrnde_stats* stats_host,
                                      float* t1_used_host, int32_t which, const lrnde_sri_tableau* tab, const float* Z,
                                      const float* z2_local);
/* Reverse sweep of ONE four-stage SRI step (src/perform_step.jl:49-106; lrnde_sde_sri_step with the same arguments):
 * loss = <du_new, u'> + w_reg * EEst*dt.  du_new (device, may be NULL = 0): cotangent of the step's result; dx (device, may be
 * NULL): cotangent of uprev — NULL when uprev is a constant of the tape, as for the local step's regulariser
 * (src/layers/neural_sde.jl:42); dp_drift / dp_diff (device): the parameter cotangents are ADDED (zero them first; a solve's
 * pullback calls this once per step, newest first).  dW, dZ, dt are constants.  reg_val_host (may be NULL): EEst*dt.
 * With w_reg != 0, dx holds the whole derivative of w_reg * EEst*dt with respect to uprev: through u', through the stages, and
 * through the residual's scale abstol + max(|uprev|, |u'|) * reltol on whichever side carries the maximum (a tie: uprev). */
int lrnde_sde_sri_step_backward(lrnde_sde* sde, const lrnde_sri_tableau* tab, const float* uprev, const float* dW, const float* dZ,
                                int32_t B, float t, float dt, float abstol, float reltol, float delta, const float* du_new,
                                float w_reg, float* dx, float* dp_drift, float* dp_diff, float* reg_val_host);

/* ---- the MNIST-SDE model around the layer (experiments/src/construct.jl:202-210):
 *   Chain(flatten, downsample = Dense(Din => D), neural_dsde, sol_to_arr, classifier = Dense(D => K)),
 *   loss = logitcrossentropy(y_pred, y) + w_reg * st.neural_dsde.reg_val (construct.jl:18-31).  D is the handle's state size.
 *
 * lrnde_sde_dense_forward — `downsample = Dense(784 => 32)` (construct.jl:203): u0[b][o] = sum_k W[o][k] x[b][k] + b[o].
 *   x (B x Din, row-major = Julia's Din x B), pd = the flat Lux block [vec(W) (D x Din, column-major: W[o][k] at o + D*k); b (D)],
 *   u0 (B x D): device.  One sample's result does not depend on B or on where the sample sits in the batch.
 * lrnde_sde_dense_backward — that layer's pullback (what Zygote takes through construct.jl:203): dpd = [vec(dW); db] with
 *   dW[o][k] = sum_b du0[b][o] x[b][k], db[o] = sum_b du0[b][o], summed over the batch in a fixed order (no atomics), and
 *   dx = du0 W (B x Din) when dx is not NULL — the experiment never asks for it (x is data).
 * lrnde_sde_classifier_ce — `classifier = Dense(32 => num_classes)` + logitcrossentropy (construct.jl:209, :18-31;
 *   experiments/src/utils.jl:88) on the SDE handle: the arguments, layout, arithmetic and errors of lrnde_classifier_ce
 *   (K in 1..16; a label outside [0, K) returns LRNDE_BADARG).
 * lrnde_sde_model_forward_record_ce — the forward half of the training step (construct.jl:18-31 through :202-210): downsample ->
 *   lrnde_sde_node_forward_record_alg -> head on sol.u[end]; the same values, bit for bit, as the three calls.  The arguments
 *   are x, Din, pd, then those of lrnde_sde_node_forward_record_alg without its x, then pc, K, labels, loss_host, logits
 *   (B x K, may be NULL), dpc (may be NULL) of the head.  The downsample is enqueued ahead of the layer, the head behind it, and
 *   one final wait delivers the loss.  The record keeps what the pullback needs (the head's cotangent of sol.u[end] included)
 *   and refers to x, pd, W (and Z): they stay alive until the backward call.  It counts in lrnde_sde_record_generation.
 * lrnde_sde_model_backward_recorded — the pullback from that record (what `Zygote.pullback` of construct.jl:18-31 returns):
 *   the series cotangent (zero but for the head's du on the last entry) -> lrnde_sde_node_backward_recorded with w_reg ->
 *   lrnde_sde_dense_backward on its dx.  dpd, dp_drift, dp_diff: device; dx (B x Din) may be NULL.  One synchronisation at the
 *   end.  Without a usable record — none yet, another batch size, or a later forward on the handle — LRNDE_BADARG.
 * NULL handles and pointers, B < 1, Din < 1, K outside 1..16 return a status. */
int lrnde_sde_dense_forward(lrnde_sde* sde, const float* x, int32_t B, int32_t Din, const float* pd, float* u0);
int lrnde_sde_dense_backward(lrnde_sde* sde, const float* x, int32_t B, int32_t Din, const float* pd, const float* du0, float* dpd,
                             float* dx);
int lrnde_sde_classifier_ce(lrnde_sde* sde, const float* u, int32_t B, const float* pc, int32_t K, const int32_t* labels,
                            float* loss_host, float* logits, float* du, float* dpc);
int lrnde_sde_model_forward_record_ce(lrnde_sde* sde, const float* x, int32_t Din, const float* pd, const float* W, int32_t nfine,
                                      int32_t B, float t0, float t2, const lrnde_sde_adapt_opts* opts, int32_t mode, float t1_or_rand,
                                      const float* z_local, int32_t save_start, const float* saveat_host, int32_t nsave,
                                      float* u_series, float* t_series_host, int32_t cap_series, int32_t* nseries_host,
                                      float* reg_val_host, int32_t* nfe_drift_host, int32_t* nfe_diffusion_host,
                                      lrnde_stats* stats_host, float* t1_used_host, int32_t which, const lrnde_sri_tableau* tab,
                                      const float* Z, const float* z2_local, const float* pc, int32_t K, const int32_t* labels,
                                      float* loss_host, float* logits, float* dpc);
int lrnde_sde_model_backward_recorded(lrnde_sde* sde, int32_t B, float w_reg, float* dpd, float* dp_drift, float* dp_diff, float* dx);


/* ---- backward pass ----
 * lrnde_vjp: the vector-Jacobian product Zygote.pullback(dudt, y, p, t) computes inside the adjoint
 * RHS (SciMLSensitivity ZygoteVJP): dy = (df/dy)^T lam, gp = (df/dp)^T lam (flat Lux layout, may be
 * NULL).  All device pointers. */
int lrnde_vjp(lrnde_ctx* ctx, const float* y, float t, const float* lam, int32_t B, float* dy, float* gp);

/* d reg_val / d ps for one local step: Zygote through `_perform_step` with integrator, k1, dt, uprev
 * constant (src/layers/neural_ode.jl:40, src/utils.jl:60; asserted by test/runtests.jl:127-131:
 * no gradient w.r.t. x).  gp: device vector of lrnde_param_count floats. */
int lrnde_step_reg_grad(lrnde_ctx* ctx, const float* uprev, const float* k1, int32_t B, float t, float dt,
                        float abstol, float reltol, int32_t reg_type, float* gp, float* reg_val_host);

/* Pullback of the NeuralODE layer for  loss = <du_end, sol.u[end]> + w_reg * reg_val
 * (what Zygote.pullback computes in experiments/src/utils.jl:104-115): forward re-solve with a dense
 * record, continuous adjoint of `solve` (SciMLSensitivity InterpolatingAdjoint(autojacvec=ZygoteVJP()):
 * reversed-time adaptive Tsit5 on [lambda; mu], same tolerances, cotangent times as tstops), plus the
 * regulariser's reverse sweep.  dx (B,D) and dp (P) are device outputs. */
int lrnde_node_backward(lrnde_ctx* ctx, const float* x, int32_t B, float t0, float t2,
                        const lrnde_solve_opts* opts, int32_t mode, int32_t reg_type, float t1_or_rand,
                        const float* du_end, float w_reg, float* dx, float* dp, lrnde_stats* stats_fwd_host,
                        lrnde_stats* stats_bwd_host);

/* ---- optimiser update rules of the experiments: experiments/src/construct.jl:104-126 builds
 * Adam / AdamW / AdaMax / Descent / Momentum / Nesterov (Optimisers.jl, un-vendored: rules restated from its documented
 * update formulas) and chains WeightDecay when cfg.weight_decay != 0.  One fused pass over a flat parameter vector:
 * x -= rule(grad) + weight_decay * x.  state1 / state2: the rule's moment vectors (device, n floats, zero-initialised by
 * the caller; unused ones may be NULL); step: 1-based update count (bias correction beta^step); eta: the learning rate
 * the scheduler returned for this step (experiments/src/utils.jl:1-68; host mirror: localregneuralde.jl_amd/optim.py).
 * AdamW(eta) = LRNDE_OPT_ADAM with weight_decay = its decay. */
enum { LRNDE_OPT_DESCENT = 0, LRNDE_OPT_MOMENTUM = 1, LRNDE_OPT_NESTEROV = 2, LRNDE_OPT_ADAM = 3, LRNDE_OPT_ADAMAX = 4 };
int lrnde_opt_update(int32_t kind, float* x, const float* grad, float* state1, float* state2, size_t n, float eta,
                     float rho_or_beta1, float beta2, float eps, int32_t step, float weight_decay, int device, void* stream);

/* ---- Latent ODE (the PhysioNet experiment): the layers `_construct_time_series` puts around the NeuralODE,
 * experiments/src/construct.jl:230-252.  The `neural_ode` block itself is a Dense-chain handle (lrnde_create_chain).
 *   gru          Recurrence(LatentGRUCell(in_dims, hidden_dims, latent_dims)), src/layers/latent_ode.jl:1-48;
 *   rec_to_gen   Chain(Dense(2L => L, tanh), Dense(L => 2N)), construct.jl:232-233;
 *   reparam      ReparameterizeLayer, src/layers/common.jl:47-77;
 *   gen_to_data  Dense(N => in_dims), construct.jl:250;
 *   loss         construct.jl:36-76 with log_likelihood_loss and kl_divergence, experiments/src/utils.jl:94-101.
 * I = in_dims, F = 2I + 1 (rows of x = vcat(data, mask, dt), construct.jl:40), H = hidden_dims, L = latent_dims,
 * N = node_dims.  Parameters: the flat Lux ComponentArray in the order gru.update_gate (layer_1 W (H x (2L+F)), b;
 * layer_2 W (L x H), b), gru.reset_gate (the same), gru.new_state (layer_2: 2L x H), rec_to_gen (L x 2L, b; 2N x L, b),
 * gen_to_data (I x N, b); every W column-major out x in, the input rows of a gate's first layer in the order of
 * vcat(y_mean, y_std, x) (latent_ode.jl:26).  latent_ode.jl:37 builds new_y_mean from new_state_std: rows 0..L-1 of
 * new_state's second layer are parameters without effect, and their cotangent is exactly zero.
 * Arrays: x (B, T, F), data / mask (B, T, I) contiguous (Julia's (F, T, B) / (I, T, B)); y (B, 2L); mu, logvar, z0,
 * eps (B, N); series (T, B, N) as lrnde_node_forward_record_ts returns it (diffeqsol_to_timeseries, src/utils.jl:42-46).
 * Limits (LRNDE_UNSUPPORTED with a message from lrnde_latent_last_error(NULL) / (h)): 3 * hidden_dims <= 128, and the
 * gates' weight image plus the backward's activations within the 160 KiB of LDS of a CU; 37/40/50/20 needs 143 KiB. */
typedef struct {
  int32_t in_dims, hidden_dims, latent_dims, node_dims;   /* cfg.ts_in_dims, ts_hidden_dims, ts_latent_dims, ts_node_dims */
} lrnde_latent_desc;
typedef struct lrnde_latent lrnde_latent;
/* construct.jl:230-252 (the layers' construction) / Lux.setup's parameter count for them / the ComponentArray itself */
int lrnde_latent_create(lrnde_latent** out, const lrnde_latent_desc* desc, int device, void* stream);
int lrnde_latent_destroy(lrnde_latent* h);
const char* lrnde_latent_last_error(const lrnde_latent* h);
size_t lrnde_latent_param_count(const lrnde_latent_desc* desc);
int lrnde_latent_set_params(lrnde_latent* h, const float* p, size_t n);
/* gru, rec_to_gen and reparam of the Chain, construct.jl:251, in ONE launch: Recurrence with return_sequence = false
 * walks the T steps (latent_ode.jl:19-47, the first call with y_mean = 0, y_std = 1) and returns the last y (B, 2L);
 * training != 0: z0 = mu + exp(logvar / 2) .* eps (common.jl:61-71) with the caller's normal draws eps; training = 0:
 * z0 = mu and logvar := mu as written in common.jl:73-77 (eps may be NULL).  y / mu / logvar / z0 may be NULL.  The call
 * is stream-ordered and keeps the record of ONE lrnde_latent_encode_backward. */
int lrnde_latent_encode(lrnde_latent* h, const float* x, int32_t B, int32_t T, int32_t training, const float* eps, float* y,
                        float* mu, float* logvar, float* z0);
/* The pullback of the above (what Zygote.pullback gives, experiments/src/utils.jl:104-115) for cotangents of z0 and of
 * st.reparam's mu / logvar (the KL term sends those, construct.jl:48), and optionally of y itself (dy (B, 2L): Recurrence
 * used outside the model); any of the four may be NULL (zero).  x: the array
 * the recorded encode read.  dx (B, T, F) may be NULL; dp: the first lrnde_latent_param_count - (I*N + I) entries of the
 * flat vector (gru, rec_to_gen).  Two launches: the reverse walk and the workgroup-order sum of its partials. */
int lrnde_latent_encode_backward(lrnde_latent* h, const float* x, int32_t B, int32_t T, const float* dy, const float* dz0,
                                 const float* dmu, const float* dlogvar, float* dx, float* dp);
/* gen_to_data, the last layer of the Chain (construct.jl:250-251): pred (B, T, I) = Dense(N => I) on every state of
 * series (T, B, N).  Stream-ordered. */
int lrnde_latent_decode(lrnde_latent* h, const float* series, int32_t T, int32_t B, float* pred);
/* gen_to_data on every saved state and the loss without the regulariser, construct.jl:43-50: ll (B) =
 * log_likelihood_loss(pred .* mask .- data .* mask, mask) (utils.jl:94-98, sigma = 0.01, summed over every (feature, time)
 * entry and divided by the column's mask sum), kl (B) = kl_divergence(mu, logvar) (utils.jl:101),
 * loss_host[0] = -mean(ll .- w_kl .* kl), loss_host[1] = -mean(ll), loss_host[2] = mean(kl) (the stats of
 * construct.jl:71-73).  Where non-NULL: the cotangents of the loss for series (T, B, N), mu, logvar (B, N) and
 * gen_to_data's parameters dpg (I*N + I).  Synchronises the stream. */
int lrnde_latent_decode_loss(lrnde_latent* h, const float* series, int32_t T, int32_t B, const float* data, const float* mask,
                             const float* mu, const float* logvar, float w_kl, float* loss_host, float* ll, float* kl,
                             float* dseries, float* dmu, float* dlogvar, float* dpg);
/* lrnde_record_generation for this handle: counts the encodes; 0 = no usable record (none yet, consumed by a backward, or
 * the parameters were set again). */
int lrnde_latent_record_generation(lrnde_latent* h, uint64_t* gen_host);

#ifdef __cplusplus
}
#endif
#endif
