"""Shapes, inputs and selection conditions of the record-growth and failed-solve tests of the Dense-chain handles
(tests/test_gpu_record_growth.py, tests/test_host_record_growth.py), importable without a GPU.

The dense record of a recorded forward starts at 64 accepted steps (node_forward_record_impl, csrc/lrnde_kernels.hip); a solve
that needs more is stopped by the step kernel's footer with LRNDE_CAPACITY, the record is doubled and the whole forward
runs again.  Every case here is a solve that crosses that line once (more than 64 accepted steps) or twice (more than 128),
or a solve that fails after many accepted steps.

How the cases were picked, and what the host test re-derives on every CPU run: the C oracle's solve over two CPU fields, the
float32 numpy field (chain_adams_cases.np_field) and the float64 field rounded once (test_gpu_chain.Chain64), gives the
accepted-step counts of COUNTS below.  At tolerance 1e-7 the two fields differ by up to 10 % (the step decisions are
rounding there), so no Tsit5 test asserts a count; each GPU test asserts on its own result that naccept is above the line it
is about, and the host test asserts that both CPU counts clear that line by MARGIN_UP and, where a test claims exactly one
doubling, stay below MARGIN_DOWN x 128.

Bars that are not 1e-5, 3e-4 or an existing test's (measured origin: the two CPU restatements and their distance; then what
the MI355X gave):

  solution against float64 (test_solution_against_float64_restatement): max(1e-5, 0.5 tol, 4 x the distance of
  np_restatement.solve over Chain32 from the same solve over Chain64), relative to the largest state.  Twin distances on
  the CPU: phys_74 6.2e-5, phys_119 2.8e-4, phys_196 3.5e-3, small3_176 1.2e-6, odd130_87 7.5e-6.
  MI355X: see SOLUTION_GPU below.

  continuous pullback against float64 autograd (test_continuous_pullback_against_float64_autograd): max(3e-4, 4 x the
  distance of chain_adjoint_np.pullback in float32 from the same in float64), relative to each gradient's norm.  Twin
  distances on the CPU: phys_119 dx 1.6e-2, dp 1.6e-2 (the float32 restatement's reversed solve takes 2137 steps where the
  float64 one takes 480: at 1e-7 the PhysioNet chain at weights x3 amplifies rounding through the reversed solve);
  odd130_87 dx 5.3e-5, dp 5.5e-5, so its bar is the project's 3e-4.  MI355X: see PULLBACK_GPU below.

  discrete pullback: the bars of tests/test_gpu_chain_discrete.py, max(1e-5, 4 x float32 twin of frozen_grads).  On the
  CPU's own grids that is 3e-3 .. 8e-3 for phys_74 and 0.3 .. 3 for phys_196 (the PhysioNet chain at weights x3 loses its
  gradient to rounding over 190 steps of span (0, 2): that bar holds nothing, and what holds the sweep there are the step
  counts of stats_bwd and the bits of the second call).  small3_176 (2e-5 .. 5e-5) is added for the small handle so that
  one walk over more than 128 recorded steps is held to a bar that means something."""
import functools
import os

import numpy as np
import torch

import chain_adams_cases as K
import wide_chain_cases as WC

f32 = np.float32

FIRST_RECORD = 64          # accepted steps the first record holds
SECOND_RECORD = 128        # ... and the record after one doubling
MARGIN_UP = 1.15           # both CPU counts >= MARGIN_UP x the line a test is about
MARGIN_DOWN = 0.85         # both CPU counts <= MARGIN_DOWN x 128 where a test claims exactly one doubling
T1_FRACTION = 0.43         # :unbiased takes t1 = 0.43 x span; :biased draws its index with 0.43
SERIES_FRACTIONS = (0.1, 0.5, 0.93, 1.0)
DISCRETE_FRACTIONS = (0.3, 0.7, 1.0)
W_REG = 2.5
B_OTHER = 5                # "another batch and back": dense_n changes, the record is reallocated at the grown capacity
MAX_ATTEMPTS = 1000        # every lin8 solve stays under this

# name -> model, batch, weight scale, tolerance, span, solver, the line it crosses, whether it claims exactly one doubling.
# B = 9: a second, partly filled 8-column tile of the small chain.  B = 17: a second 16-column tile with one column on the
# wide handle, three workgroups on the small one.
CASES = {
    "phys_74": dict(model="physionet", B=9, scale=3.0, tol=1e-6, span=(0.0, 1.0), solver="tsit5", line=64, one_doubling=True),
    "phys_119": dict(model="physionet", B=17, scale=3.0, tol=1e-7, span=(0.0, 1.0), solver="tsit5", line=64, one_doubling=False),
    "phys_196": dict(model="physionet", B=17, scale=3.0, tol=1e-7, span=(0.0, 2.0), solver="tsit5", line=128, one_doubling=False),
    "small3_176": dict(model="small3", B=5, scale=3.0, tol=1e-7, span=(0.0, 6.0), solver="tsit5", line=128, one_doubling=False),
    "odd130_87": dict(model="odd130", B=17, scale=3.0, tol=1e-7, span=(0.0, 2.0), solver="tsit5", line=64, one_doubling=False),
    "phys_vcab3_1e-3": dict(model="physionet", B=9, scale=3.0, tol=1e-3, span=(0.0, 1.0), solver="vcab3", line=64, one_doubling=True),
    "phys_vcab3_1e-4": dict(model="physionet", B=9, scale=3.0, tol=1e-4, span=(0.0, 1.0), solver="vcab3", line=128, one_doubling=False),
    "phys_vcabm3_1e-4": dict(model="physionet", B=9, scale=3.0, tol=1e-4, span=(0.0, 1.0), solver="vcabm3", line=64, one_doubling=True),
    "phys_vcabm3_1e-5": dict(model="physionet", B=9, scale=3.0, tol=1e-5, span=(0.0, 1.0), solver="vcabm3", line=128, one_doubling=False),
    # small3_176's inputs with VCAB3: a Hermite record of several hundred steps on a field whose gradient survives rounding
    "small3_vcab3_1e-7": dict(model="small3", B=5, scale=3.0, tol=1e-7, span=(0.0, 6.0), solver="vcab3", line=128, one_doubling=False),
}
# accepted steps of the C oracle's solve on the CPU: (over the float32 numpy field, over the float64 field rounded once)
COUNTS = {
    "phys_74": (74, 74), "phys_119": (119, 117), "phys_196": (196, 192), "small3_176": (176, 168), "odd130_87": (87, 79),
    "phys_vcab3_1e-3": (82, 82), "phys_vcab3_1e-4": (149, 149), "phys_vcabm3_1e-4": (81, 81), "phys_vcabm3_1e-5": (155, 155),
    "small3_vcab3_1e-7": (1340, 1340),
}
TSIT5_SMALL = ("phys_74", "phys_119", "phys_196", "small3_176")     # the small handle
TSIT5_WIDE = ("phys_74", "phys_196", "odd130_87")                   # the wide handle (widths 20 / 40 too; same f-eval bits)
ADAMS = ("phys_vcab3_1e-3", "phys_vcab3_1e-4", "phys_vcabm3_1e-4", "phys_vcabm3_1e-5")
# the series pullback over a Hermite record against float64 autograd: the issue's case, where the gradient at tolerance
# 1e-4 is lost to the chain's amplification with either solver (Tsit5 and VCAB3 are both 0.9 of the reference's norm away,
# so the rule "twice the Tsit5 pullback's error" holds nothing there), and small3, where 3e-4 means something.  The
# tolerance of the small3 case comes from the CPU: the oracle's VCAB3 solve over the float32 field is 5.8e-5 of the state's
# scale from scipy DOP853 (float64, 1e-12) at tolerance 1e-6 and 1.3e-5 at 1e-7, where Tsit5 at 1e-6 is 6e-7 away.  A
# pullback is no better than the solution it differentiates: with VCAB3 at 1e-6 (754 steps) the MI355X gave 5.2e-4 / 5.0e-4
# for dx / dp, 9 x the solution's error and over the bar by the solver's truncation alone (Tsit5 on the same inputs:
# 3.1e-5 / 4.0e-5).  So the case takes 1e-7: 1340 steps, the record grown five times.
# Each entry: (case, the pullback case whose inputs and RK4 reference it shares)
ADAMS_PULLBACK = (("phys_vcab3_1e-4", "phys_vcab3_1e-4"), ("small3_vcab3_1e-7", "small3_176"))

# MaxIters past the first record: phys_74 with maxiters = 70 fills the record at step 65, retries, and stops at iteration 71:
# 66 accepted and 4 rejected attempts with either CPU field.  The VCABM3 handle of the recovery test takes phys_vcabm3_1e-5
# the same way (its first 70 attempts hold at most 5 rejected ones: asserted in the host test).
MAXITERS_PAST = 70
MAXITERS_PAST_COUNTS = (66, 4)

# what the MI355X gave against the bars above (relative distance -> bar)
SOLUTION_GPU = {   # both handles alike: sol.u[end] from the float64 restatement -> bar
    "phys_74": (1.12e-4, 2.47e-4), "phys_119": (3.81e-4, 1.11e-3), "phys_196": (4.40e-3, 1.42e-2), "small3_176": (2.05e-6, 1.0e-5),
    "odd130_87": (1.03e-5, 2.99e-5),
}
PULLBACK_GPU = {   # both handles alike: (dx, dp) from float64 autograd -> bar
    "phys_119": ((2.24e-2, 2.27e-2), 6.4e-2), "odd130_87": ((6.75e-5, 6.69e-5), 3e-4), "small3_176": ((2.16e-5, 1.57e-5), 3e-4),
    # the Adams records: VCAB3 (Tsit5 on the same inputs and tolerance)
    "phys_vcab3_1e-4": ((0.957, 0.886), (0.962, 0.878)), "small3_vcab3_1e-7": ((7.20e-5, 7.22e-5), (2.16e-5, 1.57e-5)),
}
DISCRETE_GPU = {   # both sweeps alike: (dx, dp) from frozen_grads in float64 -> (bound dx, bound dp)
    "phys_74": ((2.85e-4, 2.60e-4), (3.04e-3, 2.81e-3)), "phys_196": ((1.09e-1, 9.63e-2), (5.58e-1, 4.90e-1)),
    "small3_176": ((1.24e-5, 1.25e-5), (3.65e-5, 3.10e-5)),
}

# ---- failed solves ----------------------------------------------------------------------------------------------------
# lin8 = Chain(Dense(8, 8, identity)), B = 5, tol 1e-3, span (0, 100): a linear field whose state overflows float32; the
# error norm becomes NaN (DtNaN, retcode 3) or, where infinite estimates reject until dt underflows, DtLessThanMin (2).
# One launch per attempt, under MAX_ATTEMPTS attempts.  CPU results (oracle over the float32 numpy field / over Chain64):
#   Tsit5 x3: DtNaN after 114 accepted, 0 rejected, with both fields (x6: 112, x12: 110)
#   VCAB3 x3: DtNaN after 763 accepted, 1 rejected; VCABM3 x3: DtNaN after 345 (346 with Chain64)
#   VCAB3 x12: DtLessThanMin after 758 accepted, 13 rejected over the float32 field; DtNaN after 751 over Chain64.
# How x12 was looked at: VCAB3 over both fields at x9, 10, 10.5, .. 14, 15, 16, 18, 20, 24.  The float32 field stops with
# DtLessThanMin at every one of them (751 .. 759 accepted, 7 .. 14 rejected); Chain64 stops with DtNaN at every one: a
# float32 product overflows to infinity where the float64 sum rounded once does not, and an infinite estimate rejects
# where a NaN stops.  No scale gives 2 with both, so x12 stays; the GPU test asserts that the oracle around Handle.rhs
# (float32 products, as the float32 numpy field) stops with 2 there and holds the GPU loop to it.
LIN8 = dict(B=5, tol=1e-3, span=(0.0, 100.0))
LIN8_STOPS = {   # (solver, scale) -> (retcode, naccept, nreject) of the oracle over the float32 numpy field
    ("tsit5", 3.0): (3, 114, 0), ("vcab3", 3.0): (3, 763, 1), ("vcabm3", 3.0): (3, 345, 0), ("vcab3", 12.0): (2, 758, 13),
}
RET_MAXITERS, RET_DT_LESS_THAN_MIN, RET_DT_NAN = 1, 2, 3


def models(P):
    m = dict(K.models(P))
    m["odd130"] = WC.td_chain(P, [130, 257, 131, 130], ["tanh", "tanh", "identity"])
    m["lin8"] = P.Chain(P.Dense(8, 8, "identity"))
    return m


def case(P, name):
    """(model, p, x, tol, span, solver) of a CASES entry"""
    c = CASES[name]
    model = models(P)[c["model"]]
    p, x = K.inputs(P, model, c["B"], c["scale"])
    return model, p, x, c["tol"], c["span"], c["solver"]


def other_batch(P, name):
    """x of the same case at B_OTHER columns (another draw)"""
    c = CASES[name]
    return K.inputs(P, models(P)[c["model"]], B_OTHER, c["scale"], seed=7)[1]


def lin8(P, scale):
    model = models(P)["lin8"]
    p, x = K.inputs(P, model, LIN8["B"], scale)
    return model, p, x


def cpu_fields(model, p):
    """the two CPU fields the cases were picked with: float32 numpy, float64 rounded once"""
    from test_gpu_chain import Chain64
    return K.np_field(model, p), Chain64(model, p)


def cpu_solves(O, model, p, x, span, tol, solver="tsit5", maxiters=10000):
    """the C oracle's solve over both CPU fields"""
    out = []
    with np.errstate(all="ignore"):
        for f in cpu_fields(model, p):
            out.append(O.solve(O.PyField(x.shape[1], f), x, span[0], span[1], tol, tol, saveat=[span[1]], solver=solver,
                               maxiters=maxiters, trace_cap=maxiters + 8))
    return out


def stop_of(r):
    return r["retcode"], r["stats"]["naccept"], r["stats"]["nreject"]


def series_times(span, fractions=SERIES_FRACTIONS):
    return [float(f32(span[0] + fr * (span[1] - span[0]))) for fr in fractions]


def cotangents(n, x, seed=21):
    return np.random.default_rng(seed).standard_normal((n,) + x.shape).astype(f32)


# ---- the float64 yardsticks -------------------------------------------------------------------------------------------
# RK4 steps of reference_grads: the smallest of 100 x 2^k at which halving the count moves both gradients by less than
# 1e-5 of their norm (asserted in the host test).  phys_119: 1600 against 800 moves them by 1.1e-5, 3200 against 1600 by
# 6.5e-7; phys_vcab3_1e-4 (B = 9): 1600 against 800 by 4e-7; odd130_87: 800 against 400 by 3.1e-6; small3_176: 1200 against
# 600 by 7.5e-6.  The references cost up to 10 s of CPU each, so they are kept, rounded to float32, in
# tests/golden/record_growth_refs.npz (written by tests/golden/make_golden.py); the host test recomputes every one and
# holds the file to it, the GPU tests read the file.
RK4_STEPS = {"phys_119": 3200, "phys_vcab3_1e-4": 1600, "odd130_87": 800, "small3_176": 1200}
RK4_CONVERGED = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_growth_refs.npz")

# The distance of chain_adjoint_np.pullback in float32 from the same in float64 (relative, 2-norm), measured on the CPU at
# the inputs of pullback_inputs; the bar of the continuous pullback is max(3e-4, 4 x this).  The host test recomputes both
# restatements (4 s each) and holds these figures to what it finds within a factor 2.
#   phys_119: forward 117 + 4 / 119 + 3 steps, reversed 480 + 4 / 2137 + 1: the float32 restatement's reversed solve is
#   rounding (the chain at weights x3, tolerance 1e-7); the float64 restatement is 5.8e-4 from RK4 autograd, so the
#   project's 3e-4 does not hold for a correct implementation here.
#   odd130_87: 79 / 87 steps forward, 191 / 845 reversed.  small3_176: 168 + 4 / 175 + 4 forward, 453 + 5 / 632 reversed; it
#   is here so that a lookup among more than 128 knots is held to the project's own 3e-4.
PULLBACK_TWINS = {
    "phys_119": dict(dx=1.59e-2, dp=1.61e-2),       # -> bars 6.4e-2
    "odd130_87": dict(dx=5.33e-5, dp=5.50e-5),      # -> 3e-4
    "small3_176": dict(dx=2.67e-5, dp=1.83e-5),     # -> 3e-4
}


def reference_grads(model, p, x, times, cots, span=(0.0, 1.0), nsteps=200):
    """test_gpu_chain.reference_grads (float64 torch autograd through RK4) with a span and a step count; every saved time
    must be a step end"""
    from test_gpu_chain import torch_field
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    f = torch_field(model, pt)
    t0, h = float(span[0]), (float(span[1]) - float(span[0])) / nsteps
    marks = {int(round((float(t) - t0) / h)): i for i, t in enumerate(times)}
    assert len(marks) == len(times) and all(abs(t0 + k * h - float(times[i])) < 1e-6 * h for k, i in marks.items()), (times, nsteps)
    u, loss = xt, 0.0
    for k in range(nsteps):
        t = t0 + k * h
        k1 = f(u, t); k2 = f(u + 0.5 * h * k1, t + 0.5 * h); k3 = f(u + 0.5 * h * k2, t + 0.5 * h); k4 = f(u + h * k3, t + h)
        u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        if k + 1 in marks:
            loss = loss + (u * torch.tensor(cots[marks[k + 1]], dtype=torch.float64)).sum()
    loss.backward()
    return xt.grad.numpy(), pt.grad.numpy()


def pullback_inputs(P, name):
    """(model, p, x, tol, span, series times, cotangents) of the continuous-pullback tests"""
    model, p, x, tol, span, _ = case(P, name)
    times = series_times(span)
    return model, p, x, tol, span, times, cotangents(len(times), x)


@functools.lru_cache(maxsize=None)
def compute_reference(name, nsteps=None):
    """(dx, dp) of float64 autograd through RK4 for a pullback case"""
    import lrnde_amd as P
    model, p, x, _tol, span, _times, cots = pullback_inputs(P, name)
    # the marks of RK4 are the exact fractions; the float32 saved times differ from them by rounding only
    exact = [span[0] + fr * (span[1] - span[0]) for fr in SERIES_FRACTIONS]
    return reference_grads(model, p, x, exact, cots, span, RK4_STEPS[name] if nsteps is None else nsteps)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(dx, dp) of compute_reference(name) as the golden file keeps them"""
    with np.load(GOLDEN) as z:
        return z[name + "/dx"].astype(np.float64), z[name + "/dp"].astype(np.float64)


def write_golden():
    np.savez_compressed(GOLDEN, **{f"{n}/{k}": v.astype(f32) for n in RK4_STEPS for k, v in zip(("dx", "dp"), compute_reference(n))})
    return GOLDEN


@functools.lru_cache(maxsize=None)
def pullback_twins(name):
    """(float64, float32) chain_adjoint_np.pullback at a pullback case's inputs"""
    import chain_adjoint_np as CA
    import lrnde_amd as P
    model, p, x, tol, span, times, cots = pullback_inputs(P, name)
    with np.errstate(all="ignore"):
        r64 = CA.pullback(model, p, x, times, cots, tol, mode="none", t0=span[0], t2=span[1])
        r32 = CA.pullback(model, p, x, times, cots, tol, mode="none", t0=span[0], t2=span[1], dtype=np.float32)
    return r64, r32


def pullback_bars(name):
    """{dx, dp: (bar, twin distance)}: max(3e-4, 4 x PULLBACK_TWINS), chain_discrete_np.bound's form at the project's
    floor for gradients"""
    return {k: (max(3e-4, 4.0 * d), d) for k, d in PULLBACK_TWINS[name].items()}


@functools.lru_cache(maxsize=None)
def solution_twins(name):
    """(float64-field solve, float32-field solve) of np_restatement.solve at a Tsit5 case, computed once"""
    import lrnde_amd as P
    import np_restatement as R
    from test_gpu_chain import Chain32, Chain64
    model, p, x, tol, span, _ = case(P, name)
    with np.errstate(all="ignore"):
        return (R.solve(Chain64(model, p), x, span[0], span[1], tol, tol), R.solve(Chain32(model, p), x, span[0], span[1], tol, tol))


def solution_bar(name):
    """(bar, twin distance): test_solve_counts_equal_where_truncation_dominates's rule"""
    from test_gpu_chain import err
    r64, r32 = solution_twins(name)
    d = err(r32["u"], r64["u"])
    return max(1e-5, 0.5 * CASES[name]["tol"], 4.0 * d), d


# ---- the Latent-ODE training step past the record ----------------------------------------------------------------------
# latent_cases.TINY with the node weights x3 (make_node_params at scale 3) and tolerance 1e-7.  On the CPU, from the z0 of
# the encoder's host restatement (tests/latent_host.cpp) with the model's own eps draw: 242 / 224 accepted steps over the
# float32 / float64 field, two doublings.  (At scale 4.5 the solve takes 3000 steps.)
LATENT = dict(B=9, T=4, times=[0.25, 0.5, 0.75, 1.0], tol=1e-7, node_scale=3.0, line=128, counts=(242, 224))


def latent_inputs(P):
    """(dims, model factory, flat, node, (data, mask, dt)) of the training-step test: tests/test_gpu_chain_adams.py's
    inputs with the node weights x3"""
    import latent_cases as LC
    c = LATENT
    dims = LC.TINY
    make = lambda: P.construct_time_series(*dims, saveat=c["times"], regularize="unbiased", abstol=c["tol"], reltol=c["tol"],
                                           maxiters=10000)
    flat, node = LC.make_params(dims, seed=11), LC.make_node_params(dims, seed=12, scale=c["node_scale"])
    data, mask, dt = LC.make_batch(dims, c["B"], c["T"], seed=13, unobserved_column=False)
    mask[:, 0, 0] = 1
    return dims, make, flat, node, (data, mask, dt)
