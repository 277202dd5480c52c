"""The yardstick of the conv handle's discrete adjoint (lrnde_conv_set_sensealg(LRNDE_SENSE_DISCRETE),
csrc/lrnde_conv_discrete.hpp) that tests/test_host_conv_discrete.py and tests/test_gpu_conv_discrete.py use.  Nothing here
is the project's own C and nothing needs a GPU: frozen_grads is torch autograd through Tsit5 steps on a GIVEN grid
(t_n, dt_n) — the times and step sizes are constants, there is no controller and no rejected attempt, k1 of a step is k7 of
the step before — over torch_field of tests/conv_geometry_cases.py with the tableau NP.A / NP.C of
oracle/np_restatement.py, loss <w, u_end>, inputs case_inputs of tests/conv_pullback_cases.py.

Distances are per quantity (dx and the five parameter blocks, distances() of conv_pullback_cases).  The bar of a quantity
is max(5e-5, 4 x d32): d32 is the distance of the float32 run of this restatement from its float64 run on the same grid —
what fp32 arithmetic in another order costs the yardstick itself — and the floor and the factor are conv_pullback_cases'.
The host test caps d32 at 2.5e-3 (that module's CAP) at every case used on the GPU."""
import functools

import numpy as np
import torch

import conv_geometry_cases as G
import conv_pullback_cases as K
import np_restatement as NP

# the rows of conv_pullback_cases the GPU test runs against the yardstick (modes none, unbiased t1 0.41, biased)
YARDSTICK_CASES = ("8x8", "8x8-test", "16x16-tanh", "12x3", "4x2-train", "20x7-identity")
# a forward solve that rejects an attempt (the discrete adjoint must not see it): the oracle accepts 21 steps and rejects
# one, whose EEst is 1.34 while no accepted step's is above 0.29, so a last-bit difference does not flip a decision.  Found
# by a search over activation, statistics mode, seed (40..59), scale (2, 3, 4) and tolerance (1e-3 .. 1e-5) at 4x2, B = 3:
# no forward of K's rows rejects (4x2-reject rejects in its adjoint only), none with batch statistics or tanh did; running
# statistics, gelu and a trajectory that grows (max |u_end| 95) do.  tests/test_host_conv_discrete.py asserts the counts.
REJECT = K.LayerCase("4x2-fwd-reject", 4, 2, 3, "gelu", False, 52, 3.0, 1e-5, 64)
MODES = (("none", K.T1), ("unbiased", K.T1), ("biased", K.T1))
REG_CASE = "8x8-reg"             # zero cotangent, w_reg = 1: the regulariser alone (a row of K.REG_LAYER_CASES)
SHARDED_CASE = "8x8"             # 2 and 3 ranks: a global batch of 6 built from this row's recipe
CS = (NP.C[0], NP.C[1], NP.C[2], NP.C[3], 1.0, 1.0)


def as_grid(t, dt):
    """a hashable grid: (tuple of t_n, tuple of dt_n) as float32 values"""
    return tuple(float(np.float32(v)) for v in t), tuple(float(np.float32(v)) for v in dt)


def oracle_grid(case, maxiters=K.MAXITERS):
    """(grid of the accepted steps, the oracle's solve result) of the oracle's traced forward solve of a case"""
    import oracle as O
    p, u, st, _w = K.case_inputs(case)
    sol = O.solve(G.oracle_field(case.W, case.H, p, case.act, case.train, st), u.reshape(case.B, -1), K.T0, K.T2, case.tol, case.tol,
                  saveat=[K.T2], maxiters=maxiters)
    assert sol["retcode"] == 0
    tr = sol["trace"]
    acc = tr[tr["accepted"] != 0]
    return as_grid(acc["t"], acc["dt"]), sol


def _stage_time(t, c, dt):
    """t + c * dt formed in fp32, as the forward forms it (the times are constants of the frozen grid)"""
    return float(np.float32(t) + np.float32(c) * np.float32(dt))


def _frozen(inputs, case, grid, dtype):
    p, u, st, w = inputs
    B = u.shape[0]
    x = torch.tensor(np.asarray(u, dtype=np.float64).reshape(B, -1), dtype=dtype, requires_grad=True)
    pt = torch.tensor(np.asarray(p, dtype=np.float64), dtype=dtype, requires_grad=True)

    def f(y, t):
        return G.torch_field(y, pt, t, case.W, case.H, case.act, case.train, st)

    ts, dts = grid
    y = x
    k1 = f(x, float(np.float32(ts[0])))
    for tn, dn in zip(ts, dts):
        ks = [k1]
        xs = None
        for s in range(2, 8):
            acc = sum(a * k for a, k in zip(NP.A[s], ks))
            xs = y + float(dn) * acc
            ks.append(f(xs, _stage_time(tn, CS[s - 2], dn)))
        y, k1 = xs, ks[6]          # a_7. are the solution weights: the stage-7 input is u_{n+1}; first same as last
    (y * torch.tensor(np.asarray(w, dtype=np.float64).reshape(B, -1), dtype=dtype)).sum().backward()
    out = (y.detach().double().numpy().reshape(u.shape), x.grad.double().numpy().reshape(u.shape), pt.grad.double().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frozen_grads(case, grid, dtype=torch.float64):
    """(u_end, dx, dp) as read-only float64 arrays: autograd of <w, u_end> through the Tsit5 steps of `grid` run in `dtype`"""
    return _frozen(K.case_inputs(case), case, grid, dtype)


def frozen_grads_inputs(inputs, case, grid, dtype=torch.float64):
    """frozen_grads for explicit (p, u, st, w) (the sharded test's global batch); `case` gives W, H, act, train"""
    return _frozen(inputs, case, grid, dtype)


@functools.lru_cache(maxsize=None)
def d32(case, grid):
    """{quantity: distance of the float32 run from the float64 run on the same grid}"""
    _u64, dx64, dp64 = frozen_grads(case, grid, torch.float64)
    _u32, dx32, dp32 = frozen_grads(case, grid, torch.float32)
    return K.distances(dx32, dp32, dx64, dp64)


def bars_from(d):
    return {k: max(K.FLOOR, K.FACTOR * v) for k, v in d.items()}


def bars(case, grid):
    """({quantity: max(5e-5, 4 x d32)}, d32)"""
    d = d32(case, grid)
    return bars_from(d), d
