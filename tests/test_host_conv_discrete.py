"""The conv handle's discrete adjoint, the part that needs no GPU (tests/conv_discrete_cases.py holds the yardstick):
the frozen-grid restatement is tied to the independent C of the oracle (its float64 forward on the oracle's accepted grid
reproduces the oracle's u_end), the float32 run of the restatement stays within the cap of its float64 run at every case
the GPU test uses, the rejecting case rejects in the oracle's FORWARD solve, the two entry points are declared, bound and
called from Julia, and the layer keyword routes.

Measured here (worst quantity of d32 / distance of the float64 forward from the oracle's u_end, of its scale):
8x8 1.6e-6 / 1.6e-6, 8x8-test 1.7e-6 / 1.4e-6, 16x16-tanh 1.9e-6 / 9.8e-7, 12x3 1.3e-6 / 1.4e-6, 4x2-train 1.2e-6 / 8.4e-7,
20x7-identity 1.2e-6 / 1.1e-6, 4x2-fwd-reject (21 accepted, 1 rejected at EEst 1.34) 1.8e-6 / 7.3e-7: every bar sits at its
floor of 5e-5."""
import inspect
import os
import re

import numpy as np
import pytest

import conv_discrete_cases as D
import conv_pullback_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [pytest.param(K.CASE[n], id=n) for n in D.YARDSTICK_CASES] + [pytest.param(D.REJECT, id=D.REJECT.name)]


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_reproduces_the_oracle_forward_and_its_f32_run_is_within_the_cap(oracle, case):
    grid, sol = D.oracle_grid(case)
    assert len(grid[0]) == sol["stats"]["naccept"] >= 1
    u_end, _dx, _dp = D.frozen_grads(case, grid)
    ref = sol["u"][-1].reshape(-1).astype(np.float64)
    dist = float(np.abs(u_end.reshape(-1) - ref).max() / np.abs(ref).max())
    d = D.d32(case, grid)
    print(f"{case.name}: {len(grid[0])} steps, {sol['stats']['nreject']} rejected; u_end {dist:.1e} of scale; d32 {K.fmt(d)}")
    assert dist <= 1e-5, f"{case.name}: the float64 restatement is {dist:.2e} of scale from the oracle's u_end"
    for name, v in d.items():
        assert np.isfinite(v) and v <= K.CAP, f"{case.name}: d32 of {name} is {v:.2e} > {K.CAP:.1e}"


def test_the_rejecting_case_rejects_in_the_oracle_forward(oracle):
    grid, sol = D.oracle_grid(D.REJECT)
    tr = sol["trace"]
    assert sol["stats"]["nreject"] >= 1 and int((tr["accepted"] == 0).sum()) == sol["stats"]["nreject"]
    assert len(grid[0]) == sol["stats"]["naccept"] == int((tr["accepted"] != 0).sum())
    # no decision near the threshold: another f-eval implementation takes the same grid
    assert float(tr["eest"][tr["accepted"] == 0].min()) > 1.05 and float(tr["eest"][tr["accepted"] != 0].max()) < 0.95
    # the grid is the accepted rows: contiguous in time, ending at t2
    t, dt = np.array(grid[0], np.float32), np.array(grid[1], np.float32)
    assert t[0] == np.float32(K.T0) and np.all(np.abs((t[:-1] + dt[:-1]) - t[1:]) <= 2e-7) and abs(float(t[-1] + dt[-1]) - K.T2) <= 2e-7


def test_twelve_by_three_takes_six_or_more_steps(oracle):
    grid, _sol = D.oracle_grid(K.CASE["12x3"])
    assert len(grid[0]) >= 6


def test_the_entry_points_are_declared_bound_and_called_from_julia():
    import lrnde_amd  # noqa: F401  (registers the package under its importable name)
    from localregneuralde_jl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    jl = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    for name, nargs in (("lrnde_conv_set_sensealg", 2), ("lrnde_conv_record_steps", 5)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/lrnde.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert name in bound and len(bound[name]) == nargs and hasattr(_lib.lib, name)
        call = re.search(r"ccall\(\(:" + name + r", lib\), Cint,\s*\((.*?)\),\n?", jl)
        assert call and len([t for t in call.group(1).split(",") if t.strip()]) == nargs, name
    layer = open(os.path.join(ROOT, "julia", "LRNDELayer.jl")).read()
    assert "conv_set_sensealg!(cctx, _lrnde_sense(n.sensealg))" in layer
    src = open(os.path.join(ROOT, "localregneuralde.jl_amd", "csrc", "lrnde_conv.hip")).read()
    assert '#include "lrnde_conv_discrete.hpp"' in src


def _conv_model(P):
    return P.TDChain(P.Chain(P.Chain(P.Conv((3, 3), 9, 64), P.BatchNorm(64, "gelu")), P.Chain(P.Conv((3, 3), 65, 64), P.BatchNorm(64, "gelu")),
                             P.Conv((3, 3), 65, 8)))


def test_the_layer_keyword_routes_and_the_pins_hold():
    import lrnde_amd as P
    from localregneuralde_jl_amd.conv import ConvHandle
    from localregneuralde_jl_amd.layers import Handle
    conv = _conv_model(P)
    for s in ("TrackerAdjoint", "ReverseDiffAdjoint", "discrete", "TrackerAdjoint()"):
        assert P.NeuralODE(conv, sensealg=s).sense == "discrete"
    for s in (None, "InterpolatingAdjoint"):
        assert P.NeuralODE(conv, sensealg=s).sense == "interpolating"
    with pytest.raises(ValueError):
        P.NeuralODE(conv, sensealg="BacksolveAdjoint")
    # the conv topology is recognised by field="auto" alone; the other fields and the MLP keep their refusals
    for field in ("wide_chain",):
        with pytest.raises(NotImplementedError):
            P.NeuralODE(P.Chain(P.Dense(8, 16, "tanh"), P.Dense(16, 8)), sensealg="TrackerAdjoint", field=field)
    mlp = P.TDChain(P.Chain(P.Dense(785, 100, "tanh"), P.Dense(101, 784)))
    with pytest.raises(NotImplementedError):
        P.NeuralODE(mlp, sensealg="TrackerAdjoint")
    with pytest.raises(NotImplementedError):
        P.NeuralODE(conv, adjoint_loop="discrete")
    assert callable(ConvHandle.set_sensealg) and callable(ConvHandle.record_steps)
    assert ConvHandle.SENSEALGS == {"interpolating": 0, "discrete": 1}
    assert len(Handle.ADJOINT_LOOP_NAMES) == 6 and "conv_discrete" not in Handle.ADJOINT_LOOP_NAMES
    doc = inspect.getdoc(P.NeuralODE.pullback)
    for name in ('"host"', '"device"', '"chain_device"', '"wide_device"', '"chain_discrete"', '"wide_discrete"', '"conv_discrete"'):
        assert name in doc
