"""VCAB3 / VCABM3 on the conv handle, the part that needs no GPU: the cases of tests/conv_adams_cases.py re-derived with the
oracle's ConvField (so a drifted seed or recipe cannot silently turn a case into another one before anyone spends a GPU run
on it), the C ABI entry's declaration / binding / Julia call, and the layer keyword."""
import os
import re

import numpy as np
import pytest

import conv_adams_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REFS = {}


def ref(oracle, name, solver):
    """the oracle's solve of a case with its own conv f-evals, computed once"""
    if (name, solver) not in _REFS:
        c = K.CASES[name] if name in K.CASES else K.PULLBACK
        fld, u = K.oracle_field(c)
        r = oracle.solve(fld, u, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True, solver=solver)
        _REFS[(name, solver)] = (r, K.coverage(r["trace"]))
    return _REFS[(name, solver)]


@pytest.mark.parametrize("solver", K.SOLVERS)
@pytest.mark.parametrize("name", list(K.CASES))
def test_every_case_ends_ok_within_the_attempt_budget(oracle, name, solver):
    r, cov = ref(oracle, name, solver)
    print(name, solver, r["stats"], cov)
    assert r["retcode"] == 0 and r["stats"]["t_final"] == np.float32(1.0)
    assert cov["attempts"] <= K.MAX_ATTEMPTS
    assert cov["max_points_in_a_step"] >= 2          # an accepted step carrying two saveat points (the duplicate)
    assert list(r["t"]) == [np.float32(s) for s in K.SAVEAT]


def test_the_listed_counts_of_the_plain_cases(oracle):
    """what the issue's table states for the two plain cases"""
    for name, solver, nf, steps in (("plain16", "vcab3", 30, 23), ("plain16", "vcabm3", 39, 17), ("plain8", "vcab3", 26, None),
                                    ("plain8", "vcabm3", 33, None)):
        r, cov = ref(oracle, name, solver)
        assert r["stats"]["nf"] == nf and r["stats"]["nreject"] == 0
        assert steps is None or r["stats"]["naccept"] == steps


@pytest.mark.parametrize("solver", K.SOLVERS)
def test_the_rejecting_cases_reject_a_multistep_attempt(oracle, solver):
    for name in K.MULTISTEP_REJECTS[solver]:
        r, cov = ref(oracle, name, solver)
        assert cov["multistep_rejects"] >= 1 and r["stats"]["nreject"] >= 1, (name, cov)


@pytest.mark.parametrize("solver", K.SOLVERS)
def test_the_kick_case_rejects_a_startup_attempt(oracle, solver):
    r, cov = ref(oracle, "kick", solver)
    assert cov["startup_rejects"] >= 1 and min(cov["rejected_at"]) < 2, cov


@pytest.mark.parametrize("solver", K.SOLVERS)
@pytest.mark.parametrize("name", K.ORACLE_CASES + ("pullback",))
def test_no_attempt_of_an_oracle_compared_case_is_near_the_threshold(oracle, name, solver):
    """equal accept patterns across two f-eval implementations are asserted only where no EEst lies within 5 % of 1"""
    r, cov = ref(oracle, name, solver)
    assert cov["margin"] >= 0.05, (name, solver, cov)


def test_the_setter_is_declared_bound_and_called_from_julia():
    from localregneuralde_jl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    m = re.search(r"int\s+lrnde_conv_set_solver\s*\(([^)]*)\)\s*;", hdr)
    assert m, "lrnde_conv_set_solver is not declared in include/lrnde.h"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert "lrnde_conv_set_solver" in bound and len(bound["lrnde_conv_set_solver"]) == nargs == 2
    assert hasattr(_lib.lib, "lrnde_conv_set_solver")
    jl = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    assert "UNTESTED" in jl
    call = re.search(r"ccall\(\(:lrnde_conv_set_solver, lib\), Cint,\s*\((.*?)\),", jl)
    assert call and len([t for t in call.group(1).split(",") if t.strip()]) == nargs
    assert "the conv handle has no such setter" not in hdr


def test_the_layer_keyword_stays_closed_and_names_the_handle_setter():
    import lrnde_amd as P
    conv = P.TDChain(P.Chain(P.Chain(P.Conv((3, 3), 9, 64), P.BatchNorm(64, "gelu")), P.Chain(P.Conv((3, 3), 65, 64), P.BatchNorm(64, "gelu")),
                             P.Conv((3, 3), 65, 8)))
    P.NeuralODE(conv, solver="Tsit5")
    for s in ("vcab3", "VCABM3()"):
        with pytest.raises(NotImplementedError, match=r"handle\(x\)\.set_solver"):
            P.NeuralODE(conv, solver=s)
    with pytest.raises(ValueError):
        P.NeuralODE(conv, solver="rk4")
    from localregneuralde_jl_amd.conv import ConvHandle
    assert callable(ConvHandle.set_solver)
