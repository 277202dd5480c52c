"""Host side of the Dense-chain VCAB3 / VCABM3 solvers: what the NeuralODE constructor accepts, the solver names, and the
branch coverage of the GPU cases (tests/chain_adams_cases.py) re-derived on the CPU with the oracle's adams_solve over the
float32 numpy field — a warning that the cases drifted before anyone spends a GPU run on them.  No GPU needed."""
import numpy as np
import pytest

import chain_adams_cases as K


def test_solver_names_round_trip():
    import lrnde_amd  # noqa: F401  (registers the package under its importable name)
    from localregneuralde_jl_amd.layers import SOLVERS, _solver_name
    assert SOLVERS == {"tsit5": 0, "vcab3": 1, "vcabm3": 2}
    for name, spellings in {"tsit5": ("Tsit5", "tsit5", "Tsit5()"), "vcab3": ("VCAB3", "vcab3", "VCAB3()"),
                            "vcabm3": ("VCABM3", "vcabm3", " VCABM3() ")}.items():
        for s in spellings:
            assert _solver_name(s) == name and _solver_name(_solver_name(s)) == name
    with pytest.raises(ValueError):
        _solver_name("rk4")


def test_constructor_matrix():
    """The layer object's `solver` keyword stays closed for the chain fields (tests/test_host_chain.py and
    tests/test_host_wide_chain.py pin that): it raises, and for field="dense_chain" the message names the route that is
    open, the handle's own setter.  Everything else constructs as before."""
    import lrnde_amd as P
    small = K.models(P)["physionet"]
    for field in ("dense_chain", "wide_chain"):
        for solver in ("Tsit5", "tsit5", "Tsit5()"):
            assert P.NeuralODE(small, field=field, solver=solver, saveat=[0.5, 1.0]).solver == "tsit5"
        for solver in ("vcab3", "vcabm3", "VCAB3()"):
            with pytest.raises(NotImplementedError, match=r"handle\(\)\.set_solver" if field == "dense_chain" else "Tsit5 only"):
                P.NeuralODE(small, field=field, solver=solver)
        with pytest.raises(ValueError):
            P.NeuralODE(small, field=field, solver="rk4")
    with pytest.raises(NotImplementedError):
        P.construct_time_series(3, 5, 3, 2, saveat=[0.5, 1.0], solver="vcabm3")
    assert P.construct_time_series(3, 5, 3, 2, saveat=[0.5, 1.0]).neural_ode.solver == "tsit5"
    # both discrete adjoints construct with Tsit5, as before
    assert P.NeuralODE(small, field="dense_chain", sensealg="TrackerAdjoint").sense == "discrete"
    assert P.NeuralODE(small, field="wide_chain", adjoint_loop="discrete").adjoint_loop == "discrete"
    # the MLP field takes the keyword, the conv field keeps Tsit5
    mlp = P.TDChain(P.Chain(P.Dense(5, 8, "tanh"), P.Dense(9, 4)))
    assert P.NeuralODE(mlp, solver="VCABM3()").solver == "vcabm3"
    conv = P.TDChain(P.Chain(P.Chain(P.Conv((3, 3), 9, 64), P.BatchNorm(64, "gelu")), P.Chain(P.Conv((3, 3), 65, 64), P.BatchNorm(64, "gelu")),
                             P.Conv((3, 3), 65, 8)))
    with pytest.raises(NotImplementedError):
        P.NeuralODE(conv, solver="vcab3")


@pytest.mark.parametrize("solver", K.SOLVERS)
def test_the_gpu_cases_reach_every_branch_on_the_cpu(oracle, solver):
    import lrnde_amd as P
    cov = {}
    for name in K.CASES:
        model, p, x, tol = K.case(P, name)
        fld = oracle.PyField(x.shape[1], K.np_field(model, p))
        r = oracle.solve(fld, x, 0.0, 1.0, tol, tol, saveat=K.SAVEAT, save_start=True, solver=solver)
        assert r["retcode"] == 0 and list(r["t"]) == [np.float32(s) for s in K.SAVEAT]
        cov[name] = K.coverage(r["trace"])
        assert cov[name]["attempts"] <= K.MAX_ATTEMPTS, (name, cov[name])
    print(solver, cov)
    assert sum(c["multistep_rejects"] for c in cov.values()) >= 1
    assert sum(c["startup_rejects"] for c in cov.values()) >= 1
    assert any(c["two_then_none"] for c in cov.values())
    # the case made for the start-up rejection still has one, with margin
    assert cov["td_kick"]["startup_rejects"] >= 1
