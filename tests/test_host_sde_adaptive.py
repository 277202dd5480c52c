"""The adaptive NeuralDSDE layer with the Milstein and four-stage SRI steps — CPU side.

* tests/sde_adaptive_np.py (the loop of oracle.sde_node_forward with the step as a parameter) run with the Euler-Heun step equals
  oracle.sde_node_forward bit for bit in every field: the helper the GPU suite compares with is pinned to the committed oracle.
* CASES: the pinned inputs of tests/test_gpu_sde_adaptive_alg.py, chosen here with the helper alone.  Every case ends with
  retcode OK (the helper raises otherwise) and at least three accepted steps in all three modes; for each of Milstein and SRI at
  least one case rejects a step.  With the controller's growth limit qmax = 1.125 and the automatic initial dt no case of
  these sizes rejects on its own (the proposal creeps up on the tolerance), so the rejecting cases start from an explicit,
  too long first step dt0: the controller has to come down the path's grid before it can go on.
  Milstein's EEst is the reference's four-argument residual — the step's own size against the tolerance (src/perform_step.jl:
  166-169) — so its tolerances are of order one: a little below 0.5 a single grid interval of these fields is refused and the
  loop ends DtLessThanMin, and long steps pass again because the residual's scale grows with |u_new|.
* the constructor accepts solver="RKMil" / "SRI" with adaptive=True; the defaults of `adaptive` are what they were."""
import numpy as np
import pytest

import sde_adaptive_np as S

f32 = np.float32
MODES = ("unbiased", "biased", "none")

# kind, (D, H, B, nfine), seed, tol, dt0 (0: automatic), tableau (SRI: seed and scale of S.sri_tableau)
CASES = [
    dict(kind="RKMil", shape=(32, 64, 40, 64), seed=7, tol=0.8, dt0=0.0),     # config-5 widths, partial last 16-column tile
    dict(kind="RKMil", shape=(2, 4, 1, 64), seed=7, tol=1.0, dt0=0.0),        # one column
    dict(kind="RKMil", shape=(33, 100, 9, 32), seed=7, tol=1.5, dt0=0.0),     # odd widths, padded fragments
    dict(kind="RKMil", shape=(64, 128, 17, 32), seed=7, tol=1.5, dt0=0.0),    # the gate's corner, two 112-row segments
    dict(kind="RKMil", shape=(72, 32, 6, 32), seed=7, tol=1.5, dt0=0.0),      # outside the gate: generic kernel and host loop
    dict(kind="RKMil", shape=(32, 64, 40, 64), seed=8, tol=0.56, dt0=1.0),    # a rejection (the GPU suite runs it on both loops)
    dict(kind="SRI", shape=(32, 64, 24, 64), seed=7, tol=0.14, dt0=0.0, tab=(41, 0.1)),
    dict(kind="SRI", shape=(20, 48, 7, 32), seed=7, tol=0.5, dt0=0.0, tab=(41, 0.1)),
    dict(kind="SRI", shape=(32, 64, 24, 64), seed=8, tol=0.14, dt0=0.4, tab=(41, 0.1)),   # rejections
]


def case_id(c):
    return "%s-%dx%dx%d-n%d-s%d%s" % ((c["kind"],) + c["shape"] + (c["seed"], "-dt0" if c["dt0"] else ""))


def case_reference(O, c, mode, **kw):
    """the helper's result for a case: (inputs, tableau, result dict)"""
    D, H, B, nfine = c["shape"]
    inp = S.case_inputs(D, H, B, nfine, c["seed"], second_path=c["kind"] == "SRI")
    drift, diff = S.oracle_fields(O, D, H, inp["pd"], inp["pg"])
    T = S.sri_tableau(O, *c["tab"]) if c["kind"] == "SRI" else None
    args = dict(mode=mode, t1_or_rand=0.43, z_local=inp["z"], dt0=c["dt0"], tableau=T, Z=inp["Z"], z2_local=inp["z2"])
    args.update(kw)
    return inp, T, S.sde_node_forward(O, c["kind"], drift, diff, inp["x"], inp["W"], 0.0, 1.0, c["tol"], c["tol"], **args)


@pytest.mark.parametrize("D,H,B,tol,nfine", [(32, 64, 40, 0.02, 256), (2, 4, 1, 0.05, 64)])
@pytest.mark.parametrize("mode", MODES)
def test_helper_with_the_euler_heun_step_is_the_oracle_loop(oracle, D, H, B, tol, nfine, mode):
    inp = S.case_inputs(D, H, B, nfine, 7)
    drift, diff = S.oracle_fields(oracle, D, H, inp["pd"], inp["pg"])
    kw = dict(mode=mode, t1_or_rand=0.43, z_local=inp["z"])
    a = S.sde_node_forward(oracle, "EulerHeun", drift, diff, inp["x"], inp["W"], 0.0, 1.0, tol, tol, **kw)
    b = oracle.sde_node_forward(drift, diff, inp["x"], inp["W"], 0.0, 1.0, tol, tol, **kw)
    assert a["dZ_local"] is None and set(a) == set(b) | {"dZ_local"}
    for k, vb in b.items():
        va = a[k]
        if vb is None:
            assert va is None, k
        elif isinstance(vb, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape and np.array_equal(va, vb), k
        elif k in ("steps", "series"):
            assert len(va) == len(vb) and all(tuple(x) == tuple(y) for x, y in zip(va, vb)), k
        else:
            assert type(va) is type(vb) and va == vb, (k, va, vb)
    assert b["naccept"] >= 3


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_pinned_cases_end_ok_with_three_accepted_steps_in_every_mode(oracle, c):
    nf, ng = S.KINDS[c["kind"]]["nf"], S.KINDS[c["kind"]]["ng"]
    for mode in MODES:
        _, _, r = case_reference(oracle, c, mode)     # (raises on MaxIters / DtLessThanMin / DtNaN)
        assert r["naccept"] >= 3, (mode, r["naccept"])
        assert np.isfinite(r["u"]).all() and (r["reg_val"] > 0) == (mode != "none")
        att = r["naccept"] + r["nreject"]
        init = 0 if c["dt0"] else 2
        loc = 0 if mode == "none" else 1
        assert r["nfe_drift"] == nf * (att + loc) + init * (1 + loc) and r["nfe_diffusion"] == ng * (att + loc) + init * (1 + loc)
        assert sum(m for _, m in r["steps"]) == c["shape"][3]     # the accepted steps tile the path's grid
        if c["dt0"]:
            assert r["nreject"] >= 1
        print(f"{case_id(c)} {mode}: accepted {r['naccept']}, rejected {r['nreject']}, dt0 {r['dt0']:.4g}, reg_val {r['reg_val']:.4g}")


@pytest.mark.parametrize("kind", ["RKMil", "SRI"])
def test_each_new_kind_has_a_case_that_rejects(oracle, kind):
    rej = [case_reference(oracle, c, "none")[2]["nreject"] for c in CASES if c["kind"] == kind]
    assert len(rej) >= 2 and max(rej) >= 1, rej


def _layer(**kw):
    import lrnde_amd as P
    return P.NeuralDSDE(P.Chain(P.Dense(4, 8, "tanh"), P.Dense(8, 4)), P.Dense(4, 4), **kw)


def test_constructor_accepts_the_adaptive_milstein_and_sri_layers():
    import oracle as O
    T = S.sri_tableau(O, 41, 0.1)
    mil = _layer(solver="RKMil", adaptive=True)
    assert mil.adaptive and mil.solver == "RKMil"
    assert _layer(solver="RKMilCommute", adaptive=True).solver == "RKMil"
    sri = _layer(solver="SRI", tableau=T, adaptive=True)
    assert sri.adaptive and sri.solver == "SRI" and sri.tableau is T
    with pytest.raises(ValueError):
        _layer(solver="SRI", adaptive=True)
    with pytest.raises(NotImplementedError):
        _layer(solver="SOSRI", adaptive=True)


def test_adaptive_defaults_are_unchanged():
    import oracle as O
    T = S.sri_tableau(O, 41, 0.1)
    assert _layer().adaptive and _layer(solver="EulerHeun").adaptive and _layer(solver="LambaEulerHeun").adaptive
    assert not _layer(solver="RKMil").adaptive and not _layer(solver="SRI", tableau=T).adaptive
    assert not _layer(adaptive=False).adaptive
    assert _layer(noise_source="device").noise_source == "device"
