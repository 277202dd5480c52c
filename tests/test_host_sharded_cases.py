"""CPU side of the sharded-handle tests (tests/test_gpu_sharded_paths.py): what has to hold of the inputs and of the
yardsticks before a GPU result may be held to them.  No GPU needed.

- the float64 restatement of the pullback (tests/chain_adjoint_np.py) states the MLP handle's field: against the oracle's;
- the row-checked inputs (sharded_cases.TS_CASES, rows = "restatement") meet chain_adjoint_np.PINNED's selection
  conditions: (1) the float64 and the float32 restatement take the same steps, (2) the mixed twins pass check_rows — here
  within sharded_cases.ROW_MARGIN of its bounds, and so do the oracle's reversed solve (ORACLE_MARGIN) and the restatements
  with the parameter cotangent regrouped by rank; the reject cases reject directly after the impulse; (3) the float64
  restatement is near enough to float64 RK4 autograd for the 3e-4 bar to be met through it;
- the rank-order float32 sum of the oracle's per-shard parameter cotangents is a yardstick of its own: the per-shard dy
  rows are the global rows bit for bit, the summed gp is NOT the global gp's bits;
- the Adams rejecting case rejects in the oracle;
- on the regulariser test's :biased inputs the reversed solve's step count scatters among correct implementations, which
  is why that test prints the sharded adjoint's steps and does not compare them.

Dropped from the row check: all ten seed-0, scale-3 inputs first proposed for it (Q and V1 at B = 21 and 34, V4 at B = 21,
plain and with the x1000 impulse).  They meet condition (1) and fail condition (2): a mixed twin leaves check_rows' bound in
dt, EEst or s at attempts 2..11 (Q-21: dt of attempt 2 off by 1.3 % against a bound of 0.8 %; V1-21: EEst of attempt 9 off
by 7 % against 6 %), i.e. on those inputs 4 x |row32 - row64| says nothing about a third implementation.  No floor was
widened: the ten stay in the GPU test for everything but the row check (their trace is held to the unsharded handle's), and
ten other inputs of the same shapes and rank layouts, found on the CPU over seeds 0..159 and scales 3, 3.5 and 4, take their
place in the row check."""
import numpy as np
import pytest

import sharded_cases as SC


@pytest.fixture(scope="module")
def P():
    import lrnde_amd
    return lrnde_amd


@pytest.mark.parametrize("shape", list(SC.SHAPES))
def test_restatement_field_is_the_mlp_handles_field(oracle, P, shape):
    """CA.Field (float64, rounded once) vs oracle.MlpField.rhs on the MLP handle's parameter vector: measured rel
    1-2e-7 on the three shapes; the bar is BASELINE's fp32 1e-5 — a wrong parameter layout would be O(1)"""
    import chain_adjoint_np as CA
    D, H = SC.SHAPES[shape]
    model, p, x = SC.inputs(P, shape, 21, scale=SC.TS_SCALE)
    fld = oracle.MlpField(D, H, p, nthreads=4)
    d = SC.rel(CA.Field(model, p)(x, 0.3), fld.rhs(x, 0.3))
    lam = np.random.default_rng(9).standard_normal(x.shape).astype(np.float32)
    dy, gp = CA.Field(model, p).vjp(x, 0.3, lam)
    dyo, gpo = oracle.mlp_vjp(fld, x, 0.3, lam)
    print(f"{shape}: restatement vs oracle rhs {d:.2e} dy {SC.rel(dy, dyo):.2e} gp {SC.rel(gp, gpo):.2e}")
    assert d < 1e-5 and SC.rel(dy, dyo) < 1e-5 and SC.rel(gp, gpo) < 1e-5


@pytest.mark.parametrize("name", [n for n, c in SC.TS_CASES.items() if c["counts"] is not None])
def test_timeseries_inputs_meet_their_selection_conditions(oracle, P, monkeypatch, name):
    """conditions (1) and (3) for every time-series input with pinned counts; for those the GPU row-checks (rows =
    "restatement") condition (2) in the three forms of sharded_cases (mixed twins, the oracle, the rank-regrouped twins), and
    the reject cases reject directly after the impulse"""
    import chain_adjoint_np as CA
    c = SC.TS_CASES[name]
    model, p, x, times, cots, tol = SC.ts_case_inputs(P, name)
    r64 = CA.pullback(model, p, x, times, cots, tol)
    r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32)
    print(f"{name}: float64 {r64['counts']} float32 {r32['counts']} forward {r64['fwd']} / {r32['fwd']}; "
          f"rel(float32, float64) dx {SC.rel(r32['dx'], r64['dx']):.2e} dp {SC.rel(r32['dp'], r64['dp']):.2e}")
    # (1) the decisions are truncation, not rounding
    assert r64["counts"] == r32["counts"] == c["counts"] and r64["fwd"] == r32["fwd"]
    assert [q[3] for q in r64["rows"]] == [q[3] for q in r32["rows"]]
    assert r64["counts"][2] == 3 + 6 * (r64["counts"][0] + r64["counts"][1]) + sum(1 for t in times if 0.0 < t < 1.0)
    assert (r64["counts"][1] >= 1) == bool(c.get("rejects"))
    if c.get("rejects"):   # the first attempt from the impulse time is rejected
        s_imp = -float(np.float32(times[c["big"][0]]))
        after = [q for q in r64["rows"] if q[0] == s_imp]
        assert len(after) >= 2 and after[0][3] == 0, after
    # (3) the RK4 bar can be met: the restatement's distance to float64 autograd + the bound the GPU is held to against it
    from test_gpu_timeseries_pullback import _reference_grads
    D, H = SC.SHAPES[c["shape"]]
    gx, gp = _reference_grads(p, x, D, H, times, cots)
    tot = max(SC.rel(r64[k], g) + max(1e-5, 4.0 * SC.rel(r32[k], r64[k])) for k, g in (("dx", gx), ("dp", gp)))
    print(f"{name}: restatement vs RK4 autograd dx {SC.rel(r64['dx'], gx):.2e} dp {SC.rel(r64['dp'], gp):.2e}; with the bound {tot:.2e}")
    assert tot <= 3e-4
    if c["rows"] != "restatement":
        return
    # (2a) the yardstick is self-consistent, with room for a third implementation
    for tag, kw in (("float32 field, float64 interpolant", dict(dtype=np.float32, interp=np.float64)),
                    ("float64 field, float32 interpolant", dict(dtype=np.float64, interp=np.float32))):
        worst = CA.check_rows(f"{name} {tag}", CA.pullback(model, p, x, times, cots, tol, **kw), r64, r32)
        assert max(worst.values()) <= SC.ROW_MARGIN, (name, tag, worst)
    # (2b) the oracle, over the attempts before the impulse at s = -0.5
    fld = oracle.MlpField(D, H, p, nthreads=4)
    ro = oracle.node_backward(fld, x, 0.0, 1.0, tol, tol, cots[-1], mode="unbiased", t1_or_rand=times[0], w_reg=0.0, trace=True)
    s_imp = -float(np.float32(times[0]))
    npre = sum(1 for q in r64["rows"] if q[0] < s_imp)
    assert npre >= 5 and [q[3] for q in ro["trace_bwd"][:npre]] == [q[3] for q in r64["rows"][:npre]]
    w = SC.rows_ratio(ro["trace_bwd"], r64, r32, before_s=s_imp)
    print(f"{name}: the oracle's first {npre} attempts: worst |row - row64| / bound {w:.3f}")
    assert w <= SC.ORACLE_MARGIN, (name, w)
    # (2c) the restatements with the parameter cotangent regrouped by rank
    monkeypatch.setattr(CA, "Field", SC.rank_regrouped_field(SC.GROUPS[c["B"]][0]))
    for tag, dt in (("float32, regrouped by rank", np.float32), ("float64, regrouped by rank", np.float64)):
        worst = CA.check_rows(f"{name} {tag}", CA.pullback(model, p, x, times, cots, tol, dtype=dt), r64, r32)
        assert max(worst.values()) <= SC.ROW_MARGIN, (name, tag, worst)


def test_the_row_checked_inputs_cover_every_family_and_a_rejection():
    rows = [c for c in SC.TS_CASES.values() if c["rows"] == "restatement"]
    assert {c["shape"] for c in rows} == set(SC.SHAPES) and {SC.GROUPS[c["B"]][0] for c in rows} == {2, 3}
    assert any(c.get("rejects") and c["shape"] == "Q" for c in rows) and any(c.get("rejects") and c["shape"] != "Q" for c in rows)


@pytest.mark.parametrize("shape,B", [("V1", 21), ("V4", 34), ("Q", 21)])
def test_rank_order_sum_is_a_yardstick_of_its_own(oracle, P, shape, B):
    """the oracle's VJP per shard: dy rows are the global call's rows bit for bit (samples are independent); the
    rank-order float32 sum of the shards' parameter cotangents is close to the global one (fp32 regrouping, < 1e-6) but
    not its bits — so a sharded lrnde_vjp is held to the sum, not to the unsharded result"""
    D, H = SC.SHAPES[shape]
    nranks, _ = SC.GROUPS[B]
    model, p, x = SC.inputs(P, shape, B)
    fld = oracle.MlpField(D, H, p, nthreads=4)
    lam = np.random.default_rng(9).standard_normal(x.shape).astype(np.float32)
    dy, gp = oracle.mlp_vjp(fld, x, 0.3, lam)
    parts = [oracle.mlp_vjp(fld, SC.shard(x, r, nranks), 0.3, SC.shard(lam, r, nranks)) for r in range(nranks)]
    assert np.array_equal(np.concatenate([q[0] for q in parts], axis=0), dy)
    s = SC.rank_order_sum([q[1] for q in parts])
    d = SC.rel(s, gp)
    print(f"{shape} B={B}: rel(rank-order sum, global gp) {d:.2e}")
    assert not np.array_equal(s, gp) and 0 < d < 1e-6


def test_adams_rejecting_case_rejects_in_the_oracle(oracle, P):
    c = SC.ADAMS_REJECT
    D, H = SC.SHAPES[c["shape"]]
    model, p, x = SC.inputs(P, c["shape"], c["B"], scale=c["scale"])
    fld = oracle.MlpField(D, H, p, nthreads=4)
    r = oracle.solve(fld, x, 0.0, 1.0, c["tol"], c["tol"], saveat=[1.0], maxiters=10000, solver=c["solver"])
    print("oracle", c["solver"], r["stats"])
    assert r["retcode"] == 0 and r["stats"]["nreject"] >= 1


@pytest.mark.parametrize("shape", ["Q", "V1"])
def test_biased_reversed_solve_step_counts_scatter_among_correct_implementations(oracle, P, shape):
    """test_regulariser_on_shards' :biased runs (3 x 7, scale 3, tol 1e-4): the reversed solve stops at every accepted forward
    step, each stop leaves a short remainder step whose estimate is rounding, and the controller climbs back from it steered
    by that noise.  Seven correct statements of the same solve — the oracle, the float64 and float32 restatements, the two
    mixed twins, both restatements regrouped by rank — take, measured here, 49 / 46 / 46 / 34 / 31 / 46 / 39 accepted steps
    on Q and 29 / 30 / 34 / 29 / 29 / 41 / 31 on V1 (the MI355X: 49 unsharded and 41 on three ranks on Q, 29 and 29 on V1).
    Asserted: they do not agree to within the one step the unsharded-handle yardstick allows, and regrouping by rank alone
    moves the float64 restatement's count; every one of them finishes."""
    import chain_adjoint_np as CA
    D, H = SC.SHAPES[shape]
    tol = 1e-4
    model, p, x = SC.inputs(P, shape, 21, scale=3.0)
    g = np.random.default_rng(4).standard_normal(x.shape).astype(np.float32)
    ro = oracle.node_backward(oracle.MlpField(D, H, p, nthreads=4), x, 0.0, 1.0, tol, tol, g, mode="biased", t1_or_rand=0.43,
                              w_reg=0.0, trace=True)
    assert ro["retcode"] == 0
    counts = {"oracle": ro["stats_bwd"]["naccept"]}
    base, regrouped = CA.Field, SC.rank_regrouped_field(3)
    for tag, F, dt, it in (("float64", base, np.float64, np.float64), ("float32", base, np.float32, np.float32),
                           ("float32 field, float64 interpolant", base, np.float32, np.float64),
                           ("float64 field, float32 interpolant", base, np.float64, np.float32),
                           ("float32 regrouped", regrouped, np.float32, np.float32), ("float64 regrouped", regrouped, np.float64, np.float64)):
        fld = F(model, p, dt)
        fw = CA.forward(fld, x, 0.0, 1.0, tol, tol)
        stops = sorted(-float(q[0]) for q in fw["steps"] if 0.0 < float(q[0]) < 1.0)   # :biased saves, and stops at, every step
        _lam, _mu, c, rows = CA.reverse(fld, CA.Record(fw["steps"], it), 0.0, 1.0, tol, tol, g, [], stops)
        assert fw["naccept"] == ro["stats_fwd"]["naccept"] and c[1] == 0
        counts[tag] = c[0]
    print(f"{shape} :biased reversed solve, accepted steps: {counts}")
    assert max(counts.values()) - min(counts.values()) > 1
    assert counts["float64 regrouped"] != counts["float64"] or counts["float32 regrouped"] != counts["float32"]
