"""The selection conditions of tests/record_growth_cases.py re-derived on the CPU — a warning that a case drifted before anyone
spends a GPU run on it: the growth margins of every case (the C oracle's solve over the float32 numpy field and over the
float64 field rounded once), MaxIters past the first record, the stops of the lin8 field, the RK4 step counts of the float64
gradient reference, and the rounding-amplification bars.  Every measured count and distance is printed.  No GPU needed."""
import numpy as np
import pytest

import record_growth_cases as G


@pytest.mark.parametrize("name", list(G.CASES))
def test_growth_margins(oracle, name):
    import lrnde_amd as P
    c = G.CASES[name]
    model, p, x, tol, span, solver = G.case(P, name)
    rs = G.cpu_solves(oracle, model, p, x, span, tol, solver)
    counts = tuple(r["stats"]["naccept"] for r in rs)
    print(name, "accepted / rejected over the float32 field and the float64 field:", [G.stop_of(r)[1:] for r in rs])
    assert all(r["retcode"] == 0 for r in rs)
    assert counts == G.COUNTS[name], "record_growth_cases.COUNTS is what the docstrings quote"
    assert c["line"] in (G.FIRST_RECORD, G.SECOND_RECORD)
    for n in counts:
        assert n >= G.MARGIN_UP * c["line"], (name, counts)
        if c["one_doubling"]:
            assert n <= G.MARGIN_DOWN * G.SECOND_RECORD, (name, counts)
    if name == "phys_74":
        assert all(r["stats"]["nreject"] == 4 for r in rs)     # the discrete sweep's case with rejected attempts


def test_both_handles_run_the_shared_cases():
    assert set(G.TSIT5_SMALL) | set(G.TSIT5_WIDE) | set(G.ADAMS) | {n for n, _ in G.ADAMS_PULLBACK} == set(G.CASES)
    for name, shared in G.ADAMS_PULLBACK:     # the Adams pullback cases run on the inputs their RK4 reference was made for
        a, b = G.CASES[name], G.CASES[shared]
        assert all(a[k] == b[k] for k in ("model", "B", "scale", "span")) and shared in G.RK4_STEPS and a["line"] == G.SECOND_RECORD
    assert {"phys_74", "phys_196"} <= set(G.TSIT5_SMALL) & set(G.TSIT5_WIDE)
    assert all(G.CASES[n]["solver"] == "tsit5" for n in G.TSIT5_SMALL + G.TSIT5_WIDE)
    assert all(G.CASES[n]["solver"] != "tsit5" and G.CASES[n]["model"] == "physionet" for n in G.ADAMS)
    # the tiles the batches were chosen for
    assert G.CASES["phys_74"]["B"] == 9 and G.CASES["phys_119"]["B"] == G.CASES["odd130_87"]["B"] == 17


@pytest.mark.parametrize("name", ["phys_74", "phys_vcabm3_1e-5"])
def test_maxiters_past_the_first_record(oracle, name):
    """with maxiters = 70 the solve has more than 64 accepted steps when it stops: the record is found full first"""
    import lrnde_amd as P
    model, p, x, tol, span, solver = G.case(P, name)
    rs = G.cpu_solves(oracle, model, p, x, span, tol, solver, maxiters=G.MAXITERS_PAST)
    print(name, "maxiters", G.MAXITERS_PAST, [G.stop_of(r) for r in rs])
    for r in rs:
        assert r["retcode"] == G.RET_MAXITERS and r["stats"]["naccept"] > G.FIRST_RECORD
        assert r["stats"]["naccept"] + r["stats"]["nreject"] == G.MAXITERS_PAST
    if name == "phys_74":
        assert all(G.stop_of(r)[1:] == G.MAXITERS_PAST_COUNTS for r in rs)


def test_lin8_stops(oracle):
    import lrnde_amd as P
    for (solver, scale), want in G.LIN8_STOPS.items():
        model, p, x = G.lin8(P, scale)
        rs = G.cpu_solves(oracle, model, p, x, G.LIN8["span"], G.LIN8["tol"], solver)
        stops = [G.stop_of(r) for r in rs]
        print("lin8", solver, "x%g" % scale, "(retcode, accepted, rejected) over the float32 field and the float64 field:", stops)
        assert stops[0] == want
        assert all(s[1] + s[2] < G.MAX_ATTEMPTS for s in stops)
        if solver == "tsit5":
            assert stops[0] == stops[1] and stops[0][0] == G.RET_DT_NAN and stops[0][1] > 100
        else:
            assert stops[0][1] > G.SECOND_RECORD
    assert G.LIN8_STOPS[("vcab3", 12.0)][0] == G.RET_DT_LESS_THAN_MIN
    assert all(v[0] == G.RET_DT_NAN for k, v in G.LIN8_STOPS.items() if k != ("vcab3", 12.0))


@pytest.mark.parametrize("name", list(G.RK4_STEPS))
def test_rk4_step_count_of_the_gradient_reference(name):
    """halving the step count moves the float64 reference by less than 1e-5 of each gradient's norm; the golden file the
    GPU tests read holds this reference, rounded to float32"""
    from test_gpu_chain import rel
    n = G.RK4_STEPS[name]
    fine, half = G.compute_reference(name), G.compute_reference(name, n // 2)
    d = [rel(h, f) for h, f in zip(half, fine)]
    kept = [rel(k, f) for k, f in zip(G.reference(name), fine)]
    print(name, f"RK4 {n // 2} against {n} steps: dx {d[0]:.2e} dp {d[1]:.2e}; the golden file from {n} steps: {kept[0]:.1e} {kept[1]:.1e}")
    assert max(d) < G.RK4_CONVERGED
    assert max(kept) < 1e-6        # float32 rounding of the stored values (6e-8 per entry), far inside every bar


@pytest.mark.parametrize("name", list(G.PULLBACK_TWINS))
def test_pullback_amplification_bars(name):
    """the float32 and float64 restatements of the continuous pullback at the GPU test's inputs: their distance, written
    down in PULLBACK_TWINS, makes the bar; the float64 one agrees with the RK4 reference inside it, so the bar is about
    rounding, not about the method"""
    from test_gpu_chain import rel
    r64, r32 = G.pullback_twins(name)
    bars = G.pullback_bars(name)
    ref = dict(zip(("dx", "dp"), G.reference(name)))
    for k in ("dx", "dp"):
        bar, kept = bars[k]
        d, e64 = rel(r32[k], r64[k]), rel(r64[k], ref[k])
        print(f"{name} {k}: float32 restatement from float64 {d:.2e} (written down: {kept:.2e}) -> bar {bar:.2e}; float64 restatement "
              f"from RK4 autograd {e64:.2e}; forward steps {r64['fwd']} / {r32['fwd']}, reversed {r64['counts'][:2]} / {r32['counts'][:2]}")
        assert bar == max(3e-4, 4.0 * kept)
        assert 0.5 * d <= kept <= 2.0 * d, "PULLBACK_TWINS no longer says what the restatements give"
        assert e64 <= bar
    assert r64["fwd"][0] > G.CASES[name]["line"] and r32["fwd"][0] > G.CASES[name]["line"]
    if name != "phys_119":
        assert all(bars[k][0] == 3e-4 for k in bars)          # the project's bar holds there


@pytest.mark.parametrize("name", G.TSIT5_SMALL + ("odd130_87",))
def test_solution_amplification_bars(name):
    from test_gpu_chain import err
    bar, d = G.solution_bar(name)
    r64, r32 = G.solution_twins(name)
    print(f"{name}: np_restatement.solve over Chain32 from Chain64 {d:.2e} -> bar {bar:.2e}; steps {r64['naccept']}+{r64['nreject']} / "
          f"{r32['naccept']}+{r32['nreject']}; |u| {np.abs(r64['u']).max():.3g}")
    assert bar == max(1e-5, 0.5 * G.CASES[name]["tol"], 4.0 * d) and np.isfinite(r64["u"]).all()
    assert err(r32["u"], r64["u"]) == d and r64["naccept"] > G.CASES[name]["line"]


@pytest.mark.parametrize("name", ["phys_74", "phys_196", "small3_176"])
def test_discrete_yardstick_on_the_long_grids(name):
    """frozen_grads and sweep64 agree on a grid of more than 64 / 128 steps; the bar the GPU sweep is held to is printed"""
    import torch
    import chain_adjoint_np as CA
    import chain_discrete_np as CD
    import lrnde_amd as P
    from test_gpu_chain import rel
    model, p, x, tol, span, _ = G.case(P, name)
    times = G.series_times(span, G.DISCRETE_FRACTIONS)
    cots = G.cotangents(len(times), x, seed=12)
    fw = CA.forward(CA.Field(model, p, np.float32), x, span[0], span[1], tol, tol, saveat=times)
    grid = CD.grid_of(fw["steps"])
    y64 = CD.frozen_grads(model, p, x, grid, span[0], span[1], times, cots)
    y32 = CD.frozen_grads(model, p, x, grid, span[0], span[1], times, cots, dtype=torch.float32)
    s64 = CD.sweep64(model, p, x, grid, span[0], span[1], times, cots)
    d = [rel(s64[k], y64[k]) for k in (0, 1)]
    print(f"{name}: {len(grid)} steps; sweep64 from frozen_grads dx {d[0]:.2e} dp {d[1]:.2e}; bar dx {CD.bound(y32[0], y64[0]):.2e} "
          f"dp {CD.bound(y32[1], y64[1]):.2e}")
    assert len(grid) > G.CASES[name]["line"] and max(d) < 1e-8


def test_latent_step_crosses_the_record(oracle):
    """the Latent-ODE training step of the GPU test: z0 from the encoder's host restatement with the model's own eps draw,
    then the node field's solve over both CPU fields"""
    import latent_cases as LC
    import lrnde_amd as P
    c = G.LATENT
    dims, make, flat, node, (data, mask, dt) = G.latent_inputs(P)
    model = make()
    st = model.initialstates(np.random.default_rng(5))
    eps, _ = model.reparam.draw(st["reparam"], c["B"], dims[3])
    z0 = LC.run_host(dims, flat, LC.x_of(data, mask, dt), eps)["z0"]
    rs = G.cpu_solves(oracle, model.gen_dynamics, node, z0, (0.0, 1.0), c["tol"])
    counts = tuple(r["stats"]["naccept"] for r in rs)
    print("latent step: accepted / rejected over the float32 field and the float64 field:", [G.stop_of(r)[1:] for r in rs])
    assert counts == c["counts"] and all(n >= G.MARGIN_UP * c["line"] for n in counts)
