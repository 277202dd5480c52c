"""The adaptive NeuralDSDE solve on the virtual Brownian tree (lrnde_sde_set_path_tree, csrc/lrnde_sde_tree.hpp):
no (nfine+1, B, D) path array exists, W at a grid index is a function of (seed, stream, column, index).

Every comparison is device against device, or against float32 numpy (tests/brownian_tree_np.py) on the device's own normals:

1. `tree_path` is the definition's array bit for bit; a column does not depend on B; a coarse tree is every 2^k-th row of a fine one;
2. plain solves with the tree enabled and W=None equal the same solves on the materialised array: state, counts, every trace row —
   Euler-Heun on both device forms and the host loop, Milstein and SRI on the device loop and the host loop;
3. the layer with noise_source="tree" equals the layer given the tree's arrays explicitly: forward (three modes, user saveat,
   three solvers) and both pullbacks, inside and outside the one-launch sweep's gate; records of the two sources do not mix;
4. the MNIST-SDE model's training step likewise;
5. the capability: L = 16 at B = 512, D = 32 — the array form would be 4.29 GB — runs forward and pullback in under 256 MB, and an
   L = 14 solve equals the oracle loop on the numpy-built path;
6. refusals come back as LRNDE_BADARG with a message and leave the handle usable."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import brownian_tree_np as BT
import sde_adaptive_np as S

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 0xA4093822299F31D0
TW, TZ = 6, 7     # the streams of the trees of W and of SRI's second path Z


def _desc(P, D, H):
    from localregneuralde_jl_amd.layers import _mlp_desc
    return _mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)))


def _handle(P, D, H=16, seed=None, scale=2.0):
    h = P.SdeHandle(_desc(P, D, H))
    if seed is not None:
        pd, pg = S.sde_params(D, H, seed)
        h.set_params((pd * f32(scale)).astype(f32), pg)
    return h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _tableau(seed=41, scale=0.1):
    from localregneuralde_jl_amd import _lib as L
    rng = np.random.default_rng(seed)
    return [float(f32(rng.uniform(-0.6, 0.9) * scale)) for _ in L.SRI_FIELDS]


def _np_tree(h, seed, stream, L, B, span):
    """the definition on the device's own normals: (2^L + 1, B, D)"""
    nfine = 1 << L
    z = h.draw_noise(seed, stream, nfine, B, 1.0, False).cpu().numpy().reshape(nfine, B * h.D)
    return BT.build(z, L, span).reshape(nfine + 1, B, h.D)


# ---- 1. the materialised path ----
@pytest.mark.parametrize("L,B,D", [(0, 2, 5), (1, 3, 5), (5, 3, 5), (8, 512, 32), (10, 6, 72)])
def test_tree_path_is_the_definition_bit_for_bit(gpu_pkg, L, B, D):
    h = _handle(gpu_pkg, D)
    for t0, t2 in ((0.0, 1.0), (0.25, 1.75)):
        got = h.tree_path(SEED, TW, L, B, t0, t2).cpu().numpy()
        ref = _np_tree(h, SEED, TW, L, B, f32(f32(t2) - f32(t0)))
        assert got.shape == ref.shape == ((1 << L) + 1, B, D) and np.isfinite(got).all() and not got[0].any()
        assert np.array_equal(_bits(got), _bits(ref)), (L, B, D, t0, t2, int((_bits(got) != _bits(ref)).sum()))
    if L == 5:   # the second path's stream, once; it is another path
        gz = h.tree_path(SEED, TZ, L, B, 0.0, 1.0).cpu().numpy()
        assert np.array_equal(_bits(gz), _bits(_np_tree(h, SEED, TZ, L, B, f32(1.0))))
        assert not np.array_equal(gz[1:], h.tree_path(SEED, TW, L, B, 0.0, 1.0).cpu().numpy()[1:])


def test_tree_path_columns_and_refinement(gpu_pkg):
    h = _handle(gpu_pkg, 32)
    big = h.tree_path(SEED, TW, 8, 512, 0.0, 1.0)
    assert torch.equal(h.tree_path(SEED, TW, 8, 7, 0.0, 1.0), big[:, :7])          # a column does not depend on B
    assert torch.equal(h.tree_path(SEED, TW, 5, 512, 0.0, 1.0), big[::8])          # W_5[k] == W_8[8 k]
    assert torch.equal(h.tree_path(SEED, TW, 0, 512, 0.0, 1.0), big[::256])
    assert not torch.equal(h.tree_path(SEED + 1, TW, 5, 7, 0.0, 1.0), big[::8, :7])
    # a Brownian motion: Var(W[nfine]) = span and unit-variance increments over 16384 columns (6 sigma)
    inc = (big[1:] - big[:-1]).double() * 16.0
    n = inc.numel()
    assert abs(float(inc.var()) - 1) < 6 * np.sqrt(2 / n) and abs(float(big[256].double().var()) - 1) < 6 * np.sqrt(2 / (512 * 32))


# ---- 2. plain solves: the tree with W=None == the array it materialises ----
SHAPES = [(32, 64, 40, 8), (5, 7, 3, 5), (64, 112, 17, 6), (72, 32, 6, 5)]    # (D, H, B, L); the last runs the generic kernels
#           tolerance per solver (Milstein's residual is the whole change of u, src/perform_step.jl:166), first step, drift scale
SOLVERS = {"EulerHeun": dict(tol=0.14, dt0=0.5, scale=2.0), "RKMil": dict(tol=0.5, dt0=1.0, scale=2.0), "SRI": dict(tol=0.1, dt0=0.4, scale=2.0)}
ROUTES = [("EulerHeun", None), ("EulerHeun", "LRNDE_SDE_NO_PERSIST"), ("EulerHeun", "LRNDE_SDE_HOST_LOOP"), ("RKMil", None),
          ("RKMil", "LRNDE_SDE_HOST_LOOP"), ("SRI", None), ("SRI", "LRNDE_SDE_HOST_LOOP")]


def _with_option(P, name, fn):
    if name is None:
        return fn()
    P.set_option(name, 1)
    try:
        return fn()
    finally:
        P.set_option(name, 0)


@pytest.mark.parametrize("solver,switch", ROUTES, ids=[f"{s}-{(w or 'default').replace('LRNDE_SDE_', '').lower()}" for s, w in ROUTES])
@pytest.mark.parametrize("D,H,B,L", SHAPES)
def test_solve_on_the_tree_equals_the_solve_on_its_array(gpu_pkg, D, H, B, L, solver, switch):
    P = gpu_pkg
    cfg = SOLVERS[solver]
    h = _handle(P, D, H, seed=7, scale=cfg["scale"])
    nfine = 1 << L
    u0 = torch.from_numpy(np.random.default_rng(107).standard_normal((B, D)).astype(f32)).cuda()
    t0, t1 = 0.25, 1.75
    kw = dict(dt0=cfg["dt0"], maxiters=4000, solver=solver, tableau=_tableau() if solver == "SRI" else None)
    W = h.tree_path(SEED, TW, L, B, t0, t1)
    Z = h.tree_path(SEED, TZ, L, B, t0, t1) if solver == "SRI" else None

    def run(tree):
        if tree:
            h.set_path_tree(SEED)
            r = h.solve_adaptive(u0, None, t0, t1, cfg["tol"], cfg["tol"], nfine=nfine, **kw)
        else:
            h.clear_path_tree()
            r = h.solve_adaptive(u0, W, t0, t1, cfg["tol"], cfg["tol"], path_z=Z, **kw)
        return r, h.last_solve_info()

    (a, ia), (b, ib) = _with_option(P, switch, lambda: (run(True), run(False)))
    print(f"{solver} D={D} H={H} B={B} L={L} {switch}: loop kind {ia['kind']}, accepted {a['stats']['naccept']}, rejected {a['stats']['nreject']}")
    assert ia["kind"] == ib["kind"]
    if switch == "LRNDE_SDE_HOST_LOOP" or D > 64:
        assert ia["kind"] == 0
    else:
        assert ia["kind"] == (2 if solver == "EulerHeun" and switch is None else 1)
    assert all(a["stats"][k] == b["stats"][k] for k in ("retcode", "naccept", "nreject", "nf", "iters")), (a["stats"], b["stats"])
    assert a["stats"]["retcode"] == 0 and a["stats"]["naccept"] >= 1
    assert np.array_equal(a["trace"].view(np.int32), b["trace"].view(np.int32))
    assert torch.equal(a["u_end"], b["u_end"]) and torch.isfinite(a["u_end"]).all()
    # a disabled handle is what it was: a NULL path is refused
    from localregneuralde_jl_amd import _lib
    with pytest.raises(_lib.LrndeError):
        h.solve_adaptive(u0, None, t0, t1, cfg["tol"], cfg["tol"], nfine=nfine, **kw)


# ---- 3. the layer ----
def _layer(P, D, H, L, solver, mode, src, **kw):
    cfg = SOLVERS[solver]
    extra = dict(tableau=_tableau(), adaptive=True) if solver == "SRI" else (dict(adaptive=True) if solver == "RKMil" else {})
    return P.NeuralDSDE(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)), P.Dense(D, D), nfine=1 << L, abstol=cfg["tol"], reltol=cfg["tol"],
                        noise_source=src, solver=solver, regularize=mode, tspan=(0.25, 1.75), **extra, **kw)


def _replica_seed(st):
    rng = copy.deepcopy(st["rng"])
    return int(rng.integers(0, 2 ** 64, dtype=np.uint64))


def _explicit(h, seed, L, B, shape, solver):
    """what the tree layer drew for `seed`, as arrays"""
    out = dict(path=h.tree_path(seed, TW, L, B, 0.25, 1.75).view((1 + (1 << L),) + shape), z_local=h.draw_noise(seed, 1, 1, B, 1.0, False)[0].view(shape))
    if solver == "SRI":
        out.update(path_z=h.tree_path(seed, TZ, L, B, 0.25, 1.75).view((1 + (1 << L),) + shape), z_local2=h.draw_noise(seed, 5, 1, B, 1.0, False)[0].view(shape))
    return out


def _ps(D, H, seed=21, scale=1.5):
    pd, pg = S.sde_params(D, H, seed)
    return dict(drift=(pd * f32(scale)).astype(f32), diffusion=pg)


@pytest.mark.parametrize("mode", ["none", "unbiased", "biased"])
@pytest.mark.parametrize("solver", ["EulerHeun", "RKMil", "SRI"])
def test_tree_layer_forward_equals_the_layer_on_explicit_arrays(gpu_pkg, solver, mode):
    P = gpu_pkg
    D, H, B, L = 32, 64, 40, 6
    ps = _ps(D, H)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, D)).astype(f32)).cuda()
    saveat = (0.25, 0.6, 1.0, 1.75)
    node = _layer(P, D, H, L, solver, mode, "tree", saveat=saveat)
    st = node.initialstates(np.random.default_rng(3))
    sol, st2 = node(x, ps, st)
    seed = _replica_seed(st)
    arr = _explicit(node.handle(), seed, L, B, (B, D), solver)
    sol_e, st2_e = node(x, ps, st, **arr)
    assert len(sol.u) == len(sol_e.u) >= 2 and list(sol.t) == list(sol_e.t)
    assert all(torch.equal(a, b) for a, b in zip(sol.u, sol_e.u)) and all(torch.isfinite(a).all() for a in sol.u)
    assert st2["reg_val"] == st2_e["reg_val"] and (st2["reg_val"] == 0) == (mode == "none")
    assert st2["nfe_drift"] == st2_e["nfe_drift"] and st2["nfe_diffusion"] == st2_e["nfe_diffusion"]
    assert sol.stats == sol_e.stats
    assert st2["rng"].bit_generator.state == st2_e["rng"].bit_generator.state != st["rng"].bit_generator.state
    print(f"{solver} {mode}: accepted {sol.stats['naccept']}, rejected {sol.stats['nreject']}, series {len(sol.u)}, reg_val {st2['reg_val']:.4g}")


@pytest.mark.parametrize("D,H,B,L,route", [(32, 64, 40, 6, 1), (72, 32, 6, 5, 0)], ids=["one-launch-sweep", "per-step"])
@pytest.mark.parametrize("solver", ["EulerHeun", "RKMil", "SRI"])
def test_tree_layer_pullbacks_equal_the_explicit_arrays(gpu_pkg, solver, D, H, B, L, route):
    P = gpu_pkg
    ps = _ps(D, H)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, D)).astype(f32)).cuda()
    node = _layer(P, D, H, L, solver, "unbiased", "tree", saveat=(0.6, 1.0, 1.75), dt0=0.5)   # (a long first step: rejected slots are rewritten)
    st = node.initialstates(np.random.default_rng(3))
    sol, _ = node(x, ps, st)
    print(f"{solver} D={D}: accepted {sol.stats['naccept']}, rejected {sol.stats['nreject']}")
    du = torch.from_numpy(np.random.default_rng(9).standard_normal((len(sol.u), B, D)).astype(f32)).cuda()
    dx, dps, info = node.pullback_series(x, ps, st, du, w_reg=2.0)
    arr = _explicit(node.handle(), _replica_seed(st), L, B, (B, D), solver)
    dx_e, dps_e, info_e = node.pullback_series(x, ps, st, du, w_reg=2.0, **arr)
    assert info["backward"]["kind"] == info_e["backward"]["kind"] == route, (info["backward"], info_e["backward"])
    assert torch.equal(dx, dx_e) and torch.equal(dps["drift"], dps_e["drift"]) and torch.equal(dps["diffusion"], dps_e["diffusion"])
    assert info["st"]["reg_val"] == info_e["st"]["reg_val"] != 0 and torch.isfinite(dx).all() and (dx != 0).any()
    dx1, dps1, i1 = node.pullback(x, ps, st, du[-1], w_reg=2.0)        # the tree again after an array forward
    dx1_e, dps1_e, i1_e = node.pullback(x, ps, st, du[-1], w_reg=2.0, noise=arr["path"]) if solver != "SRI" else \
        node.pullback_series(x, ps, st, None, du_end=du[-1], w_reg=2.0, **arr)
    assert torch.equal(dx1, dx1_e) and torch.equal(dps1["drift"], dps1_e["drift"]) and torch.equal(dps1["diffusion"], dps1_e["diffusion"])
    assert i1["backward"]["kind"] == i1_e["backward"]["kind"] == route, (i1["backward"], i1_e["backward"])


def test_records_of_the_two_sources_do_not_mix(gpu_pkg):
    """a tree forward, then clear_path_tree() and a fresh array forward on the SAME handle: the backward sweeps the array record
    (the result of a handle that never saw the tree); and a tree record made after it is swept from its own increments"""
    P = gpu_pkg
    D, H, B, L = 32, 64, 24, 6
    ps = _ps(D, H)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((B, D)).astype(f32)).cuda()
    h = P.SdeHandle(_desc(P, D, H))
    h.set_params(ps["drift"], ps["diffusion"])
    fresh = P.SdeHandle(_desc(P, D, H))
    fresh.set_params(ps["drift"], ps["diffusion"])
    z = h.draw_noise(SEED, 1, 1, B, 1.0, False)[0]
    W = h.tree_path(SEED + 9, TW, L, B, 0.0, 1.0)         # another path than the tree forward's
    kw = dict(mode="unbiased", t1_or_rand=0.43, z_local=z)
    h.set_path_tree(SEED)
    ft = h.node_forward_record(x, None, 0.0, 1.0, 0.14, 0.14, nfine=1 << L, **kw)
    du = torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(ft["u"].shape)).astype(f32)).cuda()
    bt = h.node_backward_recorded(du, w_reg=1.0)
    h.clear_path_tree()
    fa = h.node_forward_record(x, W, 0.0, 1.0, 0.14, 0.14, **kw)
    ba = h.node_backward_recorded(du[: fa["u"].shape[0]], w_reg=1.0)
    fresh.node_forward_record(x, W, 0.0, 1.0, 0.14, 0.14, **kw)
    bf = fresh.node_backward_recorded(du[: fa["u"].shape[0]], w_reg=1.0)
    assert all(torch.equal(ba[k], bf[k]) for k in ("dx", "dp_drift", "dp_diff"))
    assert not torch.equal(ba["dx"], bt["dx"])
    h.set_path_tree(SEED)
    h.node_forward_record(x, None, 0.0, 1.0, 0.14, 0.14, nfine=1 << L, **kw)
    h.clear_path_tree()                                   # the record remembers its source: the backward needs no path
    bt2 = h.node_backward_recorded(du, w_reg=1.0)
    assert all(torch.equal(bt[k], bt2[k]) for k in ("dx", "dp_drift", "dp_diff"))


@pytest.mark.parametrize("first", ["tree", "array"])
def test_a_grown_record_serves_a_larger_batch(gpu_pkg, first):
    """the record's capacity is counted in slots of the CURRENT batch: a forward at a small B leaves a buffer of 256 slots (a tree
    record that grew past 64, or an array record of nfine = 256), which at a 4x larger B holds exactly the 64 slots the next tree
    forward asks for first — that forward accepts more than 64 steps, so it has to grow the record again, and its forward and
    pullback equal a fresh handle's bit for bit"""
    P = gpu_pkg
    D, H, L, tol = 8, 16, 14, 0.1
    pd, pg = S.sde_params(D, H, 7)
    pd = (pd * f32(2.0)).astype(f32)
    xs = {B: torch.from_numpy(np.random.default_rng(107).standard_normal((B, D)).astype(f32)).cuda() for B in (4, 16)}

    def tree_run(h, B):
        h.set_path_tree(SEED)
        z = h.draw_noise(SEED, 1, 1, B, 1.0, False)[0]
        fw = h.node_forward_record(xs[B], None, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.43, z_local=z, nfine=1 << L)
        du = torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(fw["u"].shape)).astype(f32)).cuda()
        return fw, h.node_backward_recorded(du, w_reg=2.0)

    h, fresh = P.SdeHandle(_desc(P, D, H)), P.SdeHandle(_desc(P, D, H))
    h.set_params(pd, pg); fresh.set_params(pd, pg)
    if first == "tree":
        f4, _ = tree_run(h, 4)
        assert f4["stats"]["naccept"] > 64      # (grew to 256 slots of 4 x 8 floats)
    else:
        h.node_forward_record(xs[4], h.tree_path(SEED, TW, 8, 4, 0.0, 1.0), 0.0, 1.0, tol, tol, mode="none")   # (nfine = 256 slots)
    fa, ba = tree_run(h, 16)
    fb, bb = tree_run(fresh, 16)
    print(f"{first} first: B=16 accepted {fa['stats']['naccept']}, rejected {fa['stats']['nreject']}")
    assert fa["stats"]["naccept"] > 64 and fa["stats"] == fb["stats"]
    assert torch.equal(fa["u"], fb["u"]) and fa["reg_val"] == fb["reg_val"] != 0 and np.array_equal(fa["t"], fb["t"])
    assert all(torch.equal(ba[k], bb[k]) for k in ("dx", "dp_drift", "dp_diff")) and torch.isfinite(ba["dx"]).all() and (ba["dx"] != 0).any()


@pytest.mark.parametrize("mode", ["unbiased", "biased"])
def test_host_loop_grows_a_tree_record_to_the_default_routes_bits(oracle, gpu_pkg, mode):
    """LRNDE_SDE_HOST_LOOP on the tree: the host-controlled loop finds its 64-slot record full (its own capacity check, ahead of
    the controller), the layer replaces the record and the solve runs again — series, times, reg_val and counts of the default
    route (the device controller) bit for bit.  nfine = 256 with the automatic initial dt at tolerance 0.05: the step length
    grows from one interval under qmax = 1.125 and tests/sde_adaptive_np.py's loop accepts 117 steps on the definition's path
    (chosen with it on the CPU); the test holds it to > 64 on the materialised path of the device's own normals."""
    P = gpu_pkg
    D, H, B, L, tol = 4, 8, 3, 8, 0.05
    pd, pg = S.sde_params(D, H, 7)
    pd = (pd * f32(2.0)).astype(f32)
    x = np.random.default_rng(107).standard_normal((B, D)).astype(f32)
    h = P.SdeHandle(_desc(P, D, H))
    h.set_params(pd, pg)
    z = h.draw_noise(SEED, 1, 1, B, 1.0, False)[0]
    drift, diff = S.oracle_fields(oracle, D, H, pd, pg)
    ref = S.sde_node_forward(oracle, "EulerHeun", drift, diff, x, _np_tree(h, SEED, TW, L, B, f32(1.0)), 0.0, 1.0, tol, tol, mode=mode,
                             t1_or_rand=0.43, z_local=z.cpu().numpy(), maxiters=1000)
    assert ref["naccept"] > 64, ref["naccept"]
    h.set_path_tree(SEED)

    def run():
        r = h.node_forward_record(torch.from_numpy(x).cuda(), None, 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.43, z_local=z, nfine=1 << L,
                                  maxiters=1000)
        return r, h.last_solve_info()

    (a, ia), (b, ib) = _with_option(P, "LRNDE_SDE_HOST_LOOP", run), run()
    print(f"{mode}: host loop accepted {a['stats']['naccept']}, rejected {a['stats']['nreject']}, series {len(a['t'])}, reg_val {a['reg_val']:.4g}")
    assert ia["kind"] == 0 and ib["kind"] == 2
    assert a["stats"]["naccept"] == b["stats"]["naccept"] == ref["naccept"] and a["stats"]["nreject"] == b["stats"]["nreject"] == ref["nreject"]
    assert a["stats"] == b["stats"] and a["stats"]["retcode"] == 0
    assert np.array_equal(_bits(a["t"]), _bits(b["t"])) and len(a["t"]) == (ref["naccept"] + 1 if mode == "biased" else 2)
    assert torch.equal(a["u"], b["u"]) and torch.isfinite(a["u"]).all()
    assert _bits(a["reg_val"]) == _bits(b["reg_val"]) and a["reg_val"] != 0
    assert a["nfe_drift"] == b["nfe_drift"] and a["nfe_diffusion"] == b["nfe_diffusion"]


# ---- 4. the model ----
def test_tree_model_training_step_equals_the_explicit_arrays(gpu_pkg):
    P = gpu_pkg
    from localregneuralde_jl_amd.sde_model import construct_mlp_sde, glorot_mlp_sde_params
    from localregneuralde_jl_amd.training import run_sde_training_step
    B = 5
    model = construct_mlp_sde(in_dims=12, state_dims=8, hidden_dims=16, num_classes=3, nfine=32, noise_source="tree", abstol=0.14, reltol=0.14)
    ps = glorot_mlp_sde_params(model, seed=2)
    st = model.initialstates(np.random.default_rng(4))
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((B, 12)).astype(f32)).cuda()
    labels = torch.tensor([0, 2, 1, 1, 0], dtype=torch.int32, device="cuda")
    loss, st2, stats, grads, _ = run_sde_training_step(model, ps, st, x, labels, 10.0)
    h = model.neural_dsde.handle()
    seed = _replica_seed(st["neural_dsde"])
    W = h.tree_path(seed, TW, 5, B, 0.0, 1.0)
    z = h.draw_noise(seed, 1, 1, B, 1.0, False)[0]
    loss_e, st2_e, stats_e, grads_e, _ = run_sde_training_step(model, ps, st, x, labels, 10.0, path=W, z_local=z)
    assert loss == loss_e and np.isfinite(loss) and stats["reg_val"] == stats_e["reg_val"] != 0 and stats["nfe"] == stats_e["nfe"]
    assert torch.equal(stats["y_pred"], stats_e["y_pred"])
    for k in ("downsample", "classifier"):
        assert torch.equal(grads[k], grads_e[k]) and (grads[k] != 0).any(), k
    for k in ("drift", "diffusion"):
        assert torch.equal(grads["neural_dsde"][k], grads_e["neural_dsde"][k]) and (grads["neural_dsde"][k] != 0).any(), k


# ---- 5. the capability ----
@pytest.mark.parametrize("mode", ["unbiased", "biased"])
def test_a_grid_of_65536_intervals_needs_no_path_array(gpu_pkg, mode):
    """L = 16 at BASELINE config 5's shape: the array form of this grid is (65536 + 1) x 512 x 32 floats = 4.29 GB (and its record of
    end states as much again); the tree's forward and pullback leave less than 256 MB in use — with the layer's default maxiters
    (1000: the record holds 2 x min(nfine, maxiters) states), and also for :biased without a saveat, whose series is every
    accepted step (never a grid-sized buffer)"""
    P = gpu_pkg
    D, H, B, L, tol = 32, 64, 512, 16, 0.14
    array_bytes = ((1 << L) + 1) * B * D * 4
    assert array_bytes > 4.29e9
    ps = _ps(D, H, seed=7, scale=2.0)
    x = torch.from_numpy(np.random.default_rng(107).standard_normal((B, D)).astype(f32)).cuda()
    node = P.NeuralDSDE(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)), P.Dense(D, D), nfine=1 << L, abstol=tol, reltol=tol,
                        noise_source="tree", regularize=mode)
    assert node.maxiters == 1000
    st = node.initialstates(np.random.default_rng(0))
    du = torch.from_numpy(np.random.default_rng(9).standard_normal((B, D)).astype(f32)).cuda()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    dx, dps, info = node.pullback(x, ps, st, du, w_reg=2.0)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    sol, st2 = info["sol"], info["st"]
    used = free0 - free1
    # (the series is held alive while the memory is read — :biased: the start value and every accepted step; :unbiased: sol(t1), sol(t2))
    assert len(sol.u) == (sol.stats["naccept"] + 1 if mode == "biased" else 2)
    print(f"L=16 B=512 D=32 {mode}: accepted {sol.stats['naccept']}, rejected {sol.stats['nreject']}, {used / 2 ** 20:.1f} MB in use after forward + pullback "
          f"(the path array alone would be {array_bytes / 1e9:.2f} GB); backward {info['backward']}")
    assert sol.stats["retcode"] == 0 and sol.t[-1] == f32(1.0)
    assert torch.isfinite(sol.u[-1]).all() and torch.isfinite(dx).all() and (dx != 0).any()
    assert torch.isfinite(dps["drift"]).all() and torch.isfinite(dps["diffusion"]).all() and np.isfinite(st2["reg_val"]) and st2["reg_val"] != 0
    assert used < 256 * 2 ** 20, used


@pytest.mark.parametrize("mode", ["unbiased", "none", "biased"])
def test_fine_grid_tree_layer_forward_equals_the_oracle_loop(oracle, gpu_pkg, mode):
    """L = 14: the layer on the tree == tests/sde_adaptive_np.py's loop fed the numpy-built path of the device's normals.  The solve
    accepts more than 64 steps, so the tree record grows and the solve runs again; :biased saves every step, so the series buffer
    does not fit at first either and the forward is repeated with the size it reported — the same bits throughout"""
    P = gpu_pkg
    D, H, B, L, tol = 8, 16, 8, 14, 0.1
    nfine = 1 << L
    pd, pg = S.sde_params(D, H, 7)
    pd = (pd * f32(2.0)).astype(f32)
    x = np.random.default_rng(107).standard_normal((B, D)).astype(f32)
    node = P.NeuralDSDE(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)), P.Dense(D, D), nfine=nfine, abstol=tol, reltol=tol,
                        noise_source="tree", regularize=mode)
    st = node.initialstates(np.random.default_rng(0))
    sol, st2 = node(torch.from_numpy(x).cuda(), dict(drift=pd, diffusion=pg), st)
    rng = copy.deepcopy(st["rng"])
    seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    r01 = f32(rng.random(dtype=f32)) if mode != "none" else f32(0)
    assert rng.bit_generator.state == st2["rng"].bit_generator.state
    h = node.handle()
    W = _np_tree(h, seed, TW, L, B, f32(1.0))
    z = h.draw_noise(seed, 1, 1, B, 1.0, False)[0].cpu().numpy()
    drift, diff = S.oracle_fields(oracle, D, H, pd, pg)
    ref = S.sde_node_forward(oracle, "EulerHeun", drift, diff, x, W, 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=float(r01), z_local=z,
                             saveat=(), save_start=-1, maxiters=node.maxiters)
    assert sol.stats["naccept"] == ref["naccept"] and sol.stats["nreject"] == ref["nreject"], (sol.stats, ref["naccept"], ref["nreject"])
    assert ref["naccept"] > 64 and (mode != "biased" or len(sol.u) == ref["naccept"] + 1 > 67)   # (both growth paths are taken)
    assert st2["nfe_drift"] == ref["nfe_drift"] and st2["nfe_diffusion"] == ref["nfe_diffusion"]
    assert np.array_equal(np.array(sol.t, f32), ref["t"]) and st2["reg_val"] == ref["reg_val"]
    assert np.array_equal(_bits(torch.stack(sol.u).cpu().numpy()), _bits(ref["u"]))
    print(f"L=14 {mode}: accepted {ref['naccept']}, rejected {ref['nreject']}, first steps {ref['steps'][:4]}, reg_val {ref['reg_val']:.4g}")


# ---- 6. refusals ----
def test_refusals_are_badarg_with_a_message_and_leave_the_handle_usable(gpu_pkg):
    from localregneuralde_jl_amd import _lib
    P = gpu_pkg
    D, B = 5, 3
    h = _handle(P, D, 7, seed=7)
    u0 = torch.from_numpy(np.random.default_rng(1).standard_normal((B, D)).astype(f32)).cuda()
    h.set_path_tree(SEED)
    for nfine in (48, 1 << 21):
        with pytest.raises(_lib.LrndeError) as e:
            h.solve_adaptive(u0, None, 0.0, 1.0, 0.2, 0.2, nfine=nfine)
        assert e.value.code == 4 and "2^L" in str(e.value), e.value
        with pytest.raises(_lib.LrndeError) as e:
            h.node_forward_record(u0, None, 0.0, 1.0, 0.2, 0.2, mode="none", nfine=nfine)
        assert e.value.code == 4 and "2^L" in str(e.value), e.value
    assert _lib.lib.lrnde_sde_set_path_tree(None, 1, SEED) == 4
    # a sharded handle refuses the tree (a shard numbers its columns from its own first sample); unsharded again it runs
    ctx, lc = C.c_void_p(), C.c_void_p()
    assert _lib.lib.lrnde_hook_sde_drift_ctx(h._h, C.byref(ctx)) == 0 and ctx.value
    assert _lib.lib.lrnde_hook_sde_drift_ctx(None, C.byref(ctx)) == 4 and _lib.lib.lrnde_hook_sde_drift_ctx(h._h, None) == 4
    assert _lib.lib.lrnde_local_comm_create(C.byref(lc), 1) == 0 and _lib.lib.lrnde_comm_init_local(ctx, lc, 0) == 0
    try:
        with pytest.raises(_lib.LrndeError) as e:
            h.solve_adaptive(u0, None, 0.0, 1.0, 0.2, 0.2, nfine=32)
        assert e.value.code == 4 and "sharded" in str(e.value), e.value
        with pytest.raises(_lib.LrndeError) as e:
            h.node_forward_record(u0, None, 0.0, 1.0, 0.2, 0.2, mode="none", nfine=32)
        assert e.value.code == 4 and "sharded" in str(e.value), e.value
    finally:
        assert _lib.lib.lrnde_comm_destroy(ctx) == 0 and _lib.lib.lrnde_local_comm_destroy(lc) == 0
    assert _lib.lib.lrnde_sde_set_path_tree(h._h, 2, SEED) == 4 and "enable" in _lib.lib.lrnde_sde_last_error(h._h).decode()
    out = torch.empty((33, B, D), dtype=torch.float32, device="cuda")
    ptr = C.c_void_p(out.data_ptr())
    assert _lib.lib.lrnde_sde_tree_path(None, SEED, TW, 5, B, 0.0, 1.0, ptr) == 4
    for args, word in (((21, B, 0.0, 1.0, ptr), "levels"), ((-1, B, 0.0, 1.0, ptr), "levels"), ((5, 0, 0.0, 1.0, ptr), "batch"),
                       ((5, B, 0.0, 1.0, None), "null"), ((5, B, 1.0, 1.0, ptr), "t2")):
        assert _lib.lib.lrnde_sde_tree_path(h._h, SEED, TW, *args) == 4, args
        assert word in _lib.lib.lrnde_sde_last_error(h._h).decode(), (args, _lib.lib.lrnde_sde_last_error(h._h))
    with pytest.raises(ValueError):
        h.solve_adaptive(u0, None, 0.0, 1.0, 0.2, 0.2)            # W=None without nfine=
    # still usable, and still on the tree
    a = h.solve_adaptive(u0, None, 0.0, 1.0, 0.2, 0.2, nfine=32)
    h.clear_path_tree()
    b = h.solve_adaptive(u0, h.tree_path(SEED, TW, 5, B, 0.0, 1.0), 0.0, 1.0, 0.2, 0.2)
    assert a["stats"]["retcode"] == 0 and torch.equal(a["u_end"], b["u_end"])
