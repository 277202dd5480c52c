"""Shared by tests/test_host_wide_chain_adjoint.py and tests/test_gpu_wide_chain_adjoint.py: the cases of the wide
Dense-chain handle's device-controlled adjoint loop (csrc/lrnde_wide_adjoint.hpp), the gate's arithmetic
(csrc/lrnde_adj_route.hpp wide_device_gate) restated, and the branch table of its two kernels.  No code is shared with the kernels."""
import numpy as np
import torch

import wide_chain_cases as WC

# fixed launches of a reversed solve besides the 2 per attempted step: 1 k_chadj_begin (one more per further 64 saved
# times), 4 for initdt (two evaluations, each a k_wadj_step and a k_wadj_mu), 2 for the launch pair whose prologue reports
# the end, 1 k_adj_out, and at most 2 k_axpy for cotangents at the solve's two end points
LAUNCH_C = 10
TOL = 1e-5

# ---- the gate (wide_device_gate) ----
SLOTS = 8                       # stage-record slots: K1's and stages 2..7, plus one so that FSAL needs no copy
MB = 2                          # k_wadj_mu: a work item is MB x MB output blocks of 16 x 16
MAX_MU_BLOCKS = 256             # its grid (CHADJ_MAX_MU_BLOCKS)
MAX_WG = 4096                   # CHADJ_MAX_WG
SCRATCH_MAX = 256 << 20         # WIDE_SCRATCH_MAX
CTRL_BYTES = 53 * 4             # sizeof(ChAdjCtrl) (static_assert in lrnde_wide_adjoint.hpp)


def rec_floats(dims):
    """one tile's stage record: every layer's input rows and output rows, and act0'(y), 16 columns each"""
    return sum((WC.ceil16(i) + WC.ceil16(o)) * WC.NB for i, o in zip(dims[:-1], dims[1:])) + WC.ceil16(dims[0]) * WC.NB


def mu_items(dims):
    """work items of k_wadj_mu per layer: (groups of MB x MB blocks of vec(W), chunks of 64 outputs of the t column / bias)"""
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        MT, KG = WC.ceil16(o) // 16, WC.ceil16(i) // 16
        out.append((-(-MT // MB) * -(-KG // MB), -(-o // 64)))
    return out


def gate(dims, B):
    """dict(fits, why, nwg, nitems, nmu, lds, bytes) of wide_device_gate for a chain of these widths at batch B"""
    nwg = -(-B // WC.NB)
    fixed = 2 * WC.ceil16(max(dims)) * WC.NB * 4 + WC.LDS_TAIL + CTRL_BYTES
    cap = min(WC.partcap(dims), ((WC.WIDE_LDS_MAX - fixed) // 4) & ~255)
    lds = fixed + 4 * cap
    nitems = sum(g + c for g, c in mu_items(dims))
    nmu = min(nitems, MAX_MU_BLOCKS)
    nbytes = SLOTS * nwg * rec_floats(dims) * 4 + 2 * CTRL_BYTES + 5 * (nwg + nmu) * 8
    why = None
    if lds > WC.WIDE_LDS_MAX:
        why = "WIDE_LDS_MAX"
    elif nwg > MAX_WG:
        why = "CHADJ_MAX_WG"
    elif nbytes > SCRATCH_MAX:
        why = "WIDE_SCRATCH_MAX"
    return dict(fits=why is None, why=why, nwg=nwg, nitems=nitems, nmu=nmu, lds=lds, bytes=nbytes)


def first_refused_batch(dims):
    """the smallest B the gate refuses (its conditions are monotone in the number of tiles)"""
    lo, hi = 1, 1 << 20
    assert gate(dims, lo)["fits"] and not gate(dims, hi)["fits"]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if gate(dims, mid)["fits"] else (lo, mid)
    return hi


# ---- branches of k_wadj_step / k_wadj_mu a (shape, B, series) case takes ----
BRANCHES = (
    "one_tile", "several_tiles",          # k_wadj_mu's tile-order sum: one term / a chain of several
    "tail_tile",                          # the last tile holds fewer than 16 columns (their delta is 0)
    "group_full", "group_tail_o", "group_tail_k",   # a layer's MB x MB groups: all full / an odd count of row blocks / of k blocks
    "edge_out", "edge_in",                # out / in no multiple of 16: rows of an edge block are not stored
    "time_col", "no_time_col",            # TDChain / plain Chain
    "vec_tail", "vec_full",               # out no multiple of 64 / a multiple: the last chunk of the t column and the bias
    "one_trip", "several_trips",          # work items within the grid / more than CHADJ_MAX_MU_BLOCKS
    "input_act",                          # act0'(y) is not 1
    "impulse", "end_only",                # K1 re-evaluated into its slot / no table entry
)


def branches(dims, td, in_act, B, times):
    s = set()
    nwg = -(-B // WC.NB)
    s.add("one_tile" if nwg == 1 else "several_tiles")
    if B % WC.NB:
        s.add("tail_tile")
    for i, o in zip(dims[:-1], dims[1:]):
        MT, KG = WC.ceil16(o) // 16, WC.ceil16(i) // 16
        if MT % MB == 0 and KG % MB == 0:
            s.add("group_full")
        if MT % MB:
            s.add("group_tail_o")
        if KG % MB:
            s.add("group_tail_k")
        if o % 16:
            s.add("edge_out")
        if i % 16:
            s.add("edge_in")
        s.add("vec_tail" if o % 64 else "vec_full")
    s.add("time_col" if td else "no_time_col")
    s.add("several_trips" if sum(g + c for g, c in mu_items(dims)) > MAX_MU_BLOCKS else "one_trip")
    if in_act != "identity":
        s.add("input_act")
    s.add("impulse" if any(0.0 < t < 1.0 for t in times) else "end_only")
    return s


SERIES = {"three_times": [0.25, 0.5, 1.0], "end_only": [1.0]}
BITS_SHAPES = ("mnist3", "odd_td", "seg_edges", "cap_mixed", "deep16", "physionet")
BITS_BATCHES = (1, 17, 33)
# the case of test_both_loops_same_bits that takes each branch (asserted from the shapes alone on the CPU)
BRANCH_CASE = {
    "one_tile": ("mnist3", 1, "three_times"), "several_tiles": ("mnist3", 33, "three_times"),
    "tail_tile": ("mnist3", 17, "three_times"),
    "group_full": ("seg_edges", 17, "three_times"), "group_tail_o": ("mnist3", 17, "three_times"),
    "group_tail_k": ("odd_td", 17, "three_times"),
    "edge_out": ("odd_td", 33, "three_times"), "edge_in": ("odd_td", 33, "three_times"),
    "time_col": ("mnist3", 33, "three_times"), "no_time_col": ("seg_edges", 33, "three_times"),
    "vec_tail": ("mnist3", 33, "three_times"), "vec_full": ("cap_mixed", 17, "three_times"),
    "one_trip": ("mnist3", 33, "three_times"), "several_trips": ("deep16", 17, "three_times"),
    "input_act": ("deep16", 33, "three_times"),
    "impulse": ("mnist3", 33, "three_times"), "end_only": ("mnist3", 33, "end_only"),
}


def case_branches(P, name, B, series):
    model = WC.shapes(P)[name]
    td, ia, _ = WC.spec(model)
    return branches(WC.model_dims(model), td, ia, B, SERIES[series])


# ---- running a pullback through the handle-level entry points ----
def handle_for(P, model, p, loop="device"):
    from localregneuralde_jl_amd.layers import Handle, _wide_chain_desc
    h = Handle(_wide_chain_desc(model))
    h.set_params(torch.from_numpy(p))
    h.set_adjoint_loop(loop)
    return h


def run_ts(h, x, times, cots, tol, mode="none", reg_type="error_estimate", t1_or_rand=0.43, w_reg=0.0, save_start=False):
    """recorded forward + pullback, with the trace of the reversed solve"""
    xd = torch.from_numpy(x).cuda()
    fw = h.node_forward_record_ts(xd, 0.0, 1.0, tol, tol, times, mode=mode, reg_type=reg_type, t1_or_rand=t1_or_rand,
                                  maxiters=10000, save_start=save_start)
    h.set_adjoint_trace(16384)
    try:
        bw = h.node_backward_recorded_ts(torch.from_numpy(np.asarray(cots, np.float32)).cuda(), w_reg=w_reg)
        rows = h.adjoint_trace()
    finally:
        h.set_adjoint_trace(0)
    sb = bw["stats_bwd"]
    return dict(dx=bw["dx"].cpu().numpy(), dp=bw["dp"].cpu().numpy(), counts=(sb["naccept"], sb["nreject"], sb["nf"]), rows=rows,
                reg_val=float(fw["reg_val"]), t1=float(fw["t1"]), ai=h.last_adjoint_info(), stats=sb,
                fwd=(fw["stats"]["naccept"], fw["stats"]["nreject"]))


def cotangents(times, x, seed=21, big=None):
    cots = np.random.default_rng(seed).standard_normal((len(times),) + x.shape).astype(np.float32)
    if big is not None:
        cots[big[0]] *= np.float32(big[1])
    return cots
