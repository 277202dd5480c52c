"""csrc/lrnde_adj_route.hpp on the host: which of its six routes a recorded backward takes and the launch plan of that
route.  The two wide gates against their restatements (wide_chain_adjoint_cases.gate, wide_chain_discrete_cases.gate); the
two small-chain gates against their arithmetic written out here from the formulas, with the last
input that fits and the first that does not at every limit; the precedence against a literal table written from the
six-point list of the header's comment; the enum against Handle.ADJOINT_LOOP_NAMES.  Integers and strings are compared
exactly.  The program is built twice: -O2, and under AddressSanitizer + UBSan.  No GPU needed."""
import itertools, os, re, subprocess, textwrap
import pytest

import wide_chain_adjoint_cases as WA
import wide_chain_cases as WC
import wide_chain_discrete_cases as WD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = textwrap.dedent(r'''
    #include "lrnde_adj_route.hpp"
    #include <cstdio>
    using namespace lrnde;
    // S <the eleven numbers of AdjDevSizes>                       sets the sizes of the cases that follow
    // R | G0..G3, then field adj_loop sensealg sharded adj_host qvjp B D P wfloats gfloats vjp_lds bufw partcap recfloats ndims dims...
    //   R: adj_route; G0..G3: chain_device_gate, chain_discrete_gate, wide_device_gate, wide_discrete_gate alone
    // E                                                           the enum's values beside the binding's names
    int main() {
      AdjDevSizes dev;
      char kind[4];
      while (scanf("%3s", kind) == 1) {
        if (kind[0] == 'E') {
          printf("host %d device %d chain_device %d wide_device %d chain_discrete %d wide_discrete %d\n", (int)ADJ_ROUTE_HOST, (int)ADJ_ROUTE_MLP_DEVICE,
                 (int)ADJ_ROUTE_CHAIN_DEVICE, (int)ADJ_ROUTE_WIDE_DEVICE, (int)ADJ_ROUTE_CHAIN_DISCRETE, (int)ADJ_ROUTE_WIDE_DISCRETE);
          continue;
        }
        if (kind[0] == 'S') {
          if (scanf("%d %d %d %d %d %d %zu %zu %zu %zu %zu", &dev.chain_tile, &dev.wide_tile, &dev.mu_block, &dev.wadj_slots, &dev.wdisc_slots,
                    &dev.wdisc_vecs, &dev.ctrl_bytes, &dev.chadj_tail, &dev.chdisc_tail, &dev.wide_tail, &dev.wadj_tail) != 11) return 2;
          continue;
        }
        AdjRouteIn in;
        int sharded = 0, adj_host = 0, qvjp = 0, ndims = 0;
        if (scanf("%d %d %d %d %d %d %d %d %zu %d %d %zu %d %d %d %d", &in.field, &in.adj_loop, &in.sensealg, &sharded, &adj_host, &qvjp, &in.B, &in.D,
                  &in.P, &in.wfloats, &in.gfloats, &in.vjp_lds, &in.bufw, &in.partcap, &in.recfloats, &ndims) != 16) return 2;
        in.sharded = sharded != 0; in.adj_host = adj_host != 0; in.qvjp = qvjp != 0;
        in.dims.resize((size_t)ndims);
        for (int& d : in.dims) if (scanf("%d", &d) != 1) return 2;
        in.dev = dev;
        AdjPlan pl;
        std::string why;
        bool ok;
        if (kind[0] == 'R') {
          const int rc = adj_route(in, &pl, &why);
          if (rc != LRNDE_OK && rc != LRNDE_UNSUPPORTED) return 3;
          ok = rc == LRNDE_OK;
        } else if (kind[0] == 'G') {
          switch (kind[1]) {
            case '0': ok = chain_device_gate(in, &pl, &why); break;
            case '1': ok = chain_discrete_gate(in, &pl, &why); break;
            case '2': ok = wide_device_gate(in, &pl, &why); break;
            case '3': ok = wide_discrete_gate(in, &pl, &why); break;
            default: return 2;
          }
        } else return 2;
        if (ok) printf("OK %d %d %d %d %d %d %d %zu %zu %zu\n", (int)pl.route, pl.nwg, pl.nmu, pl.nitems, pl.wg_lds, pl.p_lds, pl.partcap, pl.lds,
                       pl.rec_floats, pl.vec_floats);
        else printf("NO %s\n", why.c_str());
      }
      return 0;
    }
''')
PLAN_FIELDS = ("route", "nwg", "nmu", "nitems", "wg_lds", "p_lds", "partcap", "lds", "rec_floats", "vec_floats")


@pytest.fixture(scope="module", params=["O2", "sanitized"])
def driver(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("adj_route_" + request.param)
    src = d / "t.cpp"
    src.write_text(SRC)
    exe = d / "t"
    flags = ["-O2"] if request.param == "O2" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                   "-static-libasan", "-static-libubsan"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)

    def run(cases):
        """cases: [(kind, dict of AdjRouteIn's fields)] -> per case a dict of the plan's fields, or the refusal's text"""
        text = "S %d %d %d %d %d %d %d %d %d %d %d\n" % DEV_SIZES + "".join(line(k, c) for k, c in cases)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out = r.stdout.split("\n")
        assert len(out) == len(cases) + 1 and out[-1] == ""
        return [dict(zip(PLAN_FIELDS, map(int, ln.split()[1:]))) if ln.startswith("OK ") else ln[3:] for ln in out[:-1]]
    run.raw = lambda text: subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
    return run


# ---- the numbers the device headers own, as the restatements and the kernels' comments quote them ----
CNB = 8                                                  # batch columns of a small-chain workgroup (lrnde_chain.hpp)
CHADJ_TAIL = WC.NW * 3 * 8 + WA.CTRL_BYTES + 32          # k_chadj_step: fp64 reduction scratch, the control block, padding
CHDISC_TAIL = 32                                         # k_chain_dsweep: padding
DEV_SIZES = (CNB, WC.NB, WA.MB, WA.SLOTS, WD.SLOTS, WD.VECS, WA.CTRL_BYTES, CHADJ_TAIL, CHDISC_TAIL, WC.LDS_TAIL, WC.LDS_TAIL + WA.CTRL_BYTES)
LDS_MAX = 160 * 1024                                     # CHADJ_LDS_MAX
MAX_WG = 4096                                            # CHADJ_MAX_WG
SCRATCH_MAX = 256 << 20                                  # CHADJ_SCRATCH_MAX
MAX_MU_BLOCKS = 256
AUTO, DEVICE, DISCRETE = 0, 1, 2                         # include/lrnde.h LRNDE_ADJ_LOOP_*
INTERPOLATING, SENSE_DISCRETE = 0, 1                     # LRNDE_SENSE_*
ORDER = ("field", "adj_loop", "sensealg", "sharded", "adj_host", "qvjp", "B", "D", "P", "wfloats", "gfloats", "vjp_lds", "bufw", "partcap",
         "recfloats")


def line(kind, c):
    dims = c.get("dims", [])
    return kind + " " + " ".join(str(int(c.get(k, 0))) for k in ORDER) + " %d " % len(dims) + " ".join(map(str, dims)) + "\n"


def wide_in(dims, B, **kw):
    return dict(field=2, B=B, D=dims[0], bufw=WC.ceil16(max(dims)) * WC.NB, partcap=WC.partcap(dims), recfloats=WA.rec_floats(dims),
                dims=list(dims), **kw)


def small_in(wfloats, gfloats, vjp_lds, P, B, **kw):
    return dict(field=1, B=B, D=1, P=P, wfloats=wfloats, gfloats=gfloats, vjp_lds=vjp_lds, **kw)


def limit_of(text):
    """the limit a refusal names: the one that is followed by ' is <number>'"""
    m = re.findall(r"([A-Z_]+_MAX(?:_WG)?) is \d+", text)
    assert len(m) == 1, text
    return m[0]


# ---- the wide gates against wide_chain_adjoint_cases.gate / wide_chain_discrete_cases.gate ----
def wide_cases(P):
    """every (dims, B) the two host tests of the wide routes assert on, and every shape at its own boundary of either gate"""
    mnist3, full, w1024, narrow = [784, 100, 100, 784], [1024, 1024, 1024], [1024, 16, 1024], [20, 40, 20]
    assert WC.model_dims(WC.shapes(P)[WD.REFUSED_SHAPE]) == w1024
    cases = [(mnist3, 512), (full, 102 * 16), (full, 102 * 16 + 1), (w1024, 2032), (w1024, 2033), (narrow, 4096 * 16), (narrow, 4096 * 16 + 1)]
    for mod in (WA, WD):
        for model in WC.shapes(P).values():
            dims = WC.model_dims(model)
            b = mod.first_refused_batch(dims)
            cases += [(dims, b - 1), (dims, b)]
    assert WA.first_refused_batch(full) == 1633 and WD.first_refused_batch(w1024) == 2033
    return cases


@pytest.mark.parametrize("which", ["device", "discrete"])
def test_wide_gates_equal_their_restatements(driver, which, P):
    mod, gate_kind, loop, route, prefix = ((WA, "G2", DEVICE, 3, "wide adjoint loop: ") if which == "device" else
                                           (WD, "G3", DISCRETE, 5, "wide discrete adjoint: "))
    cases = wide_cases(P)
    alone = driver([(gate_kind, wide_in(d, B)) for d, B in cases])
    routed = driver([("R", wide_in(d, B, adj_loop=loop)) for d, B in cases])
    seen = set()
    for (dims, B), got, via in zip(cases, alone, routed):
        g = mod.gate(dims, B)
        seen.add(g["why"])
        if g["fits"]:
            assert isinstance(got, dict), (dims, B, got)
            assert (got["nwg"], got["nitems"], got["nmu"], got["lds"]) == (g["nwg"], g["nitems"], g["nmu"], g["lds"]), (dims, B, got, g)
            if which == "device":
                assert got["rec_floats"] == WA.SLOTS * g["nwg"] * WA.rec_floats(dims) and got["vec_floats"] == 0
                assert got["rec_floats"] * 4 + 2 * WA.CTRL_BYTES + 5 * (got["nwg"] + got["nmu"]) * 8 == g["bytes"]
                assert got["partcap"] == (g["lds"] - 2 * WC.ceil16(max(dims)) * WC.NB * 4 - WC.LDS_TAIL - WA.CTRL_BYTES) // 4
            else:
                assert got["rec_floats"] == WD.SLOTS * g["nwg"] * WA.rec_floats(dims) and got["vec_floats"] == WD.VECS * B * dims[0]
                assert (got["rec_floats"] + got["vec_floats"]) * 4 == g["bytes"] and got["partcap"] == 0
            assert got["wg_lds"] == got["p_lds"] == 0 and got["route"] == 0
            assert via == dict(got, route=route), (dims, B, via)
        else:
            assert isinstance(got, str) and limit_of(got) == g["why"], (dims, B, got, g)
            want = {"WIDE_LDS_MAX": "the step kernel needs %d bytes of LDS, WIDE_LDS_MAX is %d" % (g["lds"], WC.WIDE_LDS_MAX),
                    "CHADJ_MAX_WG": "B = %d is %d workgroups, CHADJ_MAX_WG is %d" % (B, g["nwg"], mod.MAX_WG),
                    "WIDE_SCRATCH_MAX": ("B = %d needs %d bytes of stage records (%d slots), WIDE_SCRATCH_MAX is %d" % (B, g["bytes"], WA.SLOTS, WA.SCRATCH_MAX)
                                         if which == "device" else
                                         "B = %d needs %d bytes of stage records (%d slots) and sweep vectors (%d), WIDE_SCRATCH_MAX is %d"
                                         % (B, g["bytes"], WD.SLOTS, WD.VECS, WD.SCRATCH_MAX))}[g["why"]]
            assert got == want and via == prefix + want, (dims, B, got, via)
    assert {None, "CHADJ_MAX_WG", "WIDE_SCRATCH_MAX"} <= seen


def test_wide_gates_refuse_an_lds_overrun_and_the_wrong_handle(driver):
    """no chain lrnde_create_wide_chain accepts misses WIDE_LDS_MAX (the create cuts the partial region to fit), so that limit
    is reached with numbers: a partial region one 256-float block too long for the discrete gate (which takes the forward
    kernels' carve as it is), and for the device gate (which cuts it back itself) buffers that alone are too long"""
    dims = [1024, 1024, 1024]
    base = wide_in(dims, 16)
    room = (WC.WIDE_LDS_MAX - 2 * base["bufw"] * 4 - WC.LDS_TAIL) // 4
    fit, over = driver([("G3", dict(base, partcap=room)), ("G3", dict(base, partcap=room + 1))])
    assert fit["lds"] == WC.WIDE_LDS_MAX - (WC.WIDE_LDS_MAX - WC.LDS_TAIL) % 4
    assert over == "the step kernel needs %d bytes of LDS, WIDE_LDS_MAX is %d" % (fit["lds"] + 4, WC.WIDE_LDS_MAX)
    # the device gate gives the control block its room out of the partial region, in blocks of 256 floats
    cut = driver([("G2", dict(base, partcap=room))])[0]
    assert cut["partcap"] == ((room * 4 - WA.CTRL_BYTES) // 4) & ~255 and cut["lds"] == 2 * base["bufw"] * 4 + 4 * cut["partcap"] + WC.LDS_TAIL + WA.CTRL_BYTES
    bufw = (WC.WIDE_LDS_MAX - WC.LDS_TAIL - WA.CTRL_BYTES) // 8
    fit, over = driver([("G2", dict(base, bufw=bufw, partcap=0)), ("G2", dict(base, bufw=bufw + 1, partcap=0))])
    assert fit["lds"] == 8 * bufw + WC.LDS_TAIL + WA.CTRL_BYTES <= WC.WIDE_LDS_MAX and fit["partcap"] == 0
    assert over == "the step kernel needs %d bytes of LDS, WIDE_LDS_MAX is %d" % (fit["lds"] + 8, WC.WIDE_LDS_MAX)
    # the gates name the handle they are for
    small = small_in(1000, 900, 4096, 1000, 8)
    assert driver([("G2", small), ("G3", small), ("G0", base), ("G1", base), ("G3", dict(base, sharded=1)), ("G1", dict(small, sharded=1))]) == \
        ["not a wide-chain handle"] * 2 + ["not a small Dense-chain handle"] * 2 + ["the handle is sharded"] * 2


# ---- the small gates: their arithmetic, written out from the formulas ----
def r4(n):
    return (n + 3) & ~3


def small_lds(wfloats, gfloats, pfloats, vjp_lds, tail):
    """forward image, then the backward image and the parameter partial where they are in LDS (each rounded up to 4 floats),
    the VJP's activation record, the kernel's tail"""
    return (wfloats + r4(gfloats) + r4(pfloats)) * 4 + vjp_lds + tail


def small_gate(which, wfloats, gfloats, vjp_lds, P, B):
    """dict(fits, why, nwg, nmu, wg_lds, p_lds, lds, bytes).  device: the step kernel keeps the forward image and, when it
    fits too, the backward image; 7 x workgroups x P floats of parameter cotangents.  discrete: forward image; plus the
    backward image; plus the workgroup's parameter partial; workgroups x P floats of partials."""
    nwg = -(-B // CNB)
    tail = CHADJ_TAIL if which == "device" else CHDISC_TAIL
    tiers = [small_lds(wfloats, 0, 0, vjp_lds, tail), small_lds(wfloats, gfloats, 0, vjp_lds, tail)]
    if which == "discrete":
        tiers.append(small_lds(wfloats, gfloats, P, vjp_lds, tail))
    nbytes = (7 if which == "device" else 1) * nwg * P * 4
    why = "CHADJ_LDS_MAX" if tiers[0] > LDS_MAX else "CHADJ_MAX_WG" if nwg > MAX_WG else "CHADJ_SCRATCH_MAX" if nbytes > SCRATCH_MAX else None
    wg_lds = int(tiers[1] <= LDS_MAX)
    p_lds = int(which == "discrete" and tiers[2] <= LDS_MAX)
    return dict(fits=why is None, why=why, nwg=nwg, nmu=min(-(-P // 64), MAX_MU_BLOCKS) if which == "device" else 0, wg_lds=wg_lds, p_lds=p_lds,
                lds=tiers[2] if p_lds else tiers[1] if wg_lds else tiers[0], bytes=nbytes, lds0=tiers[0])


# Chain(Dense(128, 96, tanh), Dense(96, 128)) of tests/test_gpu_chain_adjoint.py: 99.2 KB of forward image, 26.6 KB of
# activation record, 98.3 KB of backward image, P = 24800
PHYSIO = dict(wfloats=24800, gfloats=24576, vjp_lds=((128 + 96) + (96 + 128) + 128 + 2 * 128) * 8 * 4, P=24800, B=12)


def small_cases(which):
    """(name, inputs, what the pair is there for): each tier of the LDS plan, and at every limit the last input that fits
    and the first that does not"""
    tail = CHADJ_TAIL if which == "device" else CHDISC_TAIL
    vjp = 8192
    room = (LDS_MAX - vjp - tail) // 4          # floats of images (and partial) that fit
    assert (LDS_MAX - vjp - tail) % 4 == 0
    c = [("physionet", dict(PHYSIO))]
    wf = 20000 + room % 4                       # (what is left beside it is a multiple of 4 floats: the images' rounding)
    # tier 0 | 1: the backward image fills LDS to the byte, then is one float longer (its rounding takes four)
    c += [("bwd_image_last", dict(wfloats=wf, gfloats=room - wf, vjp_lds=vjp, P=100 if which == "device" else room, B=9)),
          ("bwd_image_first_out", dict(wfloats=wf, gfloats=room - wf + 1, vjp_lds=vjp, P=100 if which == "device" else room, B=9))]
    if which == "discrete":   # tier 1 | 2: the parameter partial beside both images
        c += [("partial_last", dict(wfloats=wf, gfloats=9000, vjp_lds=vjp, P=room - wf - 9000, B=9)),
              ("partial_first_out", dict(wfloats=wf, gfloats=9000, vjp_lds=vjp, P=room - wf - 9000 + 1, B=9))]
    # CHADJ_LDS_MAX: the forward image alone
    c += [("lds_last", dict(wfloats=room, gfloats=4, vjp_lds=vjp, P=64, B=8)), ("lds_first_out", dict(wfloats=room + 1, gfloats=4, vjp_lds=vjp, P=64, B=8))]
    # CHADJ_MAX_WG: one column past 4096 tiles of 8
    c += [("wg_last", dict(wfloats=1000, gfloats=900, vjp_lds=vjp, P=100, B=MAX_WG * CNB)),
          ("wg_first_out", dict(wfloats=1000, gfloats=900, vjp_lds=vjp, P=100, B=MAX_WG * CNB + 1))]
    # CHADJ_SCRATCH_MAX: 7 x nwg x P floats (device) / nwg x P floats (discrete); one float of P apart, then one column of B apart
    per = 7 if which == "device" else 1
    pmax = SCRATCH_MAX // (4 * per)
    c += [("scratch_last_P", dict(wfloats=1000, gfloats=900, vjp_lds=vjp, P=pmax, B=8)),
          ("scratch_first_out_P", dict(wfloats=1000, gfloats=900, vjp_lds=vjp, P=pmax + 1, B=8)),
          ("scratch_last_B", dict(wfloats=1000, gfloats=900, vjp_lds=vjp, P=pmax // 2, B=16)),
          ("scratch_first_out_B", dict(wfloats=1000, gfloats=900, vjp_lds=vjp, P=pmax // 2, B=17))]
    return c


@pytest.mark.parametrize("which", ["device", "discrete"])
def test_small_gates_equal_their_arithmetic(driver, which):
    cases = small_cases(which)
    got = driver([("G0" if which == "device" else "G1", small_in(**c)) for _n, c in cases])
    want = {n: small_gate(which, **c) for n, c in cases}
    # what the cases were chosen for, from the restatement alone
    tiers = lambda n: (want[n]["fits"], want[n]["wg_lds"], want[n]["p_lds"])
    assert tiers("bwd_image_last") == (True, 1, 0) and tiers("bwd_image_first_out") == (True, 0, 0) and want["bwd_image_last"]["lds"] == LDS_MAX
    if which == "discrete":
        assert tiers("partial_last") == (True, 1, 1) and tiers("partial_first_out") == (True, 1, 0) and want["partial_last"]["lds"] == LDS_MAX
    assert want["lds_last"]["fits"] and want["lds_last"]["lds0"] == LDS_MAX and want["lds_first_out"]["why"] == "CHADJ_LDS_MAX"
    assert want["wg_last"]["fits"] and want["wg_last"]["nwg"] == MAX_WG and want["wg_first_out"]["why"] == "CHADJ_MAX_WG"
    for k in "PB":
        assert want["scratch_last_" + k]["fits"] and want["scratch_first_out_" + k]["why"] == "CHADJ_SCRATCH_MAX"
        assert want["scratch_last_" + k]["bytes"] <= SCRATCH_MAX < want["scratch_first_out_" + k]["bytes"]
    # the PhysioNet numbers of tests/test_gpu_chain_adjoint.py: 99.2 + 26.6 + 0.4 KB without the backward image, 224 KB with it
    w = want["physionet"]
    if which == "device":
        assert w["lds"] == 99200 + 26624 + 436 == 126260 and (w["wg_lds"], w["nwg"], w["nmu"]) == (0, 2, 256) and w["fits"]
        assert w["lds"] + 24576 * 4 > LDS_MAX
    else:
        assert w["lds"] == 99200 + 26624 + 32 and (w["wg_lds"], w["p_lds"], w["nwg"]) == (0, 0, 2) and w["fits"]
    for (name, c), g in zip(cases, got):
        w = want[name]
        if w["fits"]:
            assert isinstance(g, dict), (name, g)
            assert {k: g[k] for k in ("nwg", "nmu", "wg_lds", "p_lds", "lds")} == {k: w[k] for k in ("nwg", "nmu", "wg_lds", "p_lds", "lds")}, (name, g, w)
            assert g["nitems"] == g["partcap"] == g["rec_floats"] == g["vec_floats"] == 0
        else:
            assert isinstance(g, str) and limit_of(g) == w["why"], (name, g, w)
            if which == "discrete":   # the texts a caller sees
                assert g == {"CHADJ_LDS_MAX": "the sweep needs %d bytes of LDS, CHADJ_LDS_MAX is %d" % (w["lds0"], LDS_MAX),
                             "CHADJ_MAX_WG": "B = %d is %d workgroups, CHADJ_MAX_WG is %d" % (c["B"], w["nwg"], MAX_WG),
                             "CHADJ_SCRATCH_MAX": "B = %d needs %d bytes of parameter partials, CHADJ_SCRATCH_MAX is %d"
                                                  % (c["B"], w["bytes"], SCRATCH_MAX)}[w["why"]], (name, g)


# ---- the route table ----
# Rows (field, adj_loop, sensealg, sharded, LRNDE_ADJ_HOST, 4-column VJP, the sizes pass the gate concerned) -> the route, or
# the refusal's beginning; A: any value; the first row that matches a case is its answer.  Written from the six points:
A = None
ROUTE_TABLE = [
    # 1. wide handle, DEVICE, not sharded, LRNDE_ADJ_HOST off: the wide device gate decides
    ((2, DEVICE, A, 0, 0, A, 1), 3),
    ((2, DEVICE, A, 0, 0, A, 0), "wide adjoint loop: B = "),
    # 2. wide handle, DISCRETE: the wide discrete gate decides, LRNDE_ADJ_HOST or not
    ((2, DISCRETE, A, 1, A, A, A), "wide discrete adjoint: the handle is sharded"),
    ((2, DISCRETE, A, 0, A, A, 1), 5),
    ((2, DISCRETE, A, 0, A, A, 0), "wide discrete adjoint: B = "),
    # 3. sensealg DISCRETE: the small discrete gate decides (the setter refuses it on the other handles: so does the call)
    ((0, A, SENSE_DISCRETE, A, A, A, A), "discrete adjoint: not a small Dense-chain handle"),
    ((2, A, SENSE_DISCRETE, A, A, A, A), "discrete adjoint: not a small Dense-chain handle"),
    ((1, A, SENSE_DISCRETE, 1, A, A, A), "discrete adjoint: the handle is sharded"),
    ((1, A, SENSE_DISCRETE, 0, A, A, 1), 4),
    ((1, A, SENSE_DISCRETE, 0, A, A, 0), "discrete adjoint: B = "),
    # 4. small chain, not sharded, LRNDE_ADJ_HOST off, the small device gate passes (adj_loop is ignored)
    ((1, A, INTERPOLATING, 0, 0, A, 1), 2),
    # 5. the 4-column VJP runs, not sharded, LRNDE_ADJ_HOST off
    ((A, A, INTERPOLATING, 0, 0, 1, A), 1),
    # 6. the host loop: a sharded handle, LRNDE_ADJ_HOST, a wide handle left on AUTO, a small chain outside its gate, ...
    ((A, A, INTERPOLATING, A, A, A, A), 0),
]
# the two cases that need care, and the combinations the setters refuse, spelled out in full
SPOT = {
    (1, DISCRETE, INTERPOLATING, 0, 0, 0, 1): 2, (0, DISCRETE, INTERPOLATING, 0, 0, 1, 1): 1, (0, DISCRETE, INTERPOLATING, 0, 0, 0, 1): 0,
    (2, DEVICE, INTERPOLATING, 1, 0, 0, 1): 0, (2, DEVICE, INTERPOLATING, 0, 1, 0, 1): 0, (2, DEVICE, INTERPOLATING, 1, 0, 0, 0): 0,
    (2, DISCRETE, INTERPOLATING, 0, 1, 0, 1): 5,
    (0, AUTO, SENSE_DISCRETE, 0, 0, 1, 1): "discrete adjoint: not a small Dense-chain handle",
    (2, AUTO, SENSE_DISCRETE, 0, 0, 0, 1): "discrete adjoint: not a small Dense-chain handle",
    (1, AUTO, SENSE_DISCRETE, 0, 1, 0, 1): 4,
}


def table_answer(case):
    hits = [ans for pat, ans in ROUTE_TABLE if all(p is A or p == v for p, v in zip(pat, case))]
    assert hits, case
    return hits[0]


def test_route_table(driver):
    small_pass, small_fail = small_in(**PHYSIO), small_in(**dict(PHYSIO, B=MAX_WG * CNB + 1))
    wide_pass, wide_fail = wide_in([784, 100, 100, 784], 512), wide_in([20, 40, 20], MAX_WG * WC.NB + 1)
    mlp = dict(field=0, B=512, D=784, P=157684)
    sizes = {0: (mlp, mlp), 1: (small_fail, small_pass), 2: (wide_fail, wide_pass)}
    combos = list(itertools.product((0, 1, 2), (AUTO, DEVICE, DISCRETE), (INTERPOLATING, SENSE_DISCRETE), (0, 1), (0, 1), (0, 1), (0, 1)))
    assert len(combos) == 3 * 3 * 2 * 2 * 2 * 2 * 2 and set(SPOT) <= set(combos)
    got = driver([("R", dict(sizes[f][fits], adj_loop=loop, sensealg=sense, sharded=sh, adj_host=host, qvjp=q)) for f, loop, sense, sh, host, q, fits in combos])
    routes = set()
    for case, g in zip(combos, got):
        want = table_answer(case)
        if case in SPOT:
            assert SPOT[case] == want, case
        if isinstance(want, int):
            assert isinstance(g, dict) and g["route"] == want, (case, g, want)
            routes.add(want)
            if want < 2:   # no plan beside the route
                assert all(g[k] == 0 for k in PLAN_FIELDS[1:]), (case, g)
        else:
            assert isinstance(g, str) and g.startswith(want), (case, g, want)
            if want.endswith("B = "):
                assert limit_of(g) == "CHADJ_MAX_WG", (case, g)
    assert routes == {0, 1, 2, 3, 4, 5}


def test_enum_values_are_the_bindings_indices(driver):
    from localregneuralde_jl_amd.layers import Handle
    words = driver.raw("E\n").split()
    assert dict(zip(words[0::2], map(int, words[1::2]))) == {n: i for i, n in enumerate(Handle.ADJOINT_LOOP_NAMES)}
    assert len(Handle.ADJOINT_LOOP_NAMES) == 6


@pytest.fixture(scope="module")
def P():
    import lrnde_amd
    return lrnde_amd
