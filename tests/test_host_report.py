"""csrc/lrnde_report.hpp on the host: the three report layouts the device-controlled loops post to pinned memory, the one
bounded wait of their host drivers, the forward loop's feed rule, the adjoint drivers' trace cursor, and the status ->
retcode / stats mapping, against a restatement in Python written from the layout comments (it does not read the header).
The wait runs in a scripted world — what ready() and query() answer and how the clock moves are the test's — because its
late, drained, error and hung branches cannot be run on a GPU.  The program is built twice: -O2, and under
AddressSanitizer + UBSan."""
import math, os, subprocess, textwrap
import numpy as np
import pytest

from np_restatement import _eps, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RUNNING, DONE = 0, 100
OK, MAXITERS, DT_LESS_THAN_MIN, DT_NAN, BADARG, CAPACITY, HIP_ERROR, NCCL_ERROR, UNSUPPORTED = range(9)   # include/lrnde.h
STATUSES = [RUNNING, MAXITERS, DT_LESS_THAN_MIN, DT_NAN, BADARG, CAPACITY, HIP_ERROR, NCCL_ERROR, UNSUPPORTED, DONE]

SRC = textwrap.dedent(r'''
    #include "lrnde_report.hpp"
    #include <cstdio>
    #include <cstring>
    #include <utility>
    #include <vector>
    using namespace lrnde;
    static float rd() { unsigned u = 0; if (scanf("%x", &u) != 1) u = 0; float x; memcpy(&x, &u, 4); return x; }
    static unsigned bits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
    // the scripted world of a wait: every ready() call takes `step` us; it answers true from call `ready_at` on (0: never)
    // or once `ready_after_q` queries have been made (0: never); query k answers q[k] (the last one for ever) after taking
    // its own jump of the clock
    struct World {
      long long t = 0, step = 0; long calls = 0, ready_at = 0; int queries = 0, ready_after_q = 0;
      std::vector<std::pair<int, long long>> q;
      bool ready() { ++calls; t += step; return (ready_at > 0 && calls >= ready_at) || (ready_after_q > 0 && queries >= ready_after_q); }
      int query() {
        const size_t k = (size_t)queries++;
        if (k < q.size()) t += q[k].second;
        return q[k < q.size() ? k : q.size() - 1].first;
      }
    };
    struct WorldClock { const World* w; long long operator()() const { return w->t; } };
    int main() {
      char kind[4];
      while (scanf("%3s", kind) == 1) {
        if (kind[0] == 'R') {   // R j status nsaved steps_left -> the word; launches status nsaved rem
          int j, status, nsaved;
          if (scanf("%d %d %d", &j, &status, &nsaved) != 3) return 2;
          const unsigned long long w = solve_report_pack(solve_report(j, status, nsaved, rd()));
          const SolveReport r = solve_report_unpack(w);
          printf("%016llx %d %d %d %d\n", w, r.launches, r.status, r.nsaved, r.rem);
        } else if (kind[0] == 'D') {   // D count status -> the word; count status
          unsigned count, status;
          if (scanf("%u %u", &count, &status) != 2) return 2;
          const unsigned long long w = sde_report_pack(count, status);
          printf("%016llx %u %u\n", w, sde_report_unpack(w).count, sde_report_unpack(w).status);
        } else if (kind[0] == 'A') {   // A extra_nf words[ADJ_R_LEN] -> the report's fields; the stats filled from it
          int extra; int hs[ADJ_R_LEN];
          if (scanf("%d", &extra) != 1) return 2;
          for (int& x : hs) if (scanf("%x", (unsigned*)&x) != 1) return 2;
          const AdjReport r = adj_report_read(hs);
          printf("%d %08x %08x %d %d %d %d %d %08x %08x %d\n", r.status, bits(r.t), bits(r.dt), r.cur, r.nf, r.naccept, r.nreject, r.iter,
                 bits(r.eest_last), bits(r.dt_init), r.ovl_timeout);
          lrnde_stats st;
          memset(&st, 0xff, sizeof(st));
          st.nsaved = 0;
          adj_stats_fill(r, extra, &st);
          printf("%d %d %d %d %d %d %08x %08x %08x %08x\n", st.retcode, st.nf, st.naccept, st.nreject, st.iters, st.nsaved, bits(st.t_final),
                 bits(st.dt_final), bits(st.eest_last), bits(st.dt_init));
        } else if (kind[0] == 'C') {   // C status -> retcode
          int status;
          if (scanf("%d", &status) != 1) return 2;
          printf("%d\n", status_retcode(status));
        } else if (kind[0] == 'F') {   // F rem seen fT fE fM -> ahead certain
          int rem, seen, fT, fE, fM;
          if (scanf("%d %d %d %d %d", &rem, &seen, &fT, &fE, &fM) != 5) return 2;
          const Feed f = feed_rule(rem, seen, fT, fE, fM);
          printf("%d %d\n", f.ahead, f.certain);
        } else if (kind[0] == 'L') {   // L t dt s1 -> maybe last
          const float t = rd(), dt = rd(), s1 = rd();
          printf("%d\n", adj_maybe_last(t, dt, s1) ? 1 : 0);
        } else if (kind[0] == 'T') {   // T cap n0 nrep (status t dt naccept eest)[nrep] -> n; the rows
          int cap, n, nrep;
          if (scanf("%d %d %d", &cap, &n, &nrep) != 3) return 2;
          std::vector<lrnde_trace_row> rows((size_t)cap + 1);   // (exactly cap rows and a guard: ASan sees a row too many)
          for (auto& r : rows) { r.t = r.dt = r.eest = -7.f; r.accepted = -7; }
          AdjTraceCursor k;
          for (int j = 1; j <= nrep; ++j) {
            AdjReport r{};
            if (scanf("%d", &r.status) != 1) return 2;
            r.t = rd(); r.dt = rd();
            if (scanf("%d", &r.naccept) != 1) return 2;
            r.eest_last = rd();
            adj_trace_report(k, j, r, rows.data(), n, cap);
          }
          printf("%d\n", n);
          for (int i = 0; i <= cap; ++i) printf("%08x %08x %08x %d\n", bits(rows[i].t), bits(rows[i].dt), bits(rows[i].eest), rows[i].accepted);
        } else if (kind[0] == 'W' || kind[0] == 'N') {
          // W every stall_us step ready_at ready_after_q nq (result jump)[nq] -> result code queries ready-calls
          // N ... the same, and n2 before it: the FIRST query of this wait first runs a second wait in the same world, ready at
          //   its call n2 -> the second's result and queries, then the line of the first
          long n2 = 0;
          if (kind[0] == 'N' && scanf("%ld", &n2) != 1) return 2;
          WaitCadence cad; World w; int nq;
          if (scanf("%ld %lld %lld %ld %d %d", &cad.every, &cad.stall_us, &w.step, &w.ready_at, &w.ready_after_q, &nq) != 6) return 2;
          w.q.resize(nq);
          for (auto& e : w.q) if (scanf("%d %lld", &e.first, &e.second) != 2) return 2;
          ReportWait<WorldClock> wait(cad, WorldClock{&w});
          const WaitResult r = wait.await([&] { return w.ready(); }, [&] {
            const int q = w.query();
            if (n2 > 0 && w.queries == 1) {
              ReportWait<WorldClock> second(cad, WorldClock{&w});
              long calls2 = 0; int queries2 = 0;
              const WaitResult r2 = second.await([&] { w.t += w.step; return ++calls2 >= n2; }, [&] { ++queries2; return (int)QUERY_NOT_READY; });
              printf("%d %d\n", (int)r2, queries2);
            }
            return q;
          });
          printf("%d %d %d %ld\n", (int)r, wait.code, w.queries, w.calls);
        } else return 2;
      }
      return 0;
    }
''')


@pytest.fixture(scope="module", params=["O2", "sanitized"])
def driver(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("report_" + request.param)
    src = d / "t.cpp"
    src.write_text(SRC)
    exe = d / "t"
    flags = ["-O2"] if request.param == "O2" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                   "-static-libasan", "-static-libubsan"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", *flags,
                    "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)

    def run(text):
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.split("\n")
    return run


def hx(x):
    return "%08x" % int(np.array([x], dtype=f32).view(np.uint32)[0])


# ---- the layouts, from their comments ----
def ring_word(launches, status, nsaved, steps_left):
    """[rem : 16][nsaved : 16][status : 8][launches : 24]; rem = ceil(steps_left), then the cap at 65535, then the floor 0"""
    sl = float(f32(steps_left))
    rem = 0 if math.isnan(sl) else (65535 if sl == math.inf else (0 if sl == -math.inf else math.ceil(sl)))
    rem = 65535 if rem > 65535 else (rem if rem > 0 else 0)
    fields = (launches & 0xffffff, status & 0xff, min(nsaved, 65535), rem)
    return fields[0] | fields[1] << 24 | fields[2] << 32 | fields[3] << 48, fields


def test_ring_word(driver):
    cases = [(l, s, n, sl) for l in (0, 1, 0xffffff, 0x1000000) for s in STATUSES for n in (0, 1, 65535, 65536)
             for sl in (-1.0, 0.0, 0.2, 1.0, 65535.5, math.inf)]
    cases += [(5, RUNNING, 3, x) for x in (math.nan, -math.inf, 65534.5, 65535.0, 65536.0, 2.0, 2.0000002, 1e30)]
    out = driver("".join("R %d %d %d %s\n" % (l - 1, s, n, hx(sl)) for l, s, n, sl in cases))
    for (l, s, n, sl), ln in zip(cases, out):
        word, fields = ring_word(l, s, n, sl)
        assert ln.split() == ["%016x" % word] + [str(v) for v in fields], ((l, s, n, sl), ln, hex(word), fields)
    # what the cases were chosen for
    assert ring_word(0x1000000, DONE, 0, 0.0)[1][0] == 0, "the launch count wraps at 24 bits"
    assert ring_word(1, DONE, 0, 0.0)[1][1] == 100, "ST_DONE survives the 8-bit field"
    assert ring_word(1, 0, 65536, 0.0)[1][2] == 65535
    assert [ring_word(1, 0, 0, x)[1][3] for x in (-1.0, 0.0, 0.2, 1.0, 65535.5, math.inf)] == [0, 0, 1, 1, 65535, 65535]
    assert ring_word(0xffffff, 0xff, 65535, math.inf)[0] == 2 ** 64 - 1


def test_sde_word(driver):
    cases = [(cnt, s) for cnt in (0, 1, 4, 0x7fffffff, 0xffffffff) for s in STATUSES + [0xffffffff]]
    out = driver("".join("D %d %d\n" % cs for cs in cases))
    for (cnt, s), ln in zip(cases, out):
        assert ln.split() == ["%016x" % (cnt | s << 32), str(cnt), str(s)], (cnt, s, ln)


def test_adjoint_block_and_stats(driver):
    """[0] seq, [1] status, [2] t, [3] dt, [4] cur, [5] nf, [6] naccept, [7] nreject, [8] iter, [9] eest_last, [10] dt_init,
    [11] the overlapped launches' timeout word, 16 words in all; floats as their bits"""
    rng = np.random.default_rng(0)
    for status, extra in ((DONE, 0), (RUNNING, 3), (DT_NAN, 1), (HIP_ERROR, 0)):
        hs = [int(v) for v in rng.integers(1, 2 ** 20, 16)]
        hs[1] = status
        fl = {i: f32(v) for i, v in ((2, -0.375), (3, 0.0123), (9, 0.75), (10, 1e-3))}
        for i, v in fl.items():
            hs[i] = int(np.array([v], f32).view(np.uint32)[0])
        out = driver("A %d %s\n" % (extra, " ".join("%x" % v for v in hs)))
        want = [str(hs[1]), hx(fl[2]), hx(fl[3]), str(hs[4]), str(hs[5]), str(hs[6]), str(hs[7]), str(hs[8]), hx(fl[9]), hx(fl[10]), str(hs[11])]
        assert out[0].split() == want, (out[0], want)
        retcode = OK if status == DONE else (MAXITERS if status == RUNNING else status)
        # retcode, nf (with the driver's own evaluations), naccept, nreject, iters, nsaved (left alone), t, dt, eest_last, dt_init
        assert out[1].split() == [str(retcode), str(hs[5] + extra), str(hs[6]), str(hs[7]), str(hs[8]), "0", hx(fl[2]), hx(fl[3]), hx(fl[9]), hx(fl[10])], out[1]


def test_retcode_mapping(driver):
    out = driver("".join("C %d\n" % s for s in STATUSES))
    want = {s: s for s in STATUSES}
    want[DONE], want[RUNNING] = OK, MAXITERS
    assert [int(x) for x in out[:len(STATUSES)]] == [want[s] for s in STATUSES]


# ---- the wait ----
READY, DRAINED, QUEUE_ERROR, HUNG = 0, 1, 2, 3
Q_DRAINED, Q_NOT_READY = 0, -1
PER_ATTEMPT, PER_LAUNCH = (0x100000, 0), (0x4000, 20000)   # (spins between checks, us without a report before a query)
DEADLINE_US = 90 * 10 ** 6


def wait_restate(cad, step, ready_at, ready_after_q, qscript, t=0):
    """the rule in words: spin on ready(); at every `every`-th failed check — with a stall time, only once that long has
    passed since the wait began or since the last query — ask the queue.  Drained: look once more, ready or drained.  An
    error: returned with its code.  Not ready: hung once more than 90 s have passed since the wait began.
    Stated over check points, not spins.  Returns (result, code, queries, ready calls, end time)."""
    every, stall = cad
    t0 = t_last = t
    calls = fails = queries = 0

    def is_ready(call):
        return (ready_at > 0 and call >= ready_at) or (ready_after_q > 0 and queries >= ready_after_q)
    while True:
        k = every - fails % every   # failed checks up to the next check point
        first = calls + 1 if (ready_after_q > 0 and queries >= ready_after_q) else (max(ready_at, calls + 1) if ready_at > 0 else None)
        if first is not None and first <= calls + k:
            t += (first - calls) * step
            return READY, 0, queries, first, t
        calls += k; fails += k; t += k * step
        if stall:
            if t - t_last < stall:
                continue
            t_last = t
        res, jump = qscript[min(queries, len(qscript) - 1)][0], (qscript[queries][1] if queries < len(qscript) else 0)
        queries += 1
        t += jump
        if res == Q_DRAINED:
            calls += 1; t += step
            return (READY if is_ready(calls) else DRAINED), 0, queries, calls, t
        if res != Q_NOT_READY:
            return QUEUE_ERROR, res, queries, calls, t
        if t - t0 > DEADLINE_US:
            return HUNG, 0, queries, calls, t


def run_wait(driver, cad, step, ready_at=0, ready_after_q=0, qscript=((Q_NOT_READY, 0),)):
    out = driver("W %d %d %d %d %d %d %s\n" % (cad[0], cad[1], step, ready_at, ready_after_q, len(qscript), " ".join("%d %d" % q for q in qscript)))
    got = tuple(int(x) for x in out[0].split())
    want = wait_restate(cad, step, ready_at, ready_after_q, list(qscript))[:4]
    assert got == want, (cad, step, ready_at, ready_after_q, qscript, got, want)
    return got


@pytest.mark.parametrize("cad", [PER_ATTEMPT, PER_LAUNCH])
def test_wait(driver, cad):
    every, stall = cad
    # a step of the clock per spin that makes every check point a query point of the 20-ms cadence too: 2 us x 0x4000 = 32.8 ms
    assert run_wait(driver, cad, 2, ready_at=1) == (READY, 0, 0, 1), "ready at once: no query"
    assert run_wait(driver, cad, 2, ready_at=every) == (READY, 0, 0, every), "ready one spin before the first query point: no query"
    assert run_wait(driver, cad, 2, ready_at=every + 1) == (READY, 0, 1, every + 1), "... and one spin later: one"
    assert run_wait(driver, cad, 2, ready_after_q=1, qscript=[(Q_DRAINED, 0)]) == (READY, 0, 1, every + 1), "drained, the report there on the re-check"
    assert run_wait(driver, cad, 2, qscript=[(Q_DRAINED, 0)]) == (DRAINED, 0, 1, every + 1), "drained without it"
    assert run_wait(driver, cad, 2, qscript=[(Q_NOT_READY, 0), (Q_NOT_READY, 0), (Q_DRAINED, 0)]) == (DRAINED, 0, 3, 3 * every + 1)
    assert run_wait(driver, cad, 2, qscript=[(Q_NOT_READY, 0), (709, 0)]) == (QUEUE_ERROR, 709, 2, 2 * every), "a queue error comes back with its code"
    assert run_wait(driver, cad, 2, qscript=[(1, 0)]) == (QUEUE_ERROR, 1, 1, every)
    # the first query takes the clock to 89.9 s: not hung; the second to just past 90 s: hung (the spins themselves take 2 x
    # 0x100000 x 2 us = 4.2 s at the slower cadence)
    spin_us = 2 * every * 2
    assert run_wait(driver, cad, 2, qscript=[(Q_NOT_READY, 89_900_000 - spin_us), (Q_NOT_READY, 100_001 + spin_us // 2)]) == (HUNG, 0, 2, 2 * every)
    assert run_wait(driver, cad, 2, ready_at=2 * every + 5, qscript=[(Q_NOT_READY, 89_900_000 - spin_us), (Q_NOT_READY, 0)]) == (READY, 0, 2, 2 * every + 5), \
        "not ready at 89.9 s: keeps waiting"
    # exactly 90 s is not yet hung; the query after it is
    assert run_wait(driver, cad, 2, qscript=[(Q_NOT_READY, DEADLINE_US - 2 * every)]) == (HUNG, 0, 2, 2 * every)


def test_wait_20ms_cadence(driver):
    every = PER_LAUNCH[0]
    # under 20 ms however many spins (a clock that does not move): no query
    assert run_wait(driver, PER_LAUNCH, 0, ready_at=40 * every + 3) == (READY, 0, 0, 40 * every + 3)
    # 1 us per spin: check points every 16.4 ms; the first past 20 ms is the second (32.8 ms), then every other one
    assert run_wait(driver, PER_LAUNCH, 1, ready_at=2 * every) == (READY, 0, 0, 2 * every)
    assert run_wait(driver, PER_LAUNCH, 1, ready_at=2 * every + 1) == (READY, 0, 1, 2 * every + 1)
    assert run_wait(driver, PER_LAUNCH, 1, ready_at=10 * every + 1) == (READY, 0, 5, 10 * every + 1), "one query per further 20 ms"
    # 5 us per spin: every check point is 82 ms after the last
    assert run_wait(driver, PER_LAUNCH, 5, ready_at=7 * every + 1) == (READY, 0, 7, 7 * every + 1)
    # the other cadence does not look at the clock
    assert run_wait(driver, PER_ATTEMPT, 0, ready_at=2 * PER_ATTEMPT[0] + 1) == (READY, 0, 2, 2 * PER_ATTEMPT[0] + 1)


def test_second_wait_has_its_own_clock(driver):
    """a wait made while another is stalled (its query took 15 ms, 47.8 ms into the first wait) starts its own 20 ms"""
    every = PER_LAUNCH[0]
    for n2, want2 in ((every + 2000, (READY, 0)), (2 * every + 2000, (READY, 1))):
        out = driver("N %d %d %d 1 0 0 1 %d 15000\n" % (n2, every, PER_LAUNCH[1], Q_DRAINED))
        first = wait_restate(PER_LAUNCH, 1, 0, 0, [(Q_DRAINED, 15000)])
        assert first[:4] == (DRAINED, 0, 1, 2 * every + 1)
        t2 = 2 * every + 15000   # the world's clock when the second wait is made
        second = wait_restate(PER_LAUNCH, 1, n2, 0, [(Q_NOT_READY, 0)], t=t2)
        assert (second[0], second[2]) == want2
        assert tuple(int(x) for x in out[0].split()) == want2, out[0]
        # (the first wait's re-check comes after the second wait's spins: its own count is one ready call more)
        assert tuple(int(x) for x in out[1].split()) == first[:4], out[1]


# ---- the feed rule ----
def feed_restate(rem, seen, fT, fE, fM):
    """near the end (rem <= fT) the estimate is taken whole, plus fE launches that find the solve finished; far from it half
    the estimate, fE and one more; at least fM, at most 16.  Certain: half the estimate beyond `seen`, one at the least"""
    ahead = rem + fE if rem <= fT else rem // 2 + fE + 1
    return min(max(ahead, fM), 16), seen + (rem // 2 if rem > 1 else 1)


@pytest.mark.parametrize("opts", [(3, 1, 2), (100, 1, 2), (0, 0, 1)])
def test_feed_rule(driver, opts):
    cases = [(rem, seen) for rem in range(41) for seen in (0, 1, 7)]
    out = driver("".join("F %d %d %d %d %d\n" % (rem, seen, *opts) for rem, seen in cases))
    for (rem, seen), ln in zip(cases, out):
        assert tuple(int(x) for x in ln.split()) == feed_restate(rem, seen, *opts), (rem, seen, opts, ln)
    assert feed_restate(0, 7, *opts)[0] == opts[2] and feed_restate(40, 0, *opts)[0] == 16, "the floor fM and the cap"
    if opts == (3, 1, 2):
        assert [feed_restate(r, 0, *opts) for r in (1, 3, 4, 40)] == [(2, 1), (4, 1), (4, 2), (16, 20)]


# ---- the adjoint trace cursor ----
def trace_restate(cap, n, reports):
    rows = {}
    prev, nacc = -1, 0
    for j, (status, t, dt, naccept, eest) in enumerate(reports, 1):
        if j > 1 and prev >= 0:
            rows[prev][2:] = [f32(eest), int(naccept > nacc)]
        prev, nacc = -1, naccept
        if status == RUNNING and n < cap:
            prev = n
            rows[n] = [f32(t), f32(dt), f32(0), -1]
            n += 1
    return n, rows


def run_trace(driver, cap, n0, reports):
    out = driver("T %d %d %d %s\n" % (cap, n0, len(reports), " ".join("%d %s %s %d %s" % (s, hx(t), hx(dt), na, hx(e)) for s, t, dt, na, e in reports)))
    n, rows = trace_restate(cap, n0, reports)
    assert int(out[0]) == n
    untouched = [hx(-7.0)] * 3 + ["-7"]
    for i in range(cap + 1):
        want = [hx(rows[i][0]), hx(rows[i][1]), hx(rows[i][2]), str(rows[i][3])] if i in rows else untouched
        assert out[1 + i].split() == want, (i, out[1 + i], want)
    return n, rows


def test_trace_cursor(driver):
    # accept, reject, accept, done: the report of attempt j carries (s, dt) of attempt j and the verdict on attempt j - 1
    script = [(RUNNING, -1.0, 0.1, 0, 0.0), (RUNNING, -0.9, 0.2, 1, 0.5), (RUNNING, -0.9, 0.05, 1, 3.0), (RUNNING, -0.85, 0.07, 2, 0.25), (DONE, 0.0, 0.07, 3, 0.125)]
    n, rows = run_trace(driver, 8, 0, script)
    assert n == 4 and [rows[i][3] for i in range(4)] == [1, 0, 1, 1] and [float(rows[i][2]) for i in range(4)] == [0.5, 3.0, 0.25, 0.125]
    # a second segment appends to the rows of the first, with a cursor of its own
    n, rows = run_trace(driver, 8, 4, script[:2])
    assert n == 6 and sorted(rows) == [4, 5] and rows[5][3] == -1
    # a full array opens no row and back-fills nothing; one that fills up on the way stops there
    assert run_trace(driver, 3, 3, script)[0] == 3
    n, rows = run_trace(driver, 2, 0, script)
    assert n == 2 and rows[1][3] == 0
    # a single attempt: nothing to back-fill, whatever the first report's eest and naccept say
    n, rows = run_trace(driver, 8, 0, [(RUNNING, -1.0, 0.1, 5, 9.0)])
    assert n == 1 and rows[0][2:] == [0.0, -1]
    assert run_trace(driver, 8, 0, [(DT_NAN, -1.0, 0.1, 0, 0.0)])[0] == 0, "an attempt that does not run gets no row"


# ---- the end-of-segment test ----
def test_maybe_last_is_inclusive(driver):
    one, half = f32(1.0), f32(0.5)
    bound = f32(f32(100) * _eps(one))
    te = f32(one - bound)               # an end exactly 100 eps short of the segment's
    assert f32(half + f32(te - half)) == te and f32(one - te) == bound
    below = np.nextafter(te, f32(0))    # one ulp further away
    over = f32(one + bound)             # exactly 100 eps(1) past it: eps at the larger magnitude, the same binade
    cases = [(half, f32(te - half), one, 1), (half, f32(below - half), one, 0), (half, f32(over - half), one, 1),
             (half, half, one, 1), (f32(0.0), f32(0.25), one, 0), (f32(-1.0), f32(te), f32(0.0), 0), (f32(-1.0), one, f32(0.0), 1)]
    out = driver("".join("L %s %s %s\n" % (hx(t), hx(dt), hx(s1)) for t, dt, s1, _ in cases))
    for (t, dt, s1, want), ln in zip(cases, out):
        e = f32(t + dt)
        restated = int(abs(f32(e - s1)) <= f32(f32(100) * _eps(np.fmax(f32(abs(e)), f32(abs(s1))))))
        assert int(ln) == restated == want, (t, dt, s1, ln, restated, want)
