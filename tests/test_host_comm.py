"""csrc/lrnde_comm.hpp on the host: lrnde::Membership (what a handle knows about its communicator: DESIGN.md §5) and the
local communicator's host barrier, compiled with LRNDE_COMM_HOST_TEST against small stand-ins for the HIP and RCCL calls
the header makes and for lc_allreduce, under AddressSanitizer and UBSan.  The stand-ins log their calls in order, the
next ncclCommInitRank / all-reduce / stream drain can be made to fail, and the program exits non-zero at the first broken
claim.  Nothing is loaded into Python."""
import os, subprocess, textwrap
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = textwrap.dedent(r'''
    #include <chrono>
    #include <cstdio>
    #include <cstdlib>
    #include <cstring>
    #include <string>
    #include <thread>
    #include <vector>
    // ---- the HIP and RCCL calls the headers make: on the host heap, logged in order ----
    enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
    enum { hipHostMallocMapped = 2, hipEventDisableTiming = 2 };
    typedef struct ev_* hipEvent_t;
    typedef struct st_* hipStream_t;
    static std::vector<std::string> calls;
    static int live_ev = 0, live_comm = 0, fail_init_next = 0, fail_ar_next = 0, fail_sync_next = 0, lc_rc_next = 0;
    static hipError_t hipMalloc(void** p, size_t bytes) { *p = malloc(bytes ? bytes : 1); return hipSuccess; }
    static hipError_t hipFree(void* p) { free(p); return hipSuccess; }
    static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static hipError_t hipHostFree(void* p) { return hipFree(p); }
    static hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
    static hipError_t hipGetLastError() { return hipSuccess; }
    static const char* hipGetErrorString(hipError_t) { return "stand-in HIP error"; }
    static hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)malloc(1); ++live_ev; calls.push_back("event"); return hipSuccess; }
    static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
    static hipError_t hipEventDestroy(hipEvent_t e) { free(e); --live_ev; return hipSuccess; }
    static hipError_t hipSetDevice(int) { return hipSuccess; }
    static hipError_t drain(const char* what) {
      calls.push_back(what);
      if (fail_sync_next) { fail_sync_next = 0; return hipErrorUnknown; }
      return hipSuccess;
    }
    static hipError_t hipStreamSynchronize(hipStream_t) { return drain("drain"); }
    static hipError_t hipDeviceSynchronize() { return drain("drain-device"); }
    struct comm_ { int n; };
    typedef comm_* ncclComm_t;
    struct ncclUniqueId { char internal[128]; };
    enum ncclResult_t { ncclSuccess = 0, ncclSystemError = 2 };
    enum ncclDataType_t { ncclFloat = 7, ncclDouble = 8 };
    enum ncclRedOp_t { ncclSum = 0 };
    static const char* ncclGetErrorString(ncclResult_t) { return "stand-in RCCL error"; }
    static ncclResult_t ncclCommInitRank(ncclComm_t* c, int n, ncclUniqueId, int) {
      calls.push_back("init");
      if (fail_init_next) { fail_init_next = 0; *c = (ncclComm_t)0x1;   /* a failed call may leave garbage behind */
                            return ncclSystemError; }
      *c = new comm_{n}; ++live_comm; return ncclSuccess;
    }
    static ncclResult_t ncclCommDestroy(ncclComm_t c) { calls.push_back("destroy"); delete c; --live_comm; return ncclSuccess; }
    static ncclResult_t ncclCommCount(ncclComm_t c, int* n) { *n = c->n; return ncclSuccess; }
    static ncclResult_t ncclAllReduce(const void*, void*, size_t, ncclDataType_t t, ncclRedOp_t, ncclComm_t, hipStream_t) {
      calls.push_back(t == ncclDouble ? "rccl-sum-f64" : "rccl-sum-f32");
      if (fail_ar_next) { fail_ar_next = 0; return ncclSystemError; }
      return ncclSuccess;
    }
    #define LRNDE_COMM_HOST_TEST
    #include "lrnde_comm.hpp"
    // the local transport (lrnde_comm.hip's on the GPU)
    int lc_allreduce(lrnde_local_comm*, int, hipStream_t, const void*, void*, size_t, bool is_double) {
      calls.push_back(is_double ? "local-sum-f64" : "local-sum-f32");
      const int rc = lc_rc_next; lc_rc_next = 0; return rc;
    }

    #define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); exit(1); } } while (0)
    using lrnde::Membership;
    static hipStream_t const S = (hipStream_t)0x10;
    static char uid[128];
    static std::string err;

    static int pos(const char* what) {   // first position in the log, -1 when absent
      for (size_t i = 0; i < calls.size(); ++i) if (calls[i] == what) return (int)i;
      return -1;
    }
    static bool counted(const Membership& m, int n_want, int kind_want) {
      int n = -1, kind = -1;
      return m.count(&n, &kind, &err) == LRNDE_OK && n == n_want && kind == kind_want;
    }
    static bool unsharded(const Membership& m) { return !m.sharded() && !m.comm && !m.lcomm && m.rank == 0 && m.nranks == 1 && counted(m, 1, 0); }
    static void free_events(lrnde_local_comm& lc) {   // (lrnde_local_comm_destroy's part)
      for (int r = 0; r < lc.n; ++r) { if (lc.ready[r]) hipEventDestroy(lc.ready[r]); if (lc.done[r]) hipEventDestroy(lc.done[r]); }
    }

    int main() {
      {  // a fresh membership: unsharded, and its all-reduce is nothing at all
        Membership m;
        REQUIRE(unsharded(m));
        float v[4] = {};
        REQUIRE(m.allreduce(S, v, v, 4, false, &err) == LRNDE_OK && m.allreduce(S, v, v, 4, true, &err) == LRNDE_OK);
        REQUIRE(calls.empty() && m.exchanges == 0 && m.bytes == 0);
        REQUIRE(m.leave(S, &err) == LRNDE_OK && calls.empty());   // nothing joined: no drain, no destroy
      }
      {  // join_rccl
        Membership m;
        REQUIRE(m.join_rccl(uid, 0, 1, 8, false, 0, S, &err) == LRNDE_OK);       // one rank, not forced: no communicator
        REQUIRE(unsharded(m) && calls.empty() && live_comm == 0);
        REQUIRE(m.join_rccl(uid, 0, 1, 8, true, 0, S, &err) == LRNDE_OK);        // forced: the sharded code on one rank
        REQUIRE(m.sharded() && m.comm && !m.lcomm && m.rank == 0 && m.nranks == 1 && counted(m, 1, 1));
        REQUIRE(calls.size() == 1 && calls[0] == "init" && live_comm == 1);
        REQUIRE(m.join_rccl(uid, 1, 2, 8, false, 0, S, &err) == LRNDE_OK);       // re-join: drain, destroy, then the new one
        REQUIRE(m.rank == 1 && m.nranks == 2 && counted(m, 2, 1) && live_comm == 1);
        REQUIRE(calls.size() == 4 && calls[1] == "drain" && calls[2] == "destroy" && calls[3] == "init");
        // bad arguments: refused with a message, and nothing changes
        const ncclComm_t held = m.comm;
        struct { const void* uid; int rank, nranks, max; } bad[] = {
            {nullptr, 0, 2, 8}, {uid, -1, 2, 8}, {uid, 2, 2, 8}, {uid, 0, 0, 8}, {uid, 0, -3, 8}, {uid, 0, 9, 8}, {uid, 9, 9, 0}};
        for (auto& b : bad) {
          calls.clear(); err.clear();
          REQUIRE(m.join_rccl(b.uid, b.rank, b.nranks, b.max, true, 0, S, &err) == LRNDE_BADARG);
          REQUIRE(!err.empty() && calls.empty() && m.comm == held && m.rank == 1 && m.nranks == 2 && live_comm == 1);
        }
        // no limit: more ranks than any handle's limit
        calls.clear();
        REQUIRE(m.join_rccl(uid, 40, 1000, 0, false, 0, S, &err) == LRNDE_OK && m.rank == 40 && counted(m, 1000, 1));
        // a failing ncclCommInitRank: what was held is gone, and the membership is an unsharded one
        calls.clear(); err.clear();
        fail_init_next = 1;
        REQUIRE(m.join_rccl(uid, 1, 2, 8, false, 0, S, &err) == LRNDE_NCCL_ERROR);
        REQUIRE(!err.empty() && unsharded(m) && live_comm == 0);
        REQUIRE(calls.size() == 3 && calls[0] == "drain" && calls[1] == "destroy" && calls[2] == "init");
        float v[2] = {};
        calls.clear();
        REQUIRE(m.allreduce(S, v, v, 2, false, &err) == LRNDE_OK && calls.empty() && m.exchanges == 0);
      }
      REQUIRE(live_comm == 0);
      {  // leave: the stream is drained strictly before the communicator goes; a null stream drains the device
        Membership m;
        REQUIRE(m.join_rccl(uid, 1, 2, 8, false, 0, S, &err) == LRNDE_OK);
        calls.clear();
        REQUIRE(m.leave(S, &err) == LRNDE_OK && unsharded(m) && live_comm == 0);
        REQUIRE(calls.size() == 2 && calls[0] == "drain" && calls[1] == "destroy");
        calls.clear();
        REQUIRE(m.leave(S, &err) == LRNDE_OK && calls.empty());
        REQUIRE(m.join_rccl(uid, 0, 2, 8, false, 0, nullptr, &err) == LRNDE_OK);
        calls.clear();
        REQUIRE(m.leave(nullptr, &err) == LRNDE_OK && calls.size() == 2 && calls[0] == "drain-device" && calls[1] == "destroy");
        // a drain that fails: the communicator is kept (work may still be queued on it), the call says so
        REQUIRE(m.join_rccl(uid, 0, 2, 8, false, 0, S, &err) == LRNDE_OK);
        calls.clear(); err.clear();
        fail_sync_next = 1;
        REQUIRE(m.leave(S, &err) == LRNDE_HIP_ERROR && !err.empty() && m.sharded() && live_comm == 1 && pos("destroy") < 0);
        REQUIRE(m.leave(S, &err) == LRNDE_OK && live_comm == 0);
      }
      {  // join_local
        lrnde_local_comm lc;
        lc.n = 2;
        Membership m0, m1, m2, m3;
        calls.clear();
        REQUIRE(m0.join_local(nullptr, 0, 0, S, &err) == LRNDE_BADARG && m0.join_local(&lc, -1, 0, S, &err) == LRNDE_BADARG &&
                m0.join_local(&lc, 2, 0, S, &err) == LRNDE_BADARG);
        REQUIRE(unsharded(m0) && calls.empty() && !lc.joined[0] && !lc.joined[1]);
        REQUIRE(m0.join_local(&lc, 0, 0, S, &err) == LRNDE_OK);
        REQUIRE(m0.sharded() && m0.lcomm == &lc && !m0.comm && m0.rank == 0 && m0.nranks == 2 && counted(m0, 2, 2));
        REQUIRE(lc.joined[0] && lc.device[0] == 0 && lc.ready[0] && lc.done[0] && live_ev == 2 && calls.size() == 2);   // (no drain: nothing was held)
        // a rank already joined
        err.clear();
        REQUIRE(m1.join_local(&lc, 0, 0, S, &err) == LRNDE_BADARG && !err.empty() && unsharded(m1) && live_ev == 2);
        // the same handle, the same communicator, another rank: refused, and it keeps what it has
        err.clear();
        REQUIRE(m0.join_local(&lc, 1, 0, S, &err) == LRNDE_BADARG && !err.empty());
        REQUIRE(m0.lcomm == &lc && m0.rank == 0 && m0.nranks == 2 && !lc.joined[1] && live_ev == 2);
        // a second device
        err.clear();
        REQUIRE(m2.join_local(&lc, 1, 1, S, &err) == LRNDE_UNSUPPORTED && !err.empty() && unsharded(m2) && !lc.joined[1] && live_ev == 2);
        // holding an RCCL communicator: it is drained and destroyed before the rendezvous is joined
        REQUIRE(m3.join_rccl(uid, 0, 2, 8, false, 0, S, &err) == LRNDE_OK && live_comm == 1);
        calls.clear();
        REQUIRE(m3.join_local(&lc, 1, 0, S, &err) == LRNDE_OK);
        REQUIRE(!m3.comm && m3.lcomm == &lc && m3.rank == 1 && m3.nranks == 2 && counted(m3, 2, 2) && live_comm == 0);
        REQUIRE(calls.size() == 4 && calls[0] == "drain" && calls[1] == "destroy" && calls[2] == "event" && calls[3] == "event");
        REQUIRE(lc.joined[1] && live_ev == 4);   // two events per joined rank
        // leaving a rendezvous drains, destroys nothing, and does not give the rank's slot back
        calls.clear();
        REQUIRE(m3.leave(S, &err) == LRNDE_OK && unsharded(m3) && calls.size() == 1 && calls[0] == "drain" && lc.joined[1]);
        REQUIRE(m3.join_local(&lc, 1, 0, S, &err) == LRNDE_BADARG && unsharded(m3));

        // allreduce on the local transport: counters add count * 4 / count * 8; a failure returns its code and counts nothing
        double v[8] = {};
        calls.clear();
        REQUIRE(m0.allreduce(S, v, v, 5, false, &err) == LRNDE_OK && m0.exchanges == 1 && m0.bytes == 20);
        REQUIRE(m0.allreduce(S, v, v, 7, true, &err) == LRNDE_OK && m0.exchanges == 2 && m0.bytes == 20 + 56);
        REQUIRE(calls.size() == 2 && calls[0] == "local-sum-f32" && calls[1] == "local-sum-f64");
        for (int code : {(int)LRNDE_HIP_ERROR, (int)LRNDE_NCCL_ERROR}) {
          err.clear(); lc_rc_next = code;
          REQUIRE(m0.allreduce(S, v, v, 7, true, &err) == code && !err.empty() && m0.exchanges == 2 && m0.bytes == 76);
        }
        REQUIRE(m0.leave(S, &err) == LRNDE_OK && m0.exchanges == 2 && m0.bytes == 76);   // the counters are the handle's life, not the membership's
        free_events(lc);
      }
      REQUIRE(live_ev == 0 && live_comm == 0);
      {  // allreduce on RCCL
        Membership m;
        double v[8] = {};
        REQUIRE(m.join_rccl(uid, 0, 1, 8, true, 0, S, &err) == LRNDE_OK);
        calls.clear();
        REQUIRE(m.allreduce(S, v, v, 10, false, &err) == LRNDE_OK && m.exchanges == 1 && m.bytes == 40);
        REQUIRE(m.allreduce(S, v, v, 3, true, &err) == LRNDE_OK && m.exchanges == 2 && m.bytes == 40 + 24);
        REQUIRE(calls.size() == 2 && calls[0] == "rccl-sum-f32" && calls[1] == "rccl-sum-f64");
        err.clear(); fail_ar_next = 1;
        REQUIRE(m.allreduce(S, v, v, 3, true, &err) == LRNDE_NCCL_ERROR && !err.empty() && m.exchanges == 2 && m.bytes == 64);
        REQUIRE(m.leave(S, &err) == LRNDE_OK);
      }
      REQUIRE(live_comm == 0);
      {  // lc_barrier: 4 threads x 2000 rounds; then a broken communicator fails every caller at once (not after the timeout)
        lrnde_local_comm lc;
        lc.n = 4;
        int good[4] = {};
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t) th.emplace_back([&lc, &good, t] { for (int i = 0; i < 2000; ++i) good[t] += lc_barrier(&lc) ? 1 : 0; });
        for (auto& t : th) t.join();
        REQUIRE(good[0] == 2000 && good[1] == 2000 && good[2] == 2000 && good[3] == 2000 && lc.gen == 2000 && lc.arrived == 0 && !lc.broken);
        lc.broken = true;
        const auto t0 = std::chrono::steady_clock::now();
        int bad[4] = {};
        th.clear();
        for (int t = 0; t < 4; ++t) th.emplace_back([&lc, &bad, t] { bad[t] = lc_barrier(&lc) ? 0 : 1; });
        for (auto& t : th) t.join();
        REQUIRE(bad[0] && bad[1] && bad[2] && bad[3] && !lc_barrier(&lc) && lc.gen == 2000);
        REQUIRE(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(30));   // (the timeout is 60 s)
      }
      puts("ok");
      return 0;
    }
''')


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("comm")
    src = d / "t.cpp"
    src.write_text(SRC)
    exe = d / "t"
    subprocess.run(["g++", "-std=c++17", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return str(exe)


def test_membership_and_barrier_on_the_host(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
