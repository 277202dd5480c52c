// lrnde_comm.hpp — the exchange layer of a batch-sharded handle (the reference has no collective:
// §2 rows 16-17).  Every collective of liblrnde is a SUM all-reduce and goes through lrnde::Membership::allreduce():
//   * RCCL (its all-reduce on the handle's stream) when the handle joined a communicator with lrnde_comm_init /
//     lrnde_conv_comm_init — one process per GPU, the product path;
//   * the in-process LOCAL communicator (lrnde_local_comm_*, include/lrnde_hooks.h) when several handles of one
//     process — driven by one host thread each, all on ONE device (join_local refuses a second device: the sum kernel
//     reads peers' buffers directly and no peer access is set up) — were joined with lrnde_comm_init_local /
//     lrnde_conv_comm_init_local.  It performs the same reduction with stream-ordered kernels and events, so that the
//     nranks > 1 code of the library (offsets into the partial-sum vectors, receive buffers, the sharded adjoint's
//     norm and parameter-cotangent sums) runs on a one-GPU box, where RCCL refuses two ranks on one device.
// A handle holds one Membership (below) and knows nothing else about its communicator; what is particular to a handle
// (which switches it reads, what it resizes after a join) stays in its entry points.  The local all-reduce, its sum
// kernel and the lrnde_local_comm_* / lrnde_comm_unique_id entry points are lrnde_comm.hip's.
// Included by lrnde_kernels.hip and lrnde_conv.hip at file scope; it does not depend on the handle type.  A test off
// the GPU defines LRNDE_COMM_HOST_TEST and supplies the HIP and RCCL names used here, and the local all-reduce, itself
// (tests/test_host_comm.py).
#pragma once

#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#ifdef LRNDE_COMM_HOST_TEST
#define LRNDE_BUF_HOST_TEST
#else
#include <rccl/rccl.h>
#endif
#include "lrnde.h"
#include "lrnde_buf.hpp"
#include "lrnde_fail.hpp"

constexpr int LRNDE_LC_MAXR = 16;

struct lrnde_local_comm {
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  unsigned long gen = 0;
  bool broken = false;  // a rank timed out or failed: every later barrier fails at once instead of hanging
  // per-rank slots of the collective in flight
  const void* send[LRNDE_LC_MAXR] = {};
  DevBuf<char> tmp[LRNDE_LC_MAXR];   // (each on its rank's device: lrnde_local_comm_destroy resets it with that device current)
  hipEvent_t ready[LRNDE_LC_MAXR] = {};  // rank's send buffer is complete (recorded on its stream)
  hipEvent_t done[LRNDE_LC_MAXR] = {};   // rank has finished READING every peer's send buffer
  int device[LRNDE_LC_MAXR] = {};
  bool joined[LRNDE_LC_MAXR] = {};
};

// host barrier over the n rank threads; false on timeout / broken communicator (never hangs a GPU box)
inline bool lc_barrier(lrnde_local_comm* lc) {
  std::unique_lock<std::mutex> lk(lc->mu);
  if (lc->broken) return false;
  const unsigned long g = lc->gen;
  if (++lc->arrived == lc->n) {
    lc->arrived = 0;
    ++lc->gen;
    lc->cv.notify_all();
    return true;
  }
  const bool ok = lc->cv.wait_for(lk, std::chrono::seconds(60), [&] { return lc->gen != g || lc->broken; });
  if (!ok || lc->broken) {
    lc->broken = true;
    lc->cv.notify_all();
    return false;
  }
  return true;
}

// sum all-reduce over the local communicator; send may equal recv (in place).  Returns 0 or a LRNDE status.
int lc_allreduce(lrnde_local_comm* lc, int rank, hipStream_t stream, const void* send, void* recv, size_t count,
                 bool is_double);

namespace lrnde {

// What a handle knows about its communicator.  Every operation returns an LRNDE_* status and writes its message into
// `err` (the handle's).  One rule for every handle: a join first leaves whatever was held; leaving drains the stream
// first (an exchange still queued on it must not outlive its communicator); rank / nranks are assigned only by a join
// that succeeded, so a failed one leaves an unsharded membership.
struct Membership {
  ncclComm_t comm = nullptr;           // RCCL communicator (one process per GPU), owned
  lrnde_local_comm* lcomm = nullptr;   // or: in-process local communicator (lrnde_hooks.h), owned by its creator; never both
  int rank = 0, nranks = 1;
  uint64_t exchanges = 0, bytes = 0;   // all-reduces issued / bytes sent since creation

  bool sharded() const { return comm != nullptr || lcomm != nullptr; }

  // stream == null: the device is drained, as a handle on the null stream is destroyed
  int leave(hipStream_t stream, std::string* err) {
    if (sharded()) {
      if (stream) LRNDE_HIPCHK(err, hipStreamSynchronize(stream)); else LRNDE_HIPCHK(err, hipDeviceSynchronize());
    }
    if (comm) { ncclCommDestroy(comm); comm = nullptr; }
    lcomm = nullptr;   // (its joined[] slot stays taken: a local rendezvous is join-once per rank)
    rank = 0; nranks = 1;
    return LRNDE_OK;
  }

  // max_ranks: the handle's limit, 0 for none.  The communicator is made when nranks > 1 or `force` (the sharded code
  // on one rank, LRNDE_FORCE_COMM); otherwise the handle is left unsharded.
  int join_rccl(const void* uid, int rank_, int nranks_, int max_ranks, bool force, int device, hipStream_t stream,
                std::string* err) {
    if (!uid || nranks_ < 1 || (max_ranks && nranks_ > max_ranks) || rank_ < 0 || rank_ >= nranks_)
      return max_ranks ? failf(err, LRNDE_BADARG, "bad communicator arguments (rank %d of %d; at most %d ranks)", rank_, nranks_, max_ranks)
                       : failf(err, LRNDE_BADARG, "bad communicator arguments (rank %d of %d)", rank_, nranks_);
    LRNDE_HIPCHK(err, hipSetDevice(device));
    { const int rl = leave(stream, err); if (rl) return rl; }
    if (nranks_ > 1 || force) {
      ncclUniqueId id;
      memcpy(&id, uid, sizeof(id));
      const ncclResult_t r = ncclCommInitRank(&comm, nranks_, id, rank_);
      if (r != ncclSuccess) { comm = nullptr; return failf(err, LRNDE_NCCL_ERROR, "ncclCommInitRank failed: %s", ncclGetErrorString(r)); }
      rank = rank_; nranks = nranks_;
    }
    return LRNDE_OK;
  }

  int join_local(lrnde_local_comm* lc, int rank_, int device, hipStream_t stream, std::string* err) {
    if (!lc || rank_ < 0 || rank_ >= lc->n) return failf(err, LRNDE_BADARG, "bad local communicator arguments (rank %d)", rank_);
    LRNDE_HIPCHK(err, hipSetDevice(device));
    if (lcomm == lc) return failf(err, LRNDE_BADARG, "the handle has already joined this local communicator (rank %d)", rank);
    { const int rl = leave(stream, err); if (rl) return rl; }   // whatever other communicator the handle held before
    {
      std::lock_guard<std::mutex> lk(lc->mu);
      if (lc->joined[rank_]) return failf(err, LRNDE_BADARG, "rank %d has already joined this local communicator", rank_);
      // one device only: the sum kernel reads the peers' send buffers directly, and no peer access is set up between devices
      for (int r = 0; r < lc->n; ++r)
        if (lc->joined[r] && lc->device[r] != device)
          return failf(err, LRNDE_UNSUPPORTED, "the in-process local communicator is single-device (rank %d is on device %d, rank %d on %d); "
                       "join an RCCL communicator across devices", r, lc->device[r], rank_, device);
      LRNDE_HIPCHK(err, hipEventCreateWithFlags(&lc->ready[rank_], hipEventDisableTiming));
      LRNDE_HIPCHK(err, hipEventCreateWithFlags(&lc->done[rank_], hipEventDisableTiming));
      lc->device[rank_] = device;
      lc->joined[rank_] = true;
    }
    lcomm = lc; rank = rank_; nranks = lc->n;
    return LRNDE_OK;
  }

  // how many ranks the communicator really has (RCCL's own count, the rendezvous size for the local one, 1 for
  // none — WORLD_SIZE says what was asked for, this says what was built) and its kind: 0 none, 1 RCCL, 2 local
  int count(int* n, int* kind, std::string* err) const {
    *n = 1; *kind = 0;
    if (comm) {
      const ncclResult_t r = ncclCommCount(comm, n);
      if (r != ncclSuccess) return failf(err, LRNDE_NCCL_ERROR, "ncclCommCount failed: %s", ncclGetErrorString(r));
      *kind = 1;
    } else if (lcomm) { *n = lcomm->n; *kind = 2; }
    return LRNDE_OK;
  }

  // every collective of the library: SUM all-reduce of `count` doubles / floats on the stream (send may equal recv).
  // The only caller of either transport; nothing happens on an unsharded membership.
  int allreduce(hipStream_t stream, const void* send, void* recv, size_t count, bool is_double, std::string* err) {
    if (comm) {
      const ncclResult_t r = ncclAllReduce(send, recv, count, is_double ? ncclDouble : ncclFloat, ncclSum, comm, stream);
      if (r != ncclSuccess) return failf(err, LRNDE_NCCL_ERROR, "ncclAllReduce failed: %s", ncclGetErrorString(r));
    } else if (lcomm) {
      const int rc = lc_allreduce(lcomm, rank, stream, send, recv, count, is_double);
      if (rc) return failf(err, rc, "local communicator all-reduce failed (rank %d of %d): %s", rank, nranks,
                           rc == LRNDE_NCCL_ERROR ? "a peer did not arrive (timeout) or the communicator is broken" : "HIP error");
    } else {
      return LRNDE_OK;
    }
    ++exchanges;
    bytes += count * (is_double ? sizeof(double) : sizeof(float));
    return LRNDE_OK;
  }
};

}  // namespace lrnde
