// lrnde_comm.hip — the communicator's own translation unit: what lrnde_comm.hpp declares and no handle owns.  The
// in-process local communicator's sum all-reduce with its kernel (one device copy in the library), the
// lrnde_local_comm_* entry points (include/lrnde_hooks.h) and lrnde_comm_unique_id (include/lrnde.h).
#include <hip/hip_runtime.h>

#include "lrnde.h"
#include "lrnde_hooks.h"
#include "lrnde_comm.hpp"

namespace {

struct LcPtrs { const void* p[LRNDE_LC_MAXR]; };

// out[i] = p[0][i] + p[1][i] + ... in rank order (what a sum all-reduce returns; with the zero-padded vectors the
// library exchanges every element has one non-zero term, so the order does not matter there)
template <class T> __global__ void k_lc_sum(LcPtrs s, int n, size_t count, T* out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    T acc = reinterpret_cast<const T*>(s.p[0])[i];
    for (int r = 1; r < n; ++r) acc = acc + reinterpret_cast<const T*>(s.p[r])[i];
    out[i] = acc;
  }
}

}  // namespace

int lc_allreduce(lrnde_local_comm* lc, int rank, hipStream_t stream, const void* send, void* recv, size_t count,
                 bool is_double) {
  const size_t bytes = count * (is_double ? sizeof(double) : sizeof(float));
  if (lc->tmp[rank].grow(bytes) != hipSuccess) return LRNDE_HIP_ERROR;
  lc->send[rank] = send;
  if (hipEventRecord(lc->ready[rank], stream) != hipSuccess) return LRNDE_HIP_ERROR;
  if (!lc_barrier(lc)) return LRNDE_NCCL_ERROR;
  LcPtrs s;
  for (int r = 0; r < lc->n; ++r) {
    s.p[r] = lc->send[r];
    if (r != rank && hipStreamWaitEvent(stream, lc->ready[r], 0) != hipSuccess) return LRNDE_HIP_ERROR;
  }
  int nb = (int)((count + 255) / 256); if (nb > 1024) nb = 1024; if (nb < 1) nb = 1;
  if (is_double) hipLaunchKernelGGL(k_lc_sum<double>, dim3(nb), dim3(256), 0, stream, s, lc->n, count, (double*)lc->tmp[rank].get());
  else hipLaunchKernelGGL(k_lc_sum<float>, dim3(nb), dim3(256), 0, stream, s, lc->n, count, (float*)lc->tmp[rank].get());
  if (hipGetLastError() != hipSuccess) return LRNDE_HIP_ERROR;
  if (hipEventRecord(lc->done[rank], stream) != hipSuccess) return LRNDE_HIP_ERROR;
  if (!lc_barrier(lc)) return LRNDE_NCCL_ERROR;
  // nobody may overwrite a send buffer (this rank's recv may BE its send buffer) before every peer has read it
  for (int r = 0; r < lc->n; ++r)
    if (r != rank && hipStreamWaitEvent(stream, lc->done[r], 0) != hipSuccess) return LRNDE_HIP_ERROR;
  if (hipMemcpyAsync(recv, lc->tmp[rank], bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) return LRNDE_HIP_ERROR;
  return LRNDE_OK;
}

extern "C" {

int lrnde_comm_unique_id(void* out) {
  if (!out) return LRNDE_BADARG;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return LRNDE_NCCL_ERROR;
  memcpy(out, &id, sizeof(id));
  return LRNDE_OK;
}

int lrnde_local_comm_create(lrnde_local_comm** out, int32_t nranks) {
  if (!out || nranks < 1 || nranks > LRNDE_LC_MAXR) return LRNDE_BADARG;
  lrnde_local_comm* lc = new lrnde_local_comm();
  lc->n = nranks;
  *out = lc;
  return LRNDE_OK;
}

int lrnde_local_comm_destroy(lrnde_local_comm* lc) {
  if (!lc) return LRNDE_OK;
  for (int r = 0; r < lc->n; ++r) {
    if (!lc->joined[r]) continue;
    hipSetDevice(lc->device[r]);
    (void)lc->tmp[r].reset();
    if (lc->ready[r]) hipEventDestroy(lc->ready[r]);
    if (lc->done[r]) hipEventDestroy(lc->done[r]);
  }
  delete lc;
  return LRNDE_OK;
}

}  // extern "C"
