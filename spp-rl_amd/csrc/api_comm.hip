// libspprl C-ABI, the RCCL exchange (§8e): the sppComm* entry points and the gradient-bucket average that
// sppAllReduceGrads (api.hip) hands its buffer list to.  Knows neither the agent nor any kernel but k_scale.
// librccl is resolved at run time (the one torch already loaded, if any), so the library has no
// link-time RCCL dependency and a C/C++ host can run data parallelism without torch.distributed.
#include <dlfcn.h>
#include <string.h>

#include <algorithm>

#include "host_base.h"

using namespace spp;

namespace {
struct RcclUid {
  char internal[SPP_COMM_ID_BYTES];
};
struct Rccl {
  int (*get_uid)(RcclUid*) = nullptr;
  int (*init_rank)(void**, int, RcclUid, int) = nullptr;
  int (*destroy)(void*) = nullptr;
  int (*all_reduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  const char* (*err)(int) = nullptr;
  bool ok = false;
};
Rccl& rccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return r;
  tried = true;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return r;
  r.get_uid = (int (*)(RcclUid*))dlsym(lib, "ncclGetUniqueId");
  r.init_rank = (int (*)(void**, int, RcclUid, int))dlsym(lib, "ncclCommInitRank");
  r.destroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
  r.all_reduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(lib, "ncclAllReduce");
  r.all_gather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(lib, "ncclAllGather");
  r.group_start = (int (*)())dlsym(lib, "ncclGroupStart");
  r.group_end = (int (*)())dlsym(lib, "ncclGroupEnd");
  r.err = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
  r.ok = r.get_uid && r.init_rank && r.destroy && r.all_reduce && r.all_gather && r.group_start && r.group_end && r.err;
  return r;
}
constexpr int kNcclFloat32 = 7, kNcclSum = 0;
}  // namespace

#define SPP_CHECK_RCCL(expr)                                                                   \
  do {                                                                                         \
    const int r_ = (expr);                                                                     \
    if (r_ != 0) {                                                                             \
      ::spp::set_error("%s:%d %s -> rccl %d (%s)", __FILE__, __LINE__, #expr, r_, rccl().err(r_)); \
      return SPP_E_RCCL;                                                                       \
    }                                                                                          \
  } while (0)

extern "C" {

// (inside extern "C" since it was written: its kernel name is the unmangled k_scale)
__global__ void k_scale(float* x, int64_t n, float s) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    x[i] *= s;
}

sppStatus sppCommGetUniqueId(void* uid_out) {
  SPP_REQUIRE(uid_out, SPP_E_INVALID_ARG, "comm uid: null");
  SPP_REQUIRE(rccl().ok, SPP_E_RCCL, "librccl.so.1 not loadable");
  RcclUid u;
  SPP_CHECK_RCCL(rccl().get_uid(&u));
  memcpy(uid_out, &u, sizeof(u));
  return SPP_OK;
}

sppStatus sppCommInitRank(void** comm_out, int nranks, const void* uid, int rank, int device) {
  SPP_REQUIRE(comm_out && uid && nranks > 0 && rank >= 0 && rank < nranks, SPP_E_INVALID_ARG,
              "comm init: nranks %d rank %d", nranks, rank);
  SPP_REQUIRE(rccl().ok, SPP_E_RCCL, "librccl.so.1 not loadable");
  SPP_CHECK_HIP(hipSetDevice(device));
  RcclUid u;
  memcpy(&u, uid, sizeof(u));
  void* c = nullptr;
  SPP_CHECK_RCCL(rccl().init_rank(&c, nranks, u, rank));
  *comm_out = c;
  return SPP_OK;
}

sppStatus sppCommDestroy(void* comm) {
  SPP_REQUIRE(comm, SPP_E_INVALID_ARG, "comm destroy: null");
  SPP_REQUIRE(rccl().ok, SPP_E_RCCL, "librccl.so.1 not loadable");
  SPP_CHECK_RCCL(rccl().destroy(comm));
  return SPP_OK;
}

// In-place sum of a device buffer over the communicator (the obs-statistics exchange of C hosts).
sppStatus sppCommAllReduceSum(void* comm, void* buf, int64_t count, int dtype, void* stream) {
  SPP_REQUIRE(comm && buf && count >= 0 && dtype >= 0 && dtype <= 4, SPP_E_INVALID_ARG,
              "comm allreduce sum: dtype %d count %lld", dtype, (long long)count);
  SPP_REQUIRE(rccl().ok, SPP_E_RCCL, "librccl.so.1 not loadable");
  // ncclFloat32 7, ncclFloat64 8, ncclInt32 2, ncclInt64 4, ncclUint32 3
  static const int kType[5] = {7, 8, 2, 4, 3};
  if (count == 0) return SPP_OK;
  SPP_CHECK_RCCL(rccl().all_reduce(buf, buf, (size_t)count, kType[dtype], kNcclSum, comm, S(stream)));
  return SPP_OK;
}

// Rank-major all-gather of `bytes` per rank (the one-pass statistics' sample exchange); in place when
// send == recv + rank * bytes.
sppStatus sppCommAllGather(void* comm, const void* send, void* recv, int64_t bytes, void* stream) {
  SPP_REQUIRE(comm && send && recv && bytes >= 0, SPP_E_INVALID_ARG, "comm allgather: bad args");
  SPP_REQUIRE(rccl().ok, SPP_E_RCCL, "librccl.so.1 not loadable");
  if (bytes == 0) return SPP_OK;
  SPP_CHECK_RCCL(rccl().all_gather(send, recv, (size_t)bytes, 0 /* ncclInt8 */, comm, S(stream)));
  return SPP_OK;
}

}  // extern "C"

// ---- the agent's gradient exchange (api.hip: sppAllReduceGrads; host_base.h)
namespace spp {

bool comm_loaded() { return rccl().ok; }

// In-place fp32 sum of each buffer over the communicator as one group, then x 1/world.
sppStatus comm_allreduce_mean(const std::vector<std::pair<float*, int64_t>>& bufs, int world, void* comm,
                              hipStream_t st) {
  SPP_CHECK_RCCL(rccl().group_start());
  for (auto& b : bufs) {
    const int r = rccl().all_reduce(b.first, b.first, (size_t)b.second, kNcclFloat32, kNcclSum, comm, st);
    if (r != 0) {
      rccl().group_end();
      set_error("ncclAllReduce -> rccl %d (%s)", r, rccl().err(r));
      return SPP_E_RCCL;
    }
  }
  SPP_CHECK_RCCL(rccl().group_end());
  if (world > 1) {
    const float inv = 1.0f / (float)world;
    for (auto& b : bufs)
      hipLaunchKernelGGL(k_scale, dim3(std::max(1, std::min(cdiv(b.second, 256), 1024))), dim3(256), 0, st, b.first,
                         b.second, inv);
  }
  SPP_CHECK_HIP(hipGetLastError());
  return SPP_OK;
}

}  // namespace spp
