// hrp_kin_history_push and hrp_kin_smooth: the recorded history of the kinematic filter and the smoother of kin_smooth_core.h.  The
// recursion itself is kin_smooth_core.h's link_one / walk_one; this file gives them the workgroup's lane and barrier, the LDS and the
// launches: links on a grid (L, B), then one workgroup per stream for the walk.
#include "hrp_common.h"
#include "kin_smooth_core.h"

namespace hrp {
namespace {

struct GroupLanes {
  __device__ __forceinline__ int lo() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int hi() const { return (int)threadIdx.x + 1; }
  __device__ __forceinline__ int lanes() const { return kins::SMOOTH_LANES; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(kins::SMOOTH_LANES) void kin_smooth_link_kernel(const hrp_kin_smooth_desc d) {
  extern __shared__ double kin_smooth_lds[];
  kins::link_one(GroupLanes{}, d, (int)blockIdx.x, (int)blockIdx.y, kin_smooth_lds);
}

__global__ __launch_bounds__(kins::SMOOTH_LANES) void kin_smooth_walk_kernel(const hrp_kin_smooth_desc d) {
  extern __shared__ double kin_smooth_lds[];
  kins::walk_one(GroupLanes{}, d, (int)blockIdx.x, kin_smooth_lds);
}

template <class T>
__device__ __forceinline__ void copy_strided(T* dst, const T* src, size_t count, size_t first, size_t step) {
  for (size_t i = first; i < count; i += step) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void kin_history_push_kernel(const hrp_kin_history_desc d) {
  const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const size_t B = (size_t)d.B, N = 2 * (size_t)d.n, slot = (size_t)d.slot;
  copy_strided(d.h_cov + slot * B * N * N, d.cov, B * N * N, first, step);
  copy_strided(d.h_mean + slot * B * N, d.mean, B * N, first, step);
  copy_strided(d.h_valid + slot * B, d.valid, B, first, step);
  if (d.dof > 0) copy_strided(d.h_q_in + slot * B * d.dof, d.q_in, B * d.dof, first, step);
  for (size_t i = first; i < B; i += step) d.h_flags[slot * B + i] = d.status[4 * i];
  if (first == 0) d.h_dt[slot] = d.dt;
}

}  // namespace
}  // namespace hrp

extern "C" int hrp_kin_history_push(const hrp_kin_history_desc* d, void* stream) {
  using namespace hrp;
  const char* why = kins::push_refusal(d);
  HRP_REQUIRE(!why, "kin_history_push: %s", why);
  const size_t work = (size_t)d->B * 4 * d->n * d->n;
  const size_t blocks = (work + 255) / 256;
  hipLaunchKernelGGL(kin_history_push_kernel, dim3((unsigned)(blocks < 256 ? blocks : 256)), dim3(256), 0, (hipStream_t)stream, *d);
  return check_launch("kin_history_push");
}

extern "C" int hrp_kin_smooth(const hrp_kin_smooth_desc* d, void* stream) {
  using namespace hrp;
  const char* why = kins::refusal(d);
  HRP_REQUIRE(!why, "kin_smooth: %s", why);
  const int n = kins::npar_of(*d);
  const size_t lds_link = kins::link_doubles(2 * n) * sizeof(double), lds_walk = kins::walk_doubles(n, d->nkp) * sizeof(double);
  HRP_REQUIRE(lds_link <= 64 * 1024 && lds_walk <= 64 * 1024, "kin_smooth: %zu / %zu bytes of LDS", lds_link, lds_walk);
  HRP_REQUIRE(d->B <= 65535, "kin_smooth: B %d > 65535 (the grid's second dimension)", d->B);
  hipLaunchKernelGGL(kin_smooth_link_kernel, dim3(d->L, d->B), dim3(kins::SMOOTH_LANES), lds_link, (hipStream_t)stream, *d);
  if (int rc = check_launch("kin_smooth (links)")) return rc;
  hipLaunchKernelGGL(kin_smooth_walk_kernel, dim3(d->B), dim3(kins::SMOOTH_LANES), lds_walk, (hipStream_t)stream, *d);
  return check_launch("kin_smooth");
}
