// hrp_kin_filter_step: the kinematic filter of kin_filter_core.h, one 64-lane workgroup per stream.  The step itself is
// kin_filter_core.h's step_one; this file gives it the wave's lane and barrier, the stream's LDS and the launch.
#include "hrp_common.h"
#include "kin_filter_core.h"

namespace hrp {
namespace {

struct WaveLanes {
  __device__ __forceinline__ int lo() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int hi() const { return (int)threadIdx.x + 1; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(kin::KIN_LANES) void kin_filter_kernel(const hrp_kin_filter_desc d) {
  extern __shared__ double kin_filter_lds[];
  kinf::step_one(WaveLanes{}, kinf::stream_of(d, (int)blockIdx.x), kin_filter_lds);
}

}  // namespace
}  // namespace hrp

extern "C" int hrp_kin_filter_step(const hrp_kin_filter_desc* d, void* stream) {
  using namespace hrp;
  const char* why = kinf::refusal(d);
  HRP_REQUIRE(!why, "kin_filter_step: %s", why);
  const int n = kin::kin_npar(d->free_q, d->dof, d->free_pose);
  const size_t lds = kinf::shared_doubles(n, d->nkp, d->dof) * sizeof(double);
  HRP_REQUIRE(lds <= 64 * 1024, "kin_filter_step: %zu bytes of LDS", lds);
  hipLaunchKernelGGL(kin_filter_kernel, dim3(d->B), dim3(kin::KIN_LANES), lds, (hipStream_t)stream, *d);
  return check_launch("kin_filter_step");
}
