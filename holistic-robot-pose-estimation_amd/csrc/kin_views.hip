// hrp_kin_solve_views: the multi-view kinematic refit of kin_views_core.h, one 64-lane workgroup per sample.  The solver itself is
// kin_views_core.h's solve_one; this file gives it the wave's lane and barrier, the sample's LDS and the launch.
#include "hrp_common.h"
#include "kin_views_core.h"

namespace hrp {
namespace {

struct WaveLanes {
  __device__ __forceinline__ int lo() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int hi() const { return (int)threadIdx.x + 1; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(kin::KIN_LANES) void kin_views_kernel(const hrp_kin_views_desc d) {
  extern __shared__ double kin_views_lds[];
  kinv::solve_one(WaveLanes{}, kinv::problem_of(d, (int)blockIdx.x), kin_views_lds);
}

}  // namespace
}  // namespace hrp

extern "C" int hrp_kin_solve_views(const hrp_kin_views_desc* d, void* stream) {
  using namespace hrp;
  const char* why = kinv::refusal(d);
  HRP_REQUIRE(!why, "kin_solve_views: %s", why);
  const int npar = kin::kin_npar(d->free_q, d->dof, 0);
  const size_t lds = kinv::shared_doubles(npar, d->nkp, d->V) * sizeof(double);
  hipLaunchKernelGGL(kin_views_kernel, dim3(d->B), dim3(kin::KIN_LANES), lds, (hipStream_t)stream, *d);
  return check_launch("kin_solve_views");
}
