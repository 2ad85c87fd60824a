// hrp_kin_solve: the kinematic refit of kin_core.h, one 64-lane workgroup per sample.  The solver itself is kin_core.h's solve_one;
// this file gives it the wave's lane and barrier, the sample's LDS and the launch.
#include "hrp_common.h"
#include "kin_core.h"

namespace hrp {
namespace {

struct WaveLanes {
  __device__ __forceinline__ int lo() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int hi() const { return (int)threadIdx.x + 1; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

__global__ __launch_bounds__(kin::KIN_LANES) void kin_solve_kernel(const hrp_kin_desc d) {
  extern __shared__ double kin_lds[];
  kin::solve_one(WaveLanes{}, kin::problem_of(d, (int)blockIdx.x), kin_lds);
}

}  // namespace
}  // namespace hrp

extern "C" int hrp_kin_solve(const hrp_kin_desc* d, void* stream) {
  using namespace hrp;
  const char* why = kin::refusal(d);
  HRP_REQUIRE(!why, "kin_solve: %s", why);
  const int npar = kin::kin_npar(d->free_q, d->dof, d->free_pose);
  const size_t lds = kin::shared_doubles(npar, d->nkp, d->pts3d != nullptr) * sizeof(double);
  HRP_REQUIRE(lds <= 64 * 1024, "kin_solve: %zu bytes of LDS", lds);
  hipLaunchKernelGGL(kin_solve_kernel, dim3(d->B), dim3(kin::KIN_LANES), lds, (hipStream_t)stream, *d);
  return check_launch("kin_solve");
}
