// Pooled robust PnP (hrp_pnp_solve_pooled): the consensus-then-refit of pnp.hip's pnp_robust_kernel for a point count that is not tied
// to a wavefront (4 <= n <= HRP_PNP_POOLED_MAX_N), which is what one camera pose from a whole sequence of frames needs.  fp32 in and
// out, fp64 inside, three launches that only the kernel boundary orders:
//   compact   one workgroup per problem: the usable points' indices in index order (rank -> index), their number m and the hypothesis
//             count H into the workspace
//   score     lane = hypothesis, grid (ceil(Hmax / 64), B): P3P on the triple (pnp_minimal.h), every root scored against the m usable
//             points, which pass through LDS in tiles of POOL_TILE; one record (count, ssq, root, R, t) per hypothesis
//   fit       one 256-thread workgroup per problem: the winner from the records in a fixed total order, then pnp_lm.h's LM with the
//             sums taken over points lane, lane + 256, ... in index order, by wsum's butterfly within a wave and in wave order across
//             the four waves.  Every value a lane branches on is such a broadcast sum, so two identical calls return identical bytes.
// A thread owns the ranks tid, tid + 256, ... throughout the fit launch, so the membership flags of the fit set are private to it.
#include "hrp_common.h"
#include "pnp_minimal.h"
#include "pnp_lm.h"

namespace hrp {
namespace {

constexpr int POOL_THREADS = 256;      // fit and compact launches
constexpr int POOL_WAVES = POOL_THREADS / 64;
constexpr int POOL_LANES = 64;         // hypotheses per workgroup of the score launch
constexpr int POOL_TILE = 256;         // points staged per pass of the score launch
constexpr int POOL_SUMS = 28;          // cost, Jte (6), the upper triangle of JtJ (21)

struct PooledRecord {                  // 112 bytes
  int count, slot;
  double ssq, R[9], t[3];
};

// the workspace of one problem: head (m, H, 0, 0), idx[round_up(n, 4)], rec[Hmax]
struct PooledLayout {
  size_t idx_off, rec_off, stride;
};
inline PooledLayout pooled_layout(int n, int hmax) {
  PooledLayout L;
  L.idx_off = 16;
  L.rec_off = L.idx_off + 4 * (size_t)round_up(n, 4);
  L.stride = L.rec_off + sizeof(PooledRecord) * (size_t)hmax;
  return L;
}

__device__ __forceinline__ void load_K(const float* __restrict__ Km, int K_stride, int b, double (&K)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = Km[(size_t)b * K_stride + k];
}
__device__ __forceinline__ void load_point(const float* __restrict__ pts2d, const float* __restrict__ pts3d, size_t p, double (&X)[3],
                                           double (&x)[2]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = pts3d[p * 3 + k];
  x[0] = pts2d[p * 2];
  x[1] = pts2d[p * 2 + 1];
}

// sum of one int per thread over the workgroup, the same in every thread
__device__ __forceinline__ int block_sum(int v, int* sI, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((tid & 63) == 0) sI[tid >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < POOL_WAVES; ++w) s += sI[w];
  return s;
}

// ---- launch 1: the usable points, compacted in index order ------------------------------------------------------------------------------
__global__ __launch_bounds__(POOL_THREADS) void pnp_pooled_compact_kernel(const float* __restrict__ pts2d, const float* __restrict__ pts3d,
                                                                          const float* __restrict__ Km, int K_stride,
                                                                          const unsigned char* __restrict__ valid, int n, int max_hypotheses,
                                                                          unsigned char* __restrict__ ws, PooledLayout L) {
  __shared__ int sCnt[POOL_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* head = (int*)(ws + (size_t)b * L.stride);
  int* idx = (int*)(ws + (size_t)b * L.stride + L.idx_off);
  double K[9];
  load_K(Km, K_stride, b, K);
  int base = 0;
  for (int p0 = 0; p0 < n; p0 += POOL_THREADS) {
    const int p = p0 + tid;
    bool ok = false;
    if (p < n) {
      double X[3], x[2], F[3];
      load_point(pts2d, pts3d, (size_t)b * n + p, X, x);
      ok = pnpmin::point_valid(valid ? valid + (size_t)b * n + p : nullptr, X, x) && pnpmin::bearing(K, x, F);
    }
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) sCnt[wave] = __popcll(mask);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int w = 0; w < POOL_WAVES; ++w) {
      off += w < wave ? sCnt[w] : 0;
      total += sCnt[w];
    }
    if (ok) idx[off + __popcll(mask & ((1ull << lane) - 1ull))] = p;
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    head[0] = base;
    head[1] = pnpmin::pooled_hypothesis_count(base, max_hypotheses);
    head[2] = head[3] = 0;
  }
}

// ---- launch 2: lane = hypothesis ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(POOL_LANES) void pnp_pooled_score_kernel(const float* __restrict__ pts2d, const float* __restrict__ pts3d,
                                                                      const float* __restrict__ Km, int K_stride, int n, double thr,
                                                                      int max_hypotheses, unsigned seed, unsigned char* __restrict__ ws,
                                                                      PooledLayout L) {
  __shared__ double sX[POOL_TILE][3], sx[POOL_TILE][2];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int* head = (const int*)(ws + (size_t)b * L.stride);
  const int* idx = (const int*)(ws + (size_t)b * L.stride + L.idx_off);
  PooledRecord* rec = (PooledRecord*)(ws + (size_t)b * L.stride + L.rec_off);
  const int m = head[0], H = head[1];
  if ((int)blockIdx.x * POOL_LANES >= H) return;      // the same for the whole workgroup
  const int h = blockIdx.x * POOL_LANES + lane;
  const bool live = h < H;
  const double thr2 = thr * thr;
  const size_t p_base = (size_t)b * n;
  double K[9];
  load_K(Km, K_stride, b, K);

  pnpmin::P3P S = {};
  if (live) {
    int tri[3];
    pnpmin::pooled_hypothesis_triple(h, m, max_hypotheses, seed, tri[0], tri[1], tri[2]);
    double X3[3][3], f3[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double x[2];
      load_point(pts2d, pts3d, p_base + idx[tri[a]], X3[a], x);
      pnpmin::bearing(K, x, f3[a]);                     // true for every usable point: the compaction asked
    }
    pnpmin::p3p_prepare(X3, f3, S);
  }

  int best_count = -1, best_slot = 0;
  double best_ssq = 0.0, bR[3][3], bt[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    bt[r] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) bR[r][k] = r == k ? 1.0 : 0.0;
  }
#pragma nounroll
  for (int slot = 0; slot < 4; ++slot) {
    double R[3][3], t[3];
    const bool has = pnpmin::p3p_pose(S, slot, R, t);
    if (!__any(has)) continue;                          // no lane holds this root
    int count = 0;
    double ssq = 0.0;
    for (int q0 = 0; q0 < m; q0 += POOL_TILE) {
      const int cnt = m - q0 < POOL_TILE ? m - q0 : POOL_TILE;
      __syncthreads();
      for (int i = lane; i < cnt; i += POOL_LANES) {
        double X[3], x[2];
        load_point(pts2d, pts3d, p_base + idx[q0 + i], X, x);
#pragma unroll
        for (int k = 0; k < 3; ++k) sX[i][k] = X[k];
        sx[i][0] = x[0];
        sx[i][1] = x[1];
      }
      __syncthreads();
      if (has) {
        for (int i = 0; i < cnt; ++i) {
          const double Xp[3] = {sX[i][0], sX[i][1], sX[i][2]}, xp[2] = {sx[i][0], sx[i][1]};
          double e2;
          if (pnpmin::reproj_e2(R, t, K, Xp, xp, e2) && e2 < thr2) {
            ++count;
            ssq += e2;
          }
        }
      }
    }
    if (has && pnpmin::score_better(count, ssq, best_count, best_ssq)) {
      best_count = count;
      best_ssq = ssq;
      best_slot = slot;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        bt[r] = t[r];
#pragma unroll
        for (int k = 0; k < 3; ++k) bR[r][k] = R[r][k];
      }
    }
  }
  if (live) {
    PooledRecord& o = rec[h];
    o.count = best_count;
    o.slot = best_slot;
    o.ssq = best_ssq;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      o.t[r] = bt[r];
#pragma unroll
      for (int k = 0; k < 3; ++k) o.R[3 * r + k] = bR[r][k];
    }
  }
}

// ---- launch 3: winner, LM on its inliers, refits ------------------------------------------------------------------------------------------
struct PooledPoints {
  const float* pts2d;
  const float* pts3d;
  const int* idx;
  const unsigned char* fit;     // LDS, by rank: 1 where the point is in the fit set
  double* red;                  // LDS, POOL_WAVES * POOL_SUMS
  size_t p_base;
  int m, tid;
};

// where JtJ[a][c], a <= c, lies among the sums: 0 the cost, 1..6 Jte, then the upper triangle row by row
__device__ __forceinline__ constexpr int tri_ix(int a, int c) { return 7 + a * 6 - a * (a - 1) / 2 + (c - a); }

// lm_eval of pnp.hip over the fit set: cost = sum |e|^2, JtJ and Jte, the same in every thread
__device__ void pooled_eval(const Pose& y, const double (&K)[9], const PooledPoints& P, double& cost, double (&JtJ)[6][6], double (&Jte)[6]) {
  J2 R[3][3];
  rodrigues_jet(y.w, R);
  double acc[POOL_SUMS];
#pragma unroll
  for (int k = 0; k < POOL_SUMS; ++k) acc[k] = 0.0;
  for (int q = P.tid; q < P.m; q += POOL_THREADS) {
    if (!P.fit[q]) continue;
    double X[3], x[2], e[2], J[2][6];
    load_point(P.pts2d, P.pts3d, P.p_base + P.idx[q], X, x);
    residual_jac(R, y.t, K, X, x, e, J);
    acc[0] += e[0] * e[0] + e[1] * e[1];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      acc[1 + a] += J[0][a] * e[0] + J[1][a] * e[1];
#pragma unroll
      for (int c = a; c < 6; ++c) acc[tri_ix(a, c)] += J[0][a] * J[0][c] + J[1][a] * J[1][c];
    }
  }
  __syncthreads();                                       // the previous call's sums have been read
#pragma unroll
  for (int k = 0; k < POOL_SUMS; ++k) {
    const double v = wsum(acc[k]);
    if ((P.tid & 63) == 0) P.red[(P.tid >> 6) * POOL_SUMS + k] = v;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < POOL_SUMS; ++k) {
    double s = P.red[k];
#pragma unroll
    for (int w = 1; w < POOL_WAVES; ++w) s += P.red[w * POOL_SUMS + k];
    acc[k] = s;
  }
  cost = acc[0];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    Jte[a] = acc[1 + a];
#pragma unroll
    for (int c = a; c < 6; ++c) JtJ[a][c] = JtJ[c][a] = acc[tri_ix(a, c)];
  }
}

// lm_refine of pnp.hip (the same damping and stopping rules, so the same objective and minimum) on pooled_eval's sums
__device__ void pooled_lm_refine(Pose& y, const double (&K)[9], const PooledPoints& P, double& cost, int& it, int& converged) {
  double JtJ[6][6], Jte[6];
  pooled_eval(y, K, P, cost, JtJ, Jte);
  double lambda = 1e-3;
  it = 0;
  converged = 0;
  for (; it < PNP_LM_MAX_IT; ++it) {
    double A[6][6], st[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = 0; c < 6; ++c) A[a][c] = JtJ[a][c];
      A[a][a] += lambda * JtJ[a][a];
      st[a] = -Jte[a];
    }
    if (chol_solve<6>(A, st)) {
      Pose yn;
      double smax = 0.0, ymax = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        yn.w[k] = y.w[k] + st[k];
        yn.t[k] = y.t[k] + st[3 + k];
        smax = fmax(smax, fmax(fabs(st[k]), fabs(st[3 + k])));
        ymax = fmax(ymax, fmax(fabs(y.w[k]), fabs(y.t[k])));
      }
      double cn, JtJn[6][6], Jten[6];
      pooled_eval(yn, K, P, cn, JtJn, Jten);
      if (cn < cost) {
        y = yn;
        cost = cn;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          Jte[a] = Jten[a];
#pragma unroll
          for (int c = 0; c < 6; ++c) JtJ[a][c] = JtJn[a][c];
        }
        lambda = fmax(lambda * 0.1, 1e-12);
        if (smax <= 1e-12 * (1.0 + ymax)) { converged = 1; ++it; break; }
        continue;
      }
    }
    lambda *= 10.0;
    if (lambda > 1e10) { converged = 1; ++it; break; }
  }
}

__device__ __forceinline__ bool pooled_inlier(const double (&R)[3][3], const double (&t)[3], const double (&K)[9], const PooledPoints& P, int q,
                                              double thr2) {
  double X[3], x[2], e2;
  load_point(P.pts2d, P.pts3d, P.p_base + P.idx[q], X, x);
  return pnpmin::reproj_e2(R, t, K, X, x, e2) && e2 < thr2;
}

__global__ __launch_bounds__(POOL_THREADS) void pnp_pooled_fit_kernel(const float* __restrict__ pts2d, const float* __restrict__ pts3d,
                                                                      const float* __restrict__ Km, int K_stride, int n, double thr,
                                                                      int min_inliers, int refine_all, const unsigned char* __restrict__ ws,
                                                                      PooledLayout L, float* __restrict__ P6d,
                                                                      unsigned char* __restrict__ inliers, int* __restrict__ status,
                                                                      float* __restrict__ rms, float* __restrict__ cov) {
  __shared__ unsigned char sFit[HRP_PNP_POOLED_MAX_N], sNew[HRP_PNP_POOLED_MAX_N];
  __shared__ double sRed[POOL_WAVES * POOL_SUMS], sWs[POOL_WAVES];
  __shared__ int sWc[POOL_WAVES], sWh[POOL_WAVES], sI[POOL_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* head = (const int*)(ws + (size_t)b * L.stride);
  const PooledRecord* rec = (const PooledRecord*)(ws + (size_t)b * L.stride + L.rec_off);
  const int m = head[0], H = head[1];
  const double thr2 = thr * thr;
  double K[9];
  load_K(Km, K_stride, b, K);
  PooledPoints P;
  P.pts2d = pts2d; P.pts3d = pts3d;
  P.idx = (const int*)(ws + (size_t)b * L.stride + L.idx_off);
  P.fit = sFit; P.red = sRed;
  P.p_base = (size_t)b * n;
  P.m = m; P.tid = tid;

  // the winner: more inliers, then the smaller sum of squares, then the lower hypothesis (a record holds its hypothesis' best root,
  // ties to the lower slot): a total order, so the order of the comparisons does not matter
  int wc = -1, wh = 0x7fffffff;
  double ws_ = 0.0;
  auto take = [&](int oc, double os, int oh) {
    if (pnpmin::score_better(oc, os, wc, ws_) || (oc == wc && os == ws_ && oh < wh)) {
      wc = oc;
      ws_ = os;
      wh = oh;
    }
  };
  for (int h = tid; h < H; h += POOL_THREADS) take(rec[h].count, rec[h].ssq, h);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(wc, o, 64), oh = __shfl_xor(wh, o, 64);
    const double os = __shfl_xor(ws_, o, 64);
    take(oc, os, oh);
  }
  if ((tid & 63) == 0) {
    sWc[tid >> 6] = wc;
    sWs[tid >> 6] = ws_;
    sWh[tid >> 6] = wh;
  }
  __syncthreads();
  wc = sWc[0]; ws_ = sWs[0]; wh = sWh[0];
#pragma unroll
  for (int w = 1; w < POOL_WAVES; ++w) take(sWc[w], sWs[w], sWh[w]);
  double bR[3][3], bt[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    bt[r] = wh < H ? rec[wh].t[r] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) bR[r][k] = wh < H ? rec[wh].R[3 * r + k] : (r == k ? 1.0 : 0.0);
  }
  const bool consensus = wc >= min_inliers, few = m < 4;      // the same in every thread

  Pose y;
  pnpmin::rot_to_aa(bR, y.w);
#pragma unroll
  for (int k = 0; k < 3; ++k) y.t[k] = bt[k];
  // the fit set: the winner's inliers, or every usable point without consensus
  int mine = 0;
  for (int q = tid; q < m; q += POOL_THREADS) {
    const bool in = !consensus || pooled_inlier(bR, bt, K, P, q, thr2);
    sFit[q] = in ? 1 : 0;
    mine += in ? 1 : 0;
  }
  for (int p = tid; p < n; p += POOL_THREADS) inliers[P.p_base + p] = 0;
  int nfit = block_sum(mine, sI, tid);

  double cost = 0.0;
  int its = 0, converged = 0;
  if (!few) {
    bool over_all = false;
    for (int round = 0;; ++round) {
      int it;
      pooled_lm_refine(y, K, P, cost, it, converged);
      its += it;
      if (!consensus || over_all) break;
      double R[3][3];
      pnpmin::aa_to_rot(y.w, R);
      int changed = 0;
      mine = 0;
      for (int q = tid; q < m; q += POOL_THREADS) {
        const bool in = pooled_inlier(R, y.t, K, P, q, thr2);
        sNew[q] = in ? 1 : 0;
        changed |= (in ? 1 : 0) != sFit[q];
        mine += in ? 1 : 0;
      }
      if (__syncthreads_or(changed) && round < HRP_PNP_POOLED_REFITS - 1) {
        for (int q = tid; q < m; q += POOL_THREADS) sFit[q] = sNew[q];
        nfit = block_sum(mine, sI, tid);
        continue;
      }
      if (!refine_all) break;
      for (int q = tid; q < m; q += POOL_THREADS) sFit[q] = 1;
      nfit = m;
      over_all = true;
    }
  }
  normalise_rotation(y);
  {
    double R[3][3];
    pnpmin::aa_to_rot(y.w, R);
    mine = 0;
    __syncthreads();                                     // the zeros above are in place
    for (int q = tid; q < m; q += POOL_THREADS) {
      const bool in = pooled_inlier(R, y.t, K, P, q, thr2);
      if (in) inliers[P.p_base + P.idx[q]] = 1;
      mine += in ? 1 : 0;
    }
  }
  const int count = block_sum(mine, sI, tid);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      P6d[b * 6 + k] = (float)y.w[k];
      P6d[b * 6 + 3 + k] = (float)y.t[k];
    }
    status[b * 4] = (consensus ? 0 : HRP_PNP_NO_CONSENSUS) | (converged ? HRP_PNP_CONVERGED : 0) | (few ? HRP_PNP_FEW_POINTS : 0);
    status[b * 4 + 1] = its;
    status[b * 4 + 2] = count;
    status[b * 4 + 3] = H;
    rms[b] = (!few && nfit) ? (float)sqrt(cost / nfit) : 0.0f;
  }
  if (!cov) return;
  // s^2 (JtJ)^-1 at the returned pose over the points of the last fit, column by column through the Cholesky factor
  const bool have = !few && nfit > 3;
  double c2 = 0.0, JtJ[6][6], Jte[6];
  if (have) pooled_eval(y, K, P, c2, JtJ, Jte);
  const double s2 = have ? c2 / (2.0 * nfit - 6.0) : 0.0;
#pragma nounroll
  for (int c = 0; c < 6; ++c) {
    double A[6][6], v[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      v[a] = a == c ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) A[a][k] = have ? JtJ[a][k] : 0.0;
    }
    const bool ok = have && chol_solve<6>(A, v);
    if (tid == 0) {
#pragma unroll
      for (int a = 0; a < 6; ++a)
        if (a <= c) cov[b * 36 + a * 6 + c] = cov[b * 36 + c * 6 + a] = ok ? (float)(s2 * v[a]) : 0.0f;
    }
  }
}

int pooled_args(const char* what, int B, int n, int max_hypotheses) {
  HRP_REQUIRE(B > 0 && B <= 65535, "%s: %d problems (1..65535)", what, B);
  HRP_REQUIRE(n >= 4 && n <= HRP_PNP_POOLED_MAX_N, "%s: %d points (4..%d supported)", what, n, HRP_PNP_POOLED_MAX_N);
  HRP_REQUIRE(max_hypotheses >= 1 && max_hypotheses <= (1 << 20), "%s: max_hypotheses %d (1..2^20)", what, max_hypotheses);
  return 0;
}

}  // namespace
}  // namespace hrp

using namespace hrp;

extern "C" int hrp_pnp_pooled_workspace_bytes(int B, int n, int max_hypotheses, size_t* bytes) {
  HRP_REQUIRE(bytes, "pnp_pooled_workspace_bytes: bad args");
  if (int rc = pooled_args("pnp_pooled_workspace_bytes", B, n, max_hypotheses)) return rc;
  *bytes = (size_t)B * pooled_layout(n, pnpmin::pooled_hypothesis_count(n, max_hypotheses)).stride;
  return 0;
}

extern "C" int hrp_pnp_solve_pooled(const float* pts2d, const float* pts3d, const float* K, int K_stride, const unsigned char* valid, int B,
                                    int n, double reproj_error, int min_inliers, int max_hypotheses, unsigned seed, int refine_all,
                                    void* workspace, size_t workspace_bytes, float* P6d, unsigned char* inliers, int* status, float* rms,
                                    float* cov, void* stream) {
  HRP_REQUIRE(pts2d && pts3d && K && P6d && inliers && status && rms && workspace, "pnp_solve_pooled: bad args");
  if (int rc = pooled_args("pnp_solve_pooled", B, n, max_hypotheses)) return rc;
  HRP_REQUIRE(K_stride == 0 || K_stride == 9, "pnp_solve_pooled: K stride %d (0 or 9)", K_stride);
  HRP_REQUIRE(reproj_error > 0.0 && reproj_error <= 1e150, "pnp_solve_pooled: reprojection threshold %g px (positive, finite)", reproj_error);
  HRP_REQUIRE(min_inliers >= 4 && min_inliers <= n, "pnp_solve_pooled: min_inliers %d (4..%d)", min_inliers, n);
  const int hmax = pnpmin::pooled_hypothesis_count(n, max_hypotheses);
  const PooledLayout L = pooled_layout(n, hmax);
  HRP_REQUIRE(workspace_bytes >= (size_t)B * L.stride, "pnp_solve_pooled: workspace of %zu bytes, %zu needed", workspace_bytes,
              (size_t)B * L.stride);
  HRP_REQUIRE((uintptr_t)workspace % 16 == 0, "pnp_solve_pooled: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  hipLaunchKernelGGL(pnp_pooled_compact_kernel, dim3(B), dim3(POOL_THREADS), 0, s, pts2d, pts3d, K, K_stride, valid, n, max_hypotheses, ws, L);
  hipLaunchKernelGGL(pnp_pooled_score_kernel, dim3(cdiv(hmax, POOL_LANES), B), dim3(POOL_LANES), 0, s, pts2d, pts3d, K, K_stride, n,
                     reproj_error, max_hypotheses, seed, ws, L);
  hipLaunchKernelGGL(pnp_pooled_fit_kernel, dim3(B), dim3(POOL_THREADS), 0, s, pts2d, pts3d, K, K_stride, n, reproj_error, min_inliers,
                     refine_all, (const unsigned char*)ws, L, P6d, inliers, status, rms, cov);
  return check_launch("pnp_solve_pooled");
}
