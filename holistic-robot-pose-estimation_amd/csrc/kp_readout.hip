// CtRNet key-point read-out (reference lib/models/ctrnet/keypoint_seg_resnet.py:29-33, 75-100, 137-143), forward only:
//   heat = ConvTranspose2d(Cin -> k, 4, stride 2, padding 1)(x) + bias      [B, k, 2 Hin, 2 Win]   (interpolate(scale 1) = identity)
//   p    = softmax(heat) over the 2 Hin * 2 Win positions of every (b, c)
//   kp   = ((sum p xc) - lim[0], (sum p yc) - lim[2]) * (width // 2, height // 2),  xc / yc = fp32 linspace(-1, 1, 2 Win / 2 Hin)
// The heat-map never exists in memory: a logit near 8 has a bf16 quantum of 2^-5, and a soft-argmax turns a logit error eps into up
// to (e^{2 eps} - 1) W / 2 pixels, so the logits stay fp32 accumulators of the matrix cores and feed an online softmax
// from registers.
//
// kp_readout_kernel, grid (row strips of the INPUT, B), four waves = the four output parities (oy & 1, ox & 1).  A transposed 4 x 4
// stride-2 convolution is, per output parity, a 2 x 2-tap sum over the input (no zero insertion):
//   out[2q + py, 2r + px] = sum_{ty, tx} x[q + dy(py, ty), r + dx(px, tx)] . w[:, c, ky, kx],   dy = (py ? 1 : 0) - ty, ky = py + 1 - 2 dy
// i.e. a GEMM [positions of the strip] x [K = 4 Cin] x [32 channel slots] whose A rows are read straight from the NHWC feature
// (16 bytes per lane: the fragment's k run is contiguous in memory) and whose B fragments come from hrp_kp_readout_pack's layout
//   [parity 4][tap 4][Cin / V][32 channel slots][V]      V = 8 (bf16) / 4 (fp32) = one lane's k run
// mfma_f32_32x32x16_bf16 / mfma_f32_32x32x2f32 leave the channel on the lane (col = lane & 31) and 16 positions in the registers
// (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so the softmax partial (max, sum e, sum e xc, sum e yc) of a channel is plain
// per-lane arithmetic; lane halves, waves and strips are combined in a fixed order (no atomics): the result is bit-reproducible.
// kp_combine_kernel folds the strips' partials (float64, strip order) and applies lim and the scale.
#include "hrp_common.h"

namespace hrp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int KP_THREADS = 256;
constexpr int KP_SLOTS = 32;             // channel slots of one MFMA column tile = HRP_TRACK_MAX_KP
constexpr int KP_MT = 2;                 // 32-position tiles in flight per wave (they share every B fragment)
static_assert(KP_SLOTS == HRP_TRACK_MAX_KP, "one MFMA column tile holds every key-point channel");

template <typename T> struct KpElem;
template <> struct KpElem<bf16_t> {
  static constexpr int V = 8;
  using Vec = bf16x8;
  __device__ static __forceinline__ void mma(const Vec& a, const Vec& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  __device__ static __forceinline__ uint16_t cvt(float v) { return f2bf(v); }
  using Store = uint16_t;
};
template <> struct KpElem<float> {
  static constexpr int V = 4;
  using Vec = f32x4;
  // lane (r, h) holds channels 4h .. 4h + 3 of an 8-channel step: four K = 2 products, k = (h, j)
  __device__ static __forceinline__ void mma(const Vec& a, const Vec& b, f32x16& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
  }
  __device__ static __forceinline__ float cvt(float v) { return v; }
  using Store = float;
};

// tap ty (0, 1) of output parity p: input offset and kernel index (file header)
__host__ __device__ inline int tap_d(int p, int t) { return (p ? 1 : 0) - t; }
__host__ __device__ inline int tap_k(int p, int t) { return p + 1 - 2 * tap_d(p, t); }

template <typename T>
__global__ void kp_pack_kernel(const float* __restrict__ w, int Cin, int k, typename KpElem<T>::Store* __restrict__ out) {
  constexpr int V = KpElem<T>::V;
  const int64_t n = (int64_t)16 * Cin * KP_SLOTS;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int j = (int)(e % V), c = (int)((e / V) % KP_SLOTS);
  const int64_t g = e / (V * KP_SLOTS);
  const int cg = (int)(g % (Cin / V)), pt = (int)(g / (Cin / V));      // pt = parity * 4 + tap
  const int par = pt >> 2, tap = pt & 3;
  const int ky = tap_k(par >> 1, tap >> 1), kx = tap_k(par & 1, tap & 1);
  const int ci = cg * V + j;
  const float v = c < k ? w[(((int64_t)ci * k + c) * 4 + ky) * 4 + kx] : 0.f;
  out[e] = KpElem<T>::cvt(v);
}

// torch.linspace(-1, 1, n) in fp32 (ATen RangeFactories: step = 2 / (n - 1); from the start below the middle, from the end above)
__device__ __forceinline__ float lin11(int i, int n, float step) {
  return i < n / 2 ? __fadd_rn(-1.f, __fmul_rn(step, (float)i)) : __fsub_rn(1.f, __fmul_rn(step, (float)(n - 1 - i)));
}

struct KpPart {
  float m, s, sx, sy;
};
// a then b, in that order, on every lane that combines the pair
__device__ __forceinline__ KpPart kp_merge(const KpPart& a, const KpPart& b) {
  const float M = fmaxf(a.m, b.m);
  const float fa = a.m == -INFINITY ? 0.f : expf(a.m - M), fb = b.m == -INFINITY ? 0.f : expf(b.m - M);
  KpPart r;
  r.m = M;
  r.s = a.s * fa + b.s * fb;
  r.sx = a.sx * fa + b.sx * fb;
  r.sy = a.sy * fa + b.sy * fb;
  return r;
}

template <typename T>
__global__ void __launch_bounds__(KP_THREADS) kp_readout_kernel(const void* __restrict__ xv, int Hin, int Win, int Cin, int pitch,
                                                                const void* __restrict__ wv, const float* __restrict__ bias, int k,
                                                                float* __restrict__ ws) {
  using E = KpElem<T>;
  using Vec = typename E::Vec;
  constexpr int V = E::V;
  __shared__ KpPart part[4][KP_SLOTS];
  const typename E::Store* x = (const typename E::Store*)xv;
  const typename E::Store* wp = (const typename E::Store*)wv;
  const int strip = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int par = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int py = par >> 1, px = par & 1;
  const int r0 = strip * HRP_KP_STRIP_ROWS, r1 = min(r0 + HRP_KP_STRIP_ROWS, Hin);
  const int P = (r1 - r0) * Win;                         // positions of this strip (>= 1)
  const int nsteps = Cin / (2 * V), ncg = Cin / V;
  const int Wo = 2 * Win, Ho = 2 * Hin;
  const float stepx = __fdiv_rn(2.f, (float)(Wo - 1)), stepy = __fdiv_rn(2.f, (float)(Ho - 1));
  const float bz = r < k ? bias[r] : 0.f;
  KpPart st = {-INFINITY, 0.f, 0.f, 0.f};
  Vec zero;
#pragma unroll
  for (int j = 0; j < V; ++j) zero[j] = 0;

  for (int base = 0; base < P; base += 32 * KP_MT) {
    f32x16 acc[KP_MT];
#pragma unroll
    for (int mt = 0; mt < KP_MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
    int q[KP_MT], c[KP_MT];
    bool valid[KP_MT];
#pragma unroll
    for (int mt = 0; mt < KP_MT; ++mt) {                 // this lane's A row: one input position per tile
      const int pi = base + mt * 32 + r;
      valid[mt] = pi < P;
      q[mt] = r0 + pi / Win;
      c[mt] = pi % Win;
    }
    for (int tap = 0; tap < 4; ++tap) {
      const int dy = tap_d(py, tap >> 1), dx = tap_d(px, tap & 1);
      const typename E::Store* ap[KP_MT];
      bool inb[KP_MT];
#pragma unroll
      for (int mt = 0; mt < KP_MT; ++mt) {
        const int iy = q[mt] + dy, ix = c[mt] + dx;
        inb[mt] = valid[mt] && iy >= 0 && iy < Hin && ix >= 0 && ix < Win;      // the transposed convolution's implicit zeros
        ap[mt] = x + (((int64_t)b * Hin + (inb[mt] ? iy : 0)) * Win + (inb[mt] ? ix : 0)) * pitch + h * V;
      }
      const typename E::Store* bp = wp + (((int64_t)(par * 4 + tap) * ncg + h) * KP_SLOTS + r) * V;
#pragma unroll 8
      for (int s = 0; s < nsteps; ++s) {
        const Vec bf = *(const Vec*)(bp + (int64_t)s * 2 * KP_SLOTS * V);
#pragma unroll
        for (int mt = 0; mt < KP_MT; ++mt) {
          const Vec af = inb[mt] ? *(const Vec*)(ap[mt] + s * 2 * V) : zero;
          E::mma(af, bf, acc[mt]);
        }
      }
    }
    // softmax partial of channel r over this lane's (up to) 32 positions: the maximum first, then one rescale of the running sums
    float lg[KP_MT][16], cx[KP_MT][16], cy[KP_MT][16];
    float tm = -INFINITY;
#pragma unroll
    for (int mt = 0; mt < KP_MT; ++mt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int pi = base + mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const bool ok = pi < P;
        const int qq = r0 + pi / Win, cc = pi % Win;
        lg[mt][i] = ok ? acc[mt][i] + bz : -INFINITY;
        cx[mt][i] = lin11(2 * cc + px, Wo, stepx);
        cy[mt][i] = lin11(2 * qq + py, Ho, stepy);
        tm = fmaxf(tm, lg[mt][i]);
      }
    if (tm > st.m) {                                     // (tm == -inf: no valid position on this lane, nothing to add)
      const float f = st.m == -INFINITY ? 0.f : expf(st.m - tm);
      st.s *= f;
      st.sx *= f;
      st.sy *= f;
      st.m = tm;
    }
    if (tm != -INFINITY) {
#pragma unroll
      for (int mt = 0; mt < KP_MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float e = lg[mt][i] == -INFINITY ? 0.f : expf(lg[mt][i] - st.m);
          st.s += e;
          st.sx += e * cx[mt][i];
          st.sy += e * cy[mt][i];
        }
    }
  }
  // lane halves (h = 0 first), then the four parities in order
  KpPart o;
  o.m = __shfl_xor(st.m, 32, 64);
  o.s = __shfl_xor(st.s, 32, 64);
  o.sx = __shfl_xor(st.sx, 32, 64);
  o.sy = __shfl_xor(st.sy, 32, 64);
  const KpPart both = h ? kp_merge(o, st) : kp_merge(st, o);
  if (h == 0) part[par][r] = both;
  __syncthreads();
  if (tid < k) {
    KpPart t = part[0][tid];
    for (int wv_ = 1; wv_ < 4; ++wv_) t = kp_merge(t, part[wv_][tid]);
    float* dst = ws + (((int64_t)b * gridDim.x + strip) * KP_SLOTS + tid) * 4;
    dst[0] = t.m;
    dst[1] = t.s;
    dst[2] = t.sx;
    dst[3] = t.sy;
  }
}

__global__ void kp_combine_kernel(const float* __restrict__ ws, int nstrips, int k, float lim0, float lim2, float sx, float sy,
                                  float* __restrict__ kp, float* __restrict__ ms) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (c >= k) return;
  const float* p = ws + ((int64_t)b * nstrips * KP_SLOTS + c) * 4;
  float M = -INFINITY;
  for (int s = 0; s < nstrips; ++s) M = fmaxf(M, p[(int64_t)s * KP_SLOTS * 4]);
  double S = 0.0, SX = 0.0, SY = 0.0;
  for (int s = 0; s < nstrips; ++s) {
    const float* e = p + (int64_t)s * KP_SLOTS * 4;
    const double f = exp((double)e[0] - (double)M);
    S += (double)e[1] * f;
    SX += (double)e[2] * f;
    SY += (double)e[3] * f;
  }
  const float xm = (float)(SX / S), ym = (float)(SY / S);
  kp[((int64_t)b * k + c) * 2] = __fmul_rn(__fsub_rn(xm, lim0), sx);          // keypoints - offset, then * scale (lines 142-143)
  kp[((int64_t)b * k + c) * 2 + 1] = __fmul_rn(__fsub_rn(ym, lim2), sy);
  if (ms) {
    ms[((int64_t)b * k + c) * 2] = M;
    ms[((int64_t)b * k + c) * 2 + 1] = (float)S;
  }
}

bool shape_ok(int B, int Hin, int Win) { return B >= 1 && B <= 65535 && Hin >= 1 && Hin <= HRP_TRACK_MAX_SIZE && Win >= 1 && Win <= HRP_TRACK_MAX_SIZE; }

}  // namespace
}  // namespace hrp

using namespace hrp;

extern "C" int hrp_kp_readout_pack(const float* weight, int Cin, int k, void* packed, int dtype, void* stream) {
  HRP_REQUIRE(weight && packed, "kp_readout_pack: null pointer");
  HRP_REQUIRE(Cin >= 32 && Cin % 32 == 0 && Cin <= (1 << 20), "kp_readout_pack: Cin %d is not a multiple of 32", Cin);
  HRP_REQUIRE(k >= 1 && k <= HRP_TRACK_MAX_KP, "kp_readout_pack: %d key-points, want 1 .. %d", k, HRP_TRACK_MAX_KP);
  HRP_REQUIRE(dtype == HRP_F32 || dtype == HRP_BF16 || dtype == HRP_F32X3, "kp_readout_pack: dtype %d", dtype);
  const int64_t n = (int64_t)16 * Cin * KP_SLOTS;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == HRP_BF16) hipLaunchKernelGGL((kp_pack_kernel<bf16_t>), grid, dim3(256), 0, (hipStream_t)stream, weight, Cin, k, (uint16_t*)packed);
  else hipLaunchKernelGGL((kp_pack_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, weight, Cin, k, (float*)packed);
  return check_launch("kp_readout_pack");
}

extern "C" int64_t hrp_kp_readout_ws(int B, int Hin) {
  if (B < 1 || Hin < 1) return 0;
  return (int64_t)B * cdiv(Hin, HRP_KP_STRIP_ROWS) * KP_SLOTS * 4 * (int64_t)sizeof(float);
}

extern "C" int hrp_kp_readout_fwd(const void* x, int dtype, int B, int Hin, int Win, int Cin, int pitch, const void* packed,
                                  const float* bias, int k, float lim0, float lim2, float scale_x, float scale_y, float* kp, float* ms,
                                  void* ws, int64_t ws_bytes, void* stream) {
  HRP_REQUIRE(x && packed && bias && kp && ws, "kp_readout_fwd: null pointer");
  HRP_REQUIRE(B >= 1 && Hin >= 1 && Win >= 1, "kp_readout_fwd: empty map (B %d, %d x %d)", B, Hin, Win);
  HRP_REQUIRE(shape_ok(B, Hin, Win), "kp_readout_fwd: B %d, map %d x %d out of range", B, Hin, Win);
  HRP_REQUIRE(Cin >= 32 && Cin % 32 == 0 && Cin <= (1 << 20), "kp_readout_fwd: Cin %d is not a multiple of 32", Cin);
  HRP_REQUIRE(k >= 1 && k <= HRP_TRACK_MAX_KP, "kp_readout_fwd: %d key-points, want 1 .. %d", k, HRP_TRACK_MAX_KP);
  HRP_REQUIRE(dtype == HRP_F32 || dtype == HRP_BF16 || dtype == HRP_F32X3, "kp_readout_fwd: dtype %d", dtype);
  const int V = dtype == HRP_BF16 ? 8 : 4;
  HRP_REQUIRE(pitch >= Cin && pitch % V == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)packed % 16 == 0,
              "kp_readout_fwd: pitch %d (want >= Cin, a multiple of %d) / 16-byte aligned operands", pitch, V);
  HRP_REQUIRE(ws_bytes >= hrp_kp_readout_ws(B, Hin), "kp_readout_fwd: workspace of %lld bytes, want %lld", (long long)ws_bytes,
              (long long)hrp_kp_readout_ws(B, Hin));
  const int nstrips = cdiv(Hin, HRP_KP_STRIP_ROWS);
  const dim3 grid(nstrips, B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == HRP_BF16)
    hipLaunchKernelGGL((kp_readout_kernel<bf16_t>), grid, dim3(KP_THREADS), 0, st, x, Hin, Win, Cin, pitch, packed, bias, k, (float*)ws);
  else
    hipLaunchKernelGGL((kp_readout_kernel<float>), grid, dim3(KP_THREADS), 0, st, x, Hin, Win, Cin, pitch, packed, bias, k, (float*)ws);
  hipLaunchKernelGGL(kp_combine_kernel, dim3(B), dim3(KP_SLOTS), 0, st, (const float*)ws, nstrips, k, lim0, lim2, scale_x, scale_y, kp, ms);
  return check_launch("kp_readout_fwd");
}
