// Parity-fused data gradient of the 3x3 stride-2 layers (bf16): the four output-parity problems of a layer
// (conv_geometry.parity_classes: 1 / 2 / 2 / 4 taps, or all padded to 4) are ONE 3x3 stride-1 tile program on the dy grid -
// nine taps, offsets {0, +1}^2, each tap's product added to the accumulators of its class (conv_tile_body's PF flag).  A
// workgroup stages the dy halo tile and the nine-tap weight slab once per K chunk instead of four times, runs 9 tap products
// per dy pixel instead of 16 and stores whole dx rows.  Within a class the additions keep the order of the class launch
// (chunk, the class's taps in ky-major order, k-step), so every dx element is bit for bit what the four launches write.
//
// A kernel of its own: the union of the three fused bodies and nothing else, so that their 4 x CT x PT accumulator sets
// never enter the register maximum of conv_batch_kernel.
#pragma once
#include "conv_batch.h"

namespace hrp {

constexpr int PARITY_VARIANT = 209;      // hrp_batch_info.variant of a fused launch
constexpr int PARITY_NOT_FUSED = -200;   // conv_parity_prepare: the batch is not made of complete quadruples - take the ordinary path
static int g_parity_fuse = 1;            // hrp_conv_parity_fuse_enable: 0 sends every batch down the ordinary path (A/B measurements)

// (tap slot, dy, dx) of class (py, px), k = 3, stride 2, pad 1: conv_geometry.class_taps(3, 1, py, px), ky-major
struct ParityTap { int dy, dx, slot; };
static const ParityTap PARITY_TAPS[4][4] = {
    {{0, 0, 4}},
    {{0, 1, 3}, {0, 0, 5}},
    {{1, 0, 1}, {0, 0, 7}},
    {{1, 1, 0}, {1, 0, 2}, {0, 1, 6}, {0, 0, 8}}};
static const int PARITY_NTAPS[4] = {1, 2, 2, 4};

// cfg 0: 256 dy pixels x 32 dx channels, 1: 128 x 32, 2: 128 x 64
__global__ __launch_bounds__(256, 2) void conv_parity_kernel(const ConvProblem* __restrict__ tab, const BatchHdr h) {
  int base;
  const int g = batch_find(h, blockIdx.x, base);
  const ConvProblem& P = tab[g];
  const int bid = (int)blockIdx.x - base;
  switch (P.cfg) {
    case 0: conv_tile_body<bf16_t, 1, 2, 1, 4, 9, false, true, true>(P.d, P.t, bid, 1, 0); break;
    case 1: conv_tile_body<bf16_t, 1, 1, 1, 4, 9, false, true, true>(P.d, P.t, bid, 1, 0); break;
    default: conv_tile_body<bf16_t, 2, 1, 1, 4, 9, false, true, true>(P.d, P.t, bid, 1, 0); break;
  }
}

// Parity class (0 .. 3) of a problem the fused kernel can take as one of four, -1 otherwise.  Host only; no pointer is read.
static int parity_class_of(const hrp_conv_desc& d) {
  if (d.dtype != HRP_BF16 || d.in_stride != 1 || d.out_stride != 2) return -1;
  if (d.out_off_y < 0 || d.out_off_y > 1 || d.out_off_x < 0 || d.out_off_x > 1) return -1;
  const int cls = d.out_off_y * 2 + d.out_off_x, real = PARITY_NTAPS[cls];
  if (d.w_ntaps != 9 && d.w_ntaps != 10) return -1;
  if (d.ntaps != real && !(d.ntaps == 4 && d.w_ntaps == 10)) return -1;
  for (int i = 0; i < real; ++i)
    if (d.dy[i] != PARITY_TAPS[cls][i].dy || d.dx[i] != PARITY_TAPS[cls][i].dx || d.wtap[i] != PARITY_TAPS[cls][i].slot) return -1;
  for (int i = real; i < d.ntaps; ++i)      // padding taps: the zero slot, any offset inside the halo
    if (d.wtap[i] != 9 || d.dy[i] < 0 || d.dy[i] > 1 || d.dx[i] < 0 || d.dx[i] > 1) return -1;
  // dx with even H and W: the four classes walk the same Ho x Wo grid
  if (d.N < 1 || d.Ho < 1 || d.Wo < 1 || d.y_H != 2 * d.Ho || d.y_W != 2 * d.Wo) return -1;
  if (d.Cin < 16 || d.Cin % 16 || d.x_pitch % 8 || d.Cout < 8 || d.Cout % 8 || d.y_pitch % 8 || d.w_cout_pad % 32 || d.w_cout_pad < d.Cout) return -1;
  if (d.res && d.res_pitch % 8) return -1;
  if (d.bias || d.scale || d.shift || d.stats || d.relu || d.bnb_x || d.bnb_mask || d.bnb_consts || d.bnb_stats) return -1;
  if (d.pro_mode || d.pro_x2 || d.pro_side || d.pro_side2 || d.pro_mask || d.res_mask || d.tail_mode) return -1;
  return cls;
}

static bool parity_same_layer(const hrp_conv_desc& a, const hrp_conv_desc& b) {
  return a.x == b.x && a.w == b.w && a.y == b.y && a.res == b.res && a.N == b.N && a.H == b.H && a.W == b.W && a.Cin == b.Cin &&
         a.x_pitch == b.x_pitch && a.Ho == b.Ho && a.Wo == b.Wo && a.Cout == b.Cout && a.y_H == b.y_H && a.y_W == b.y_W &&
         a.y_pitch == b.y_pitch && (!a.res || a.res_pitch == b.res_pitch) && a.w_ntaps == b.w_ntaps && a.w_cout_pad == b.w_cout_pad;
}

// The four class problems of a layer -> the one nine-tap problem on the dy grid (taps class by class: pf_tap_class).
static hrp_conv_desc parity_fused_desc(const hrp_conv_desc& c0) {
  hrp_conv_desc f = c0;
  f.out_off_y = f.out_off_x = 0;
  f.ntaps = 9;
  int k = 0;
  for (int cls = 0; cls < 4; ++cls)
    for (int i = 0; i < PARITY_NTAPS[cls]; ++i, ++k) {
      f.dy[k] = PARITY_TAPS[cls][i].dy; f.dx[k] = PARITY_TAPS[cls][i].dx; f.wtap[k] = PARITY_TAPS[cls][i].slot;
    }
  for (; k < HRP_MAX_TAPS; ++k) f.dy[k] = f.dx[k] = f.wtap[k] = 0;
  return f;
}

template <int CT, int PT>
static int parity_plan_cfg(const hrp_conv_desc& f, ConvProblem& P, int& lds) {
  const int rc = plan_cfg<bf16_t, CT, PT, 1, 4, 9>(f, P.t, lds, false);
  if (rc != HRP_OK) return rc;
  // the LDS image of an epilogue pass holds two dx pixels per dy pixel
  const int image = round_up(2 * (32 * PT * 4) * (32 * CT * 2 + 16), 16);
  if (image > P.t.lds_stats_off) { lds += image - P.t.lds_stats_off; P.t.lds_stats_off = image; }
  return lds > 160 * 1024 ? -100 : HRP_OK;
}

// small: the 128-pixel tile with 32 channels for every problem (twice the workgroups of the large tiles)
static int parity_plan_one(const hrp_conv_desc& f, ConvProblem& P, int& lds, bool small) {
  g_conv_lds_budget_kb = 76;
  int rc = -100;
  if (!small && f.Cout <= 32) { rc = parity_plan_cfg<1, 2>(f, P, lds); P.cfg = 0; }
  if (!small && f.Cout > 32) { rc = parity_plan_cfg<2, 1>(f, P, lds); P.cfg = 2; }
  if (rc == -100) { rc = parity_plan_cfg<1, 1>(f, P, lds); P.cfg = 1; }
  return rc;
}

// -> HRP_OK (table and info filled: one entry per quadruple), PARITY_NOT_FUSED, or an error of the descriptor check.
static int conv_parity_prepare(const hrp_conv_desc* descs, int n, void* table, hrp_batch_info* info) {
  if (n % 4 || !g_parity_fuse) return PARITY_NOT_FUSED;
  int cls[HRP_BATCH_MAX], quad[HRP_BATCH_MAX], first[HRP_BATCH_MAX / 4], seen[HRP_BATCH_MAX / 4], nq = 0;
  for (int i = 0; i < n; ++i) {
    if (!descs[i].x || !descs[i].w || !descs[i].y) return PARITY_NOT_FUSED;      // (conv_check of the ordinary path reports it)
    cls[i] = parity_class_of(descs[i]);
    if (cls[i] < 0 || (uintptr_t)descs[i].x % 16 || (uintptr_t)descs[i].w % 16 || (uintptr_t)descs[i].y % 16 || (uintptr_t)descs[i].res % 16)
      return PARITY_NOT_FUSED;
    int q = 0;
    while (q < nq && !parity_same_layer(descs[first[q]], descs[i])) ++q;
    if (q == nq) {
      if (nq == n / 4) return PARITY_NOT_FUSED;
      first[nq] = i; seen[nq] = 0; ++nq;
    }
    if (seen[q] & (1 << cls[i])) return PARITY_NOT_FUSED;
    seen[q] |= 1 << cls[i];
    quad[i] = q;
  }
  for (int q = 0; q < nq; ++q)
    if (seen[q] != 15) return PARITY_NOT_FUSED;
  if (nq != n / 4) return PARITY_NOT_FUSED;

  ConvProblem probs[HRP_BATCH_MAX / 4];
  long weight[HRP_BATCH_MAX / 4];
  int lds_max = 0, total = 0;
  // the largest tiles first; a launch that then stays below two workgroups per CU takes the small tile everywhere: it is one
  // round of workgroups either way, and the small tile's workgroup is the shorter one
  const char* mw = getenv("HRP_PARITY_MIN_WGS");      // (read per call: tests reach the large tiles with small problems)
  const int min_wgs = mw ? atoi(mw) : 512;
  for (int pass = 0; pass < 2; ++pass) {
    lds_max = 0; total = 0;
    for (int q = 0; q < nq; ++q) {
      memset(&probs[q], 0, sizeof(ConvProblem));
      probs[q].d = parity_fused_desc(descs[first[q]]);
      int lds = 0;
      const int rc = parity_plan_one(probs[q].d, probs[q], lds, pass == 1);
      if (rc == -100) return PARITY_NOT_FUSED;
      if (rc != HRP_OK) return rc;
      lds_max = lds > lds_max ? lds : lds_max;
      total += probs[q].t.nblocks;
      const int ct = probs[q].cfg == 2 ? 2 : 1, pt = probs[q].cfg == 0 ? 2 : 1;
      weight[q] = (long)cdiv(probs[q].d.Cin * 2, ROW) * 9 * ct * pt;
    }
    if (total >= min_wgs) break;
  }
  int order[HRP_BATCH_MAX / 4];
  for (int q = 0; q < nq; ++q) order[q] = q;
  for (int i = 1; i < nq; ++i)   // stable insertion sort, heaviest first
    for (int j = i; j > 0 && weight[order[j]] > weight[order[j - 1]]; --j) { int t_ = order[j]; order[j] = order[j - 1]; order[j - 1] = t_; }
  ConvProblem* tab = (ConvProblem*)table;
  memset(tab, 0, sizeof(ConvProblem) * n);
  int blk = 0;
  for (int k = 0; k < nq; ++k) {
    info->blk0[k] = blk;
    blk += probs[order[k]].t.nblocks;
    tab[k] = probs[order[k]];
  }
  for (int k = nq; k <= n; ++k) info->blk0[k] = blk;      // table entries past the fused count: parked at the grid size
  info->grid = blk;
  info->lds_bytes = lds_max;
  info->variant = PARITY_VARIANT;
  return HRP_OK;
}

static int conv_parity_launch(const void* table_dev, const hrp_batch_info* info, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)conv_parity_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  const BatchHdr h = make_hdr(info->blk0, info->n);
  hipLaunchKernelGGL(conv_parity_kernel, dim3(info->grid), dim3(256), info->lds_bytes, s, (const ConvProblem*)table_dev, h);
  return check_launch("conv_parity_kernel");
}

}  // namespace hrp
