// bf16 instantiations of the batched tile convolution (conv_batch.h) and the parity-fused stride-2 data gradient (conv_parity.h).
#include "conv_parity.h"
namespace hrp {
int conv_batch_prepare_bf16(const hrp_conv_desc* descs, int n, void* table, hrp_batch_info* info) {
  // complete parity quadruples of 3x3 stride-2 data gradients, whatever their tap counts: one fused problem per layer
  const int rc = conv_parity_prepare(descs, n, table, info);
  return rc != PARITY_NOT_FUSED ? rc : conv_batch_prepare_t<bf16_t>(descs, n, table, info);
}
int conv_batch_launch_bf16(const void* table_dev, const hrp_batch_info* info, hipStream_t s) {
  return info->variant == PARITY_VARIANT ? conv_parity_launch(table_dev, info, s) : conv_batch_launch_t<bf16_t>(table_dev, info, s);
}
int64_t conv_batch_table_bytes(int n) { return (int64_t)n * sizeof(ConvProblem); }
}

extern "C" int hrp_conv_parity_fusable(const hrp_conv_desc* d) {
  return d && hrp::parity_class_of(*d) >= 0 ? 1 : 0;
}

extern "C" int hrp_conv_parity_fuse_enable(int on) {
  const int prev = hrp::g_parity_fuse;
  hrp::g_parity_fuse = on ? 1 : 0;
  return prev;
}

extern "C" int hrp_batch_conv_parity_configs(const void* table_host, const hrp_batch_info* info, int32_t* out) {
  using namespace hrp;
  HRP_REQUIRE(table_host && info && out && info->family == HRP_BATCH_CONV && info->n >= 1 && info->n <= HRP_BATCH_MAX,
              "conv parity configs: needs a prepared HRP_BATCH_CONV table");
  if (info->variant != PARITY_VARIANT) return 0;
  const ConvProblem* tab = (const ConvProblem*)table_host;
  for (int i = 0; i < info->n / 4; ++i) out[i] = tab[i].cfg == 0 ? 1214 : tab[i].cfg == 1 ? 1114 : 2114;
  return info->n / 4;
}

#ifdef HRP_TIMELINE
// (the batched kernels of this translation unit stamp their own copy of the timeline array)
extern "C" int hrp_debug_conv_timeline_batch(void* dst, int nblocks, int clear) {
  if (dst) (void)hipMemcpyFromSymbol(dst, HIP_SYMBOL(hrp::g_conv_timeline), sizeof(unsigned long long) * 8 * nblocks);
  if (clear) {
    void* p = nullptr;
    (void)hipGetSymbolAddress(&p, HIP_SYMBOL(hrp::g_conv_timeline));
    (void)hipMemset(p, 0, sizeof(unsigned long long) * 8192 * 8);
  }
  return 0;
}
#endif
