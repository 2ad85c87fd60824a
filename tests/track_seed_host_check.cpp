// Host check program of the tracker's acquisition step (track_seed in csrc/track_core.h), built by tests/test_track_seed_host.py with
// the host compiler and -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off.  The same function the kernel of
// hrp_track_seed calls.
//   track_seed_host_check run IN OUT      track_seed of every case in IN; status, have and the state to OUT
// A case: int32 [nkp, have, hm, wm, use_mask, use_ms, min_inside, force, W, H], float [min_prob, min_peak], double [inv_sx, inv_sy],
// float det [nkp][2], float ms [nkp][2], float mask [hm][wm] (only with use_mask), double state [nkp][2].
// Every array is a heap allocation of exactly its size, so a read outside the mask or a write outside the state stops the
// program under ASan; a float -> int conversion of an unchecked value stops it under UBSan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "track_core.h"

namespace {

template <typename T>
T* exact(size_t n) {                      // (n == 0: a one-element block that nothing may touch is still a valid pointer)
  return (T*)malloc((n ? n : 1) * sizeof(T));
}

int run(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  FILE* o = fopen(out, "wb");
  if (!f || !o) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  for (int32_t i = 0; i < n; ++i) {
    int32_t h[10];
    float thr[2];
    double inv[2];
    if (fread(h, 4, 10, f) != 10 || fread(thr, 4, 2, f) != 2 || fread(inv, 8, 2, f) != 2) return 2;
    const int nkp = h[0], hm = h[2], wm = h[3];
    if (nkp < 1 || nkp > HRP_TRACK_MAX_KP || hm < 0 || wm < 0 || hm > HRP_TRACK_MAX_SIZE || wm > HRP_TRACK_MAX_SIZE) return 2;
    float* det = exact<float>(2 * nkp);
    float* ms = exact<float>(2 * nkp);
    float* mask = h[4] ? exact<float>((size_t)hm * wm) : nullptr;
    double* state = exact<double>(2 * nkp);
    if (fread(det, 4, 2 * nkp, f) != (size_t)(2 * nkp) || fread(ms, 4, 2 * nkp, f) != (size_t)(2 * nkp)) return 2;
    if (mask && fread(mask, 4, (size_t)hm * wm, f) != (size_t)hm * wm) return 2;
    if (fread(state, 8, 2 * nkp, f) != (size_t)(2 * nkp)) return 2;
    int32_t have = h[1];
    const int32_t st = track::track_seed(det, nkp, inv[0], inv[1], mask, hm, wm, thr[0], h[5] ? ms : nullptr, thr[1], h[6], h[7], h[8],
                                         h[9], state, have);
    fwrite(&st, 4, 1, o);
    fwrite(&have, 4, 1, o);
    fwrite(state, 8, 2 * nkp, o);
    free(det);
    free(ms);
    free(mask);
    free(state);
  }
  fclose(f);
  fclose(o);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: track_seed_host_check run IN OUT\n");
  return 2;
}
