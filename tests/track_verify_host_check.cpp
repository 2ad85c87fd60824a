// Host check program of the tracker's verification step (track_verify in csrc/track_core.h), built by
// tests/test_track_verify_host.py with the host compiler and -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off.
// The same functions the kernel of hrp_track_verify calls.
//   track_verify_host_check run IN OUT    track_verify of every case in IN; status, have, counts, sums and the state to OUT
//   track_verify_host_check sizeof        sizeof(hrp_track_verify_desc) and the values of the HRP_VERIFY_* constants
// A case: int32 [nkp, have, hm, wm, use_alpha, nb, samples, min_fg, min_samples], float [min_prob], double [scale x, scale y,
// extend_ratio 0, extend_ratio 1, min_support, min_coverage, min_iou], int32 bones [nb][2], float mask [hm][wm], float alpha [hm][wm]
// (only with use_alpha), double state [nkp][2].
// Every array is a heap allocation of exactly its size, so a read outside the mask stops the program under ASan; a float -> int
// conversion of an unchecked value stops it under UBSan.
#include <stddef.h>
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
    int32_t h[9];
    float min_prob;
    double v[7];
    if (fread(h, 4, 9, f) != 9 || fread(&min_prob, 4, 1, f) != 1 || fread(v, 8, 7, f) != 7) return 2;
    const int nkp = h[0], hm = h[2], wm = h[3], nb = h[5], S = h[6];
    if (nkp < 1 || nkp > HRP_TRACK_MAX_KP || hm < 1 || wm < 1 || hm > HRP_TRACK_MAX_SIZE || wm > HRP_TRACK_MAX_SIZE || nb < 0 ||
        nb > HRP_TRACK_MAX_BONES || S < 1 || S > HRP_TRACK_MAX_SAMPLES)
      return 2;
    const size_t px = (size_t)hm * wm;
    int32_t(*bones)[2] = (int32_t(*)[2])exact<int32_t>(2 * nb);
    float* mask = exact<float>(px);
    float* alpha = h[4] ? exact<float>(px) : nullptr;
    double* state = exact<double>(2 * nkp);
    if (fread(bones, 4, 2 * nb, f) != (size_t)(2 * nb) || fread(mask, 4, px, f) != px) return 2;
    if (alpha && fread(alpha, 4, px, f) != px) return 2;
    if (fread(state, 8, 2 * nkp, f) != (size_t)(2 * nkp)) return 2;
    int32_t have = h[1], counts[4];
    double sums[3];
    const int32_t st = track::track_verify(state, nkp, have, v[0], v[1], mask, alpha, hm, wm, bones, nb, S, v[2], v[3], min_prob, h[7],
                                           h[8], v[4], v[5], v[6], counts, sums);
    fwrite(&st, 4, 1, o);
    fwrite(&have, 4, 1, o);
    fwrite(counts, 4, 4, o);
    fwrite(sums, 8, 3, o);
    fwrite(state, 8, 2 * nkp, o);
    free(bones);
    free(mask);
    free(alpha);
    free(state);
  }
  fclose(f);
  fclose(o);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "sizeof")) {
    printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d\n", sizeof(hrp_track_verify_desc), offsetof(hrp_track_verify_desc, B),
           offsetof(hrp_track_verify_desc, bones), offsetof(hrp_track_verify_desc, scale), offsetof(hrp_track_verify_desc, min_prob),
           HRP_VERIFY_SKIPPED, HRP_VERIFY_KEPT, HRP_VERIFY_UNDECIDED, HRP_VERIFY_DROPPED, HRP_VERIFY_FAIL_SUPPORT,
           HRP_VERIFY_FAIL_COVERAGE, HRP_VERIFY_FAIL_IOU, HRP_TRACK_MAX_BONES, HRP_TRACK_MAX_SAMPLES);
    return 0;
  }
  fprintf(stderr, "usage: track_verify_host_check run IN OUT | sizeof\n");
  return 2;
}
