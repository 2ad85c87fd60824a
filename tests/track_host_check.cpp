// Host check program of the streaming tracker's core (csrc/track_core.h), built by tests/test_track_host.py with the host compiler and
// -fsanitize=address,undefined -fno-sanitize-recover -ffp-contract=off.  The same functions the kernels of csrc/track.hip call.
//   track_host_check sizeof                 prints sizeof(hrp_track_geom)
//   track_host_check geom IN OUT            track_geometry of every case in IN; records, K and k_value to OUT
//   track_host_check pixels IN OUT          track_geometry + track_pixel over both views of one case with its frame
//   track_host_check hostile                hostile estimates, wrong records and track_update; one line per case, exit 1 on a failure
// Every frame is allocated at exactly H * W * 3 bytes, so a read outside it stops the program under ASan.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "track_core.h"

namespace {

struct Case {
  int32_t W, H, nkp, have, h0, w0, h1, w1, two, mode;
  double er[2];
  float K[9];
  std::vector<double> kp;
};

struct Result {
  hrp_track_geom g;
  float K_root[9], K_other[9], k;
};

bool read_case(FILE* f, Case& c) {
  if (fread(&c.W, 4, 10, f) != 10 || fread(c.er, 8, 2, f) != 2 || fread(c.K, 4, 9, f) != 9) return false;
  if (c.nkp < 1 || c.nkp > HRP_TRACK_MAX_KP) return false;
  c.kp.resize(2 * c.nkp);
  return fread(c.kp.data(), 8, c.kp.size(), f) == c.kp.size();
}

Result run(const Case& c) {
  Result r;
  memset(&r, 0, sizeof r);
  const track::Views vw = {{c.h0, c.two ? c.h1 : c.h0}, {c.w0, c.two ? c.w1 : c.w0}, c.two};
  track::track_geometry(c.kp.data(), c.nkp, c.have, c.K, c.W, c.H, vw, c.er[0], c.er[1], c.mode, r.g, r.K_root, r.K_other, r.k);
  return r;
}

// every pixel of an h x w view, NCHW
std::vector<uint8_t> view_pixels(const uint8_t* frame, int W, int H, const hrp_track_geom& g, int h, int w) {
  std::vector<uint8_t> out((size_t)3 * h * w);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      uint8_t rgb[3];
      track::track_pixel(frame, W, H, g, h, w, x, y, rgb);
      for (int ch = 0; ch < 3; ++ch) out[((size_t)ch * h + y) * w + x] = rgb[ch];
    }
  return out;
}

int failures = 0;

void expect(bool ok, const char* name, const char* what) {
  if (!ok) {
    printf("FAIL %s: %s\n", name, what);
    ++failures;
  }
}

// a frame of exactly H * W * 3 bytes on the heap (ASan's red zones lie directly around it)
uint8_t* make_frame(int W, int H) {
  uint8_t* f = (uint8_t*)malloc((size_t)W * H * 3);
  for (size_t i = 0; i < (size_t)W * H * 3; ++i) f[i] = (uint8_t)(i * 2654435761u >> 24);
  return f;
}

void hostile_case(const char* name, int W, int H, const std::vector<double>& kp, int have, int want_status, bool want_whole,
                  const float* Kin = nullptr) {
  Case c;
  c.W = W, c.H = H, c.nkp = (int)kp.size() / 2, c.have = have, c.h0 = c.w0 = 16, c.h1 = c.w1 = 8, c.two = 1;
  c.er[0] = 0.2, c.er[1] = 0.13;
  const float K[9] = {615.f, 0.f, W / 2.f, 0.f, 615.f, H / 2.f, 0.f, 0.f, 1.f};
  memcpy(c.K, Kin ? Kin : K, sizeof K);
  c.kp = kp;
  uint8_t* frame = make_frame(W, H);
  for (int mode = 0; mode < 3; ++mode) {
    c.mode = mode;
    const Result r = run(c);
    const hrp_track_geom& g = r.g;
    const bool valid = 0 <= g.crop_x0 && g.crop_x0 < g.crop_x1 && g.crop_x1 <= W && 0 <= g.crop_y0 && g.crop_y0 < g.crop_y1 && g.crop_y1 <= H;
    const bool whole = g.crop_x0 == 0 && g.crop_y0 == 0 && g.crop_x1 == W && g.crop_y1 == H;
    printf("case %s mode %d status %d crop %d %d %d %d side %d k %.9g\n", name, mode, g.status, g.crop_x0, g.crop_y0, g.crop_x1, g.crop_y1,
           g.side, (double)r.k);
    expect(valid, name, "crop box outside the frame");
    expect(g.side == (g.crop_x1 - g.crop_x0 > g.crop_y1 - g.crop_y0 ? g.crop_x1 - g.crop_x0 : g.crop_y1 - g.crop_y0), name, "side");
    expect(r.k > 0.f && r.k <= std::numeric_limits<float>::max(), name, "k_value not finite and positive");
    // the status the case names holds for the default (extended) box: a box without area is refused there, not in origin mode
    if (mode == 0 && want_status >= 0) expect(g.status == want_status, name, "status");
    if (want_whole && mode == 0) expect(whole && (g.status & HRP_TRACK_NO_ESTIMATE), name, "whole frame expected");
    if (g.status & HRP_TRACK_NO_ESTIMATE) expect(whole, name, "HRP_TRACK_NO_ESTIMATE without the whole frame");
    const std::vector<uint8_t> a = view_pixels(frame, W, H, g, 16, 16), b = view_pixels(frame, W, H, g, 8, 8);
    // and the copy path (side == out) when the canvas is small enough to walk
    if (g.side <= 640) view_pixels(frame, W, H, g, g.side, g.side);
    (void)a, (void)b;
  }
  free(frame);
}

// records that no geometry would produce: track_pixel must still stay inside the frame
void wrong_records() {
  const int W = 37, H = 23;
  uint8_t* frame = make_frame(W, H);
  const int v[] = {-2147483647 - 1, -100000, -1, 0, 1, 22, 23, 36, 37, 38, 4096, 100000, 2147483647};
  const int n = sizeof v / sizeof v[0];
  long walked = 0;
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      for (int s = 0; s < n; ++s) {
        hrp_track_geom g;
        memset(&g, 0, sizeof g);
        g.crop_x0 = v[a], g.crop_y0 = v[b], g.crop_x1 = v[(a + b + 3) % n], g.crop_y1 = v[(a + s + 5) % n];
        g.side = v[s], g.off_x = v[(b + s) % n], g.off_y = v[(a + 2 * s) % n];
        for (int hw = 5; hw <= 40; hw += 35) {
          view_pixels(frame, W, H, g, hw, hw);
          ++walked;
        }
        if (g.side >= 1 && g.side <= 64) view_pixels(frame, W, H, g, g.side, g.side);
      }
  printf("wrong_records %ld walked\n", walked);
  free(frame);
}

void update_case(const char* name, const std::vector<float>& xyz, int min_inside, int want_have) {
  const int nkp = (int)xyz.size() / 3, W = 640, H = 480;
  const float K[9] = {615.f, 0.f, 320.f, 0.f, 615.f, 240.f, 0.f, 0.f, 1.f};
  std::vector<double> state(2 * nkp);
  std::vector<float> out(2 * nkp);
  const int have = track::track_update(xyz.data(), nkp, K, W, H, min_inside, state.data(), out.data());
  printf("update %s have %d\n", name, have);
  expect(have == want_have, name, "have");
}

int hostile() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const int NO = HRP_TRACK_NO_ESTIMATE, BAD = HRP_TRACK_BAD_BOX;
  const std::vector<double> good = {200, 150, 420, 330, 310, 200, 250, 300};
  auto with = [&](double v) {
    std::vector<double> k = good;
    k[3] = v;
    return k;
  };
  auto all = [&](double x, double y) { return std::vector<double>{x, y, x + 30, y + 10, x + 10, y + 40, x + 5, y + 5}; };
  hostile_case("good", 640, 480, good, 1, 0, false);
  hostile_case("nan", 640, 480, with(nan), 1, NO | BAD, true);
  hostile_case("plus_inf", 640, 480, with(inf), 1, NO | BAD, true);
  hostile_case("minus_inf", 640, 480, with(-inf), 1, NO | BAD, true);
  hostile_case("one_plus_1e300", 640, 480, with(1e300), 1, -1, false);          // one far point: the box is clamped, valid
  hostile_case("one_minus_1e300", 640, 480, with(-1e300), 1, -1, false);
  hostile_case("one_minus_1e9", 640, 480, with(-1e9), 1, -1, false);
  hostile_case("all_plus_1e300", 640, 480, std::vector<double>(8, 1e300), 1, NO | BAD, true);
  hostile_case("all_minus_1e300", 640, 480, std::vector<double>(8, -1e300), 1, NO | BAD, true);
  hostile_case("all_minus_1e9", 640, 480, std::vector<double>(8, -1e9), 1, NO | BAD, true);
  hostile_case("all_nan", 640, 480, std::vector<double>(8, nan), 1, NO | BAD, true);
  hostile_case("left", 640, 480, all(-500, 200), 1, NO | BAD, true);
  hostile_case("right", 640, 480, all(900, 200), 1, NO | BAD, true);
  hostile_case("above", 640, 480, all(300, -400), 1, NO | BAD, true);
  hostile_case("below", 640, 480, all(300, 700), 1, NO | BAD, true);
  // one point: a valid 150 x 120 crop, but the extended box has no area, so k_value is infinite and the estimate is refused
  hostile_case("one_point", 640, 480, std::vector<double>{300, 200, 300, 200, 300, 200, 300, 200}, 1, NO | BAD, true);
  hostile_case("have_0", 640, 480, good, 0, NO, true);
  hostile_case("have_0_nan_state", 640, 480, std::vector<double>(8, nan), 0, NO, true);
  hostile_case("frame_1x1", 1, 1, std::vector<double>{0.5, 0.5, 0.25, 0.75}, 1, -1, false);
  hostile_case("frame_1x1_have_0", 1, 1, good, 0, NO, true);
  hostile_case("frame_4096x1", 4096, 1, std::vector<double>{100, 0.5, 3000, 0.25}, 1, -1, false);
  hostile_case("frame_4096x1_have_0", 4096, 1, good, 0, NO, true);
  hostile_case("frame_1x4096_nan", 1, 4096, with(nan), 1, NO | BAD, true);
  const float Knan[9] = {NAN, 0.f, 320.f, 0.f, 615.f, 240.f, 0.f, 0.f, 1.f};
  hostile_case("K_nan", 640, 480, good, 1, NO | BAD, true, Knan);
  const float Kzero[9] = {0.f, 0.f, 320.f, 0.f, 0.f, 240.f, 0.f, 0.f, 1.f};
  hostile_case("K_zero", 640, 480, good, 1, NO | BAD, true, Kzero);
  wrong_records();
  const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
  update_case("good", {0.f, 0.f, 1.f, 0.1f, 0.1f, 1.2f, -0.1f, 0.05f, 0.9f}, 1, 1);
  update_case("nan", {0.f, 0.f, 1.f, fnan, 0.1f, 1.2f, -0.1f, 0.05f, 0.9f}, 1, 0);
  update_case("inf", {0.f, 0.f, 1.f, 0.1f, finf, 1.2f, -0.1f, 0.05f, 0.9f}, 1, 0);
  update_case("z_zero", {0.f, 0.f, 1.f, 0.1f, 0.1f, 0.f, -0.1f, 0.05f, 0.9f}, 1, 0);
  update_case("z_negative", {0.f, 0.f, 1.f, 0.1f, 0.1f, -1.2f, -0.1f, 0.05f, 0.9f}, 1, 0);
  update_case("all_outside", {5.f, 0.f, 1.f, 6.f, 0.1f, 1.2f, -7.f, 0.05f, 0.9f}, 1, 0);
  update_case("one_inside_of_two_wanted", {0.f, 0.f, 1.f, 6.f, 0.1f, 1.2f, -7.f, 0.05f, 0.9f}, 2, 0);
  update_case("two_inside_of_two_wanted", {0.f, 0.f, 1.f, 0.1f, 0.1f, 1.2f, -7.f, 0.05f, 0.9f}, 2, 1);
  update_case("tiny_z_overflows", {3e38f, 0.f, 1e-45f, 0.1f, 0.1f, 1.2f, -0.1f, 0.05f, 0.9f}, 1, 1);
  printf("hostile failures %d\n", failures);
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "sizeof") {
    printf("%zu\n", sizeof(hrp_track_geom));
    return 0;
  }
  if (cmd == "hostile") return hostile();
  if ((cmd != "geom" && cmd != "pixels") || argc != 4) {
    fprintf(stderr, "usage: track_host_check sizeof | hostile | geom IN OUT | pixels IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  int32_t n = 0;
  if (fread(&n, 4, 1, in) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    Case c;
    if (!read_case(in, c)) return 2;
    const Result r = run(c);
    fwrite(&r.g, sizeof r.g, 1, out);
    fwrite(r.K_root, 4, 9, out);
    fwrite(r.K_other, 4, 9, out);
    fwrite(&r.k, 4, 1, out);
    if (cmd == "pixels") {
      uint8_t* frame = (uint8_t*)malloc((size_t)c.W * c.H * 3);
      if (fread(frame, 1, (size_t)c.W * c.H * 3, in) != (size_t)c.W * c.H * 3) return 2;
      const std::vector<uint8_t> a = view_pixels(frame, c.W, c.H, r.g, c.h0, c.w0);
      fwrite(a.data(), 1, a.size(), out);
      if (c.two) {
        const std::vector<uint8_t> b = view_pixels(frame, c.W, c.H, r.g, c.h1, c.w1);
        fwrite(b.data(), 1, b.size(), out);
      }
      free(frame);
    }
  }
  fclose(in);
  fclose(out);
  return 0;
}
