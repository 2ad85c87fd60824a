// Stand-alone host check of csrc/jpeg_core.h (built and run by tests/test_jpeg_host.py; also the program to build with
// -fsanitize=address,undefined).  It runs the decoder core the way the kernels of csrc/jpeg.hip do - descriptor check, segment
// decode, inverse DCT per block, colour per pixel - on
//   1. every case of the input file: the frame must equal the recorded one, the status must be zero;
//   2. a seeded corpus of damaged copies of the cases flagged for it: the file truncated at every 97th length, and 200
//      single-byte changes inside the scan data.  Every run must return with the guard bytes around every buffer intact.
// Input (written by the test, native byte order): int32 ncases, then per case int32 damage, hrp_jpeg_image (scan_off relative to
// the file, the buffer offsets zero), int32 nseg, hrp_jpeg_segment[nseg], int64 nfile, the file, int64 nrgb, the frame.
// Output: one line per failure and a last line
//   "valid <cases> mismatch <n> | damaged <runs> guard <n> differ <n> silent <n> silent_truncated <n> trailing_only <n> checksum_only <n>"
// silent: damaged runs whose frame differs from the recorded one under status 0 (silent_truncated: the truncated files among
// them); checksum_only: those that differ and have nothing but HRP_JPEG_ERR_CHECKSUM - no decoder error tells them from a
// well-formed scan; trailing_only: those that have HRP_JPEG_WARN_TRAILING besides it and nothing else.  Exit status 1 for a mismatch or a guard violation, 2 for a bad input file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_core.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t GUARD_BYTE = 0xA5;

struct Guarded {      // n bytes with GUARD bytes of 0xA5 on either side, one allocation of exactly that size
  uint8_t* base = nullptr;
  size_t n = 0;
  explicit Guarded(size_t bytes) : n(bytes) {
    base = (uint8_t*)malloc(n + 2 * GUARD);
    if (!base) abort();
    memset(base, GUARD_BYTE, n + 2 * GUARD);
  }
  ~Guarded() { free(base); }
  Guarded(const Guarded&) = delete;
  uint8_t* data() { return base + GUARD; }
  bool intact() const {
    for (size_t i = 0; i < GUARD; ++i)
      if (base[i] != GUARD_BYTE || base[GUARD + n + i] != GUARD_BYTE) return false;
    return true;
  }
};

struct Case {
  int damage;
  hrp_jpeg_image d;
  std::vector<hrp_jpeg_segment> segs;
  std::vector<uint8_t> file, rgb;
};

// what hrp_jpeg_decode's five launches do, for one image
int decode(const hrp_jpeg_image& d, const std::vector<hrp_jpeg_segment>& segs, const uint8_t* bytes, size_t nbytes, int16_t* coef,
           size_t ncoef, uint8_t* planes, size_t nplanes, uint8_t* frame, size_t nframe) {
  jpeg::Geom g;
  if (!jpeg::jpeg_image_fits(d, g, nbytes, ncoef, nplanes, nframe)) return HRP_JPEG_ERR_DESC;
  memset(coef, 0, ncoef * sizeof(int16_t));
  uint32_t a, b;
  jpeg::jpeg_adler_part(bytes + d.scan_off, (size_t)d.sum_len, 0, (size_t)d.sum_len, a, b);
  const int sum = jpeg::jpeg_adler_finish((size_t)d.sum_len, a, b) != d.scan_sum ? HRP_JPEG_ERR_CHECKSUM : 0;
  jpeg::Tables t;
  const bool ok = jpeg::jpeg_build_tables(d, t);
  int status = sum | (ok ? 0 : HRP_JPEG_ERR_DESC);
  if (ok)
    for (const hrp_jpeg_segment& s : segs)
      status |= jpeg::jpeg_segment_fits(s, d, g) ? jpeg::jpeg_decode_segment(d, g, s, bytes, t, coef + d.coef_off) : HRP_JPEG_ERR_DESC;
  for (int j = 0; j < g.blocks; ++j) jpeg::jpeg_idct_image_block(d, g, j, coef + d.coef_off, planes + d.plane_off);
  for (int y = 0; y < d.height; ++y)
    for (int x = 0; x < d.width; ++x)
      jpeg::jpeg_pixel(d, g, planes + d.plane_off, x, y, frame + d.frame_off + ((size_t)y * d.width + x) * 3);
  return status;
}

struct Run {
  int status;
  bool guards, equal;
};

// the case with `file` (nfile bytes, possibly fewer than the original) in buffers of exactly the needed sizes
Run run(const Case& c, const uint8_t* file, size_t nfile) {
  hrp_jpeg_image d = c.d;
  std::vector<hrp_jpeg_segment> segs = c.segs;
  // a shorter file: the scan and its segments end where the file ends (what the host does when it splits what it has)
  const int64_t n = (int64_t)nfile;
  if (d.scan_off > n) d.scan_off = n;
  if (d.scan_off + d.scan_len > n) d.scan_len = n - d.scan_off;
  if (d.scan_off + d.sum_len > n) d.sum_len = n - d.scan_off;
  for (hrp_jpeg_segment& s : segs) {
    if (s.off > n) s.off = n;
    if (s.off + s.len > n) s.len = n - s.off;
  }
  jpeg::Geom g;
  if (!jpeg::jpeg_geom(d, g)) return {HRP_JPEG_ERR_DESC, true, false};
  const size_t ncoef = (size_t)g.blocks * 64, nframe = (size_t)d.width * d.height * 3;
  Guarded in(nfile), coef(ncoef * sizeof(int16_t)), planes(ncoef), frame(nframe);
  memcpy(in.data(), file, nfile);
  memset(planes.data(), 0, ncoef);
  memset(frame.data(), 0, nframe);
  Run r;
  r.status = decode(d, segs, in.data(), nfile, (int16_t*)coef.data(), ncoef, planes.data(), ncoef, frame.data(), nframe);
  r.guards = in.intact() && coef.intact() && planes.intact() && frame.intact() && memcmp(in.data(), file, nfile) == 0;
  r.equal = nframe == c.rgb.size() && memcmp(frame.data(), c.rgb.data(), nframe) == 0;
  return r;
}

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  int32_t ncases = 0;
  if (!f || !read_exact(f, &ncases, 4) || ncases < 1 || ncases > 1000) return 2;
  std::vector<Case> cases((size_t)ncases);
  for (Case& c : cases) {
    int32_t damage, nseg;
    int64_t n;
    if (!read_exact(f, &damage, 4) || !read_exact(f, &c.d, sizeof c.d) || !read_exact(f, &nseg, 4) || nseg < 0 || nseg > 100000) return 2;
    c.damage = damage;
    c.segs.resize((size_t)nseg);
    if (!read_exact(f, c.segs.data(), sizeof(hrp_jpeg_segment) * (size_t)nseg)) return 2;
    if (!read_exact(f, &n, 8) || n < 0 || n > (1 << 26)) return 2;
    c.file.resize((size_t)n);
    if (!read_exact(f, c.file.data(), (size_t)n) || !read_exact(f, &n, 8) || n < 0 || n > (1 << 26)) return 2;
    c.rgb.resize((size_t)n);
    if (!read_exact(f, c.rgb.data(), (size_t)n)) return 2;
  }
  fclose(f);

  int mismatch = 0, runs = 0, guard = 0, differ = 0, silent = 0, silent_truncated = 0, trailing_only = 0, checksum_only = 0;
  for (size_t i = 0; i < cases.size(); ++i) {
    const Run r = run(cases[i], cases[i].file.data(), cases[i].file.size());
    if (!r.equal || r.status != 0 || !r.guards) {
      printf("case %zu: equal %d status %d guards %d\n", i, (int)r.equal, r.status, (int)r.guards);
      ++mismatch;
    }
  }
  uint64_t rng = 0x9E3779B97F4A7C15ull;      // seeded: the corpus is the same on every run
  auto next = [&rng]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng >> 33);
  };
  auto account = [&](const Run& r, size_t i, const char* what, size_t at) {
    ++runs;
    if (!r.guards) {
      printf("case %zu %s %zu: guard bytes overwritten\n", i, what, at);
      ++guard;
    }
    if (!r.equal) {
      ++differ;
      if (r.status == 0) ++silent;
      if (r.status == 0 && what[0] == 't') ++silent_truncated;
      if (r.status == HRP_JPEG_ERR_CHECKSUM) ++checksum_only;
      if (r.status == (HRP_JPEG_ERR_CHECKSUM | HRP_JPEG_WARN_TRAILING)) ++trailing_only;
    }
  };
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    if (!c.damage) continue;
    for (size_t len = 0; len < c.file.size(); len += 97) account(run(c, c.file.data(), len), i, "truncated at", len);
    for (int k = 0; k < 200 && c.d.scan_len > 0; ++k) {
      std::vector<uint8_t> copy = c.file;
      const size_t at = (size_t)c.d.scan_off + next() % (size_t)c.d.scan_len;
      uint8_t v = (uint8_t)next();
      if (v == copy[at]) v ^= 0x40;
      copy[at] = v;
      account(run(c, copy.data(), copy.size()), i, "byte changed at", at);
    }
  }
  printf("valid %d mismatch %d | damaged %d guard %d differ %d silent %d silent_truncated %d trailing_only %d checksum_only %d\n", ncases,
         mismatch, runs, guard, differ, silent, silent_truncated, trailing_only, checksum_only);
  return mismatch || guard ? 1 : 0;
}
