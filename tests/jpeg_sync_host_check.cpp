// Stand-alone host check of the many-lanes-per-segment entropy stage of csrc/jpeg_core.h (jpeg_sync_subseq and the helpers
// around it; built and run by tests/test_jpeg_sync_host.py, also the program to build with -fsanitize=address,undefined).
// It runs the schedule of jpeg_sync_kernel lane by lane - step (a) from guessed states, rounds that read the previous round's
// exit states, the exclusive prefix sum, the final pass - with every segment of every case taken as a long one, and compares
// with jpeg_decode_segment on the same bytes:
//   1. every case at S = 16, 64, 4096: coefficients equal, status 0, the frame equal to the recorded one;
//   2. every case at S = 16 with three guessed start states and the lanes of every pass in ascending and in descending order:
//      coefficients and status equal to the serial decoder's in every run;
//   3. the damaged corpus of jpeg_host_check.cpp (same seed, same recipe) at S = 16 and 128, and every flagged case with
//      0 .. 9 bytes and an EOI marker appended INSIDE its last segment (the one place where the serial decoder's status
//      depends on how far ahead its reader had loaded): coefficients, status and frame equal, guard bytes intact.
// Input: the format of jpeg_host_check.cpp.  Output: one line "case <i> subseq <n> rounds <n> wrong <n>" per case (S = 16, guess
// (0, 0): sub-sequences, rounds of step (b), lanes whose first exit state was not the final one), one line per failure, and
//   "valid <runs> mismatch <n> | order <runs> differ <n> | damaged <runs> guard <n> differ <n> serial <n> | looped <cases>"
// serial: runs that took jpeg_segment_status; looped: cases with a wrong first exit and two or more rounds.
// Exit status 1 for a difference or a guard violation, 2 for a bad input file.
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

struct Sched {
  int64_t S;
  int guess_unit, guess_k;
  bool descending;
};
struct Stats {
  uint32_t subseqs = 0, rounds = 0, wrong = 0, serial = 0;
};

// one segment the way one workgroup of jpeg_sync_kernel decodes it; `region` is its SyncHead and slots
int sync_segment(const hrp_jpeg_image& d, const jpeg::Geom& g, const hrp_jpeg_segment& s, const uint8_t* bytes, const jpeg::Tables& t,
                 int16_t* coef, const Sched& sc, jpeg::SyncSlot* region, Stats& st) {
  if (s.len == 0) return jpeg::jpeg_decode_segment(d, g, s, bytes, t, coef);
  const int64_t n = (s.len + sc.S - 1) / sc.S;
  jpeg::SyncHead& head = *(jpeg::SyncHead*)region;
  jpeg::SyncSlot* sl = region + 1;
  auto lanes = [&](auto fn) {
    if (sc.descending)
      for (int64_t i = n - 1; i >= 0; --i) fn(i);
    else
      for (int64_t i = 0; i < n; ++i) fn(i);
  };
  lanes([&](int64_t i) { jpeg::jpeg_sync_first(d, g, s, bytes, t, i, n, sc.S, sc.guess_unit, sc.guess_k, sl[i]); });
  std::vector<jpeg::SyncState> first((size_t)n);
  for (int64_t i = 0; i < n; ++i) first[(size_t)i] = sl[i].exit;
  uint32_t rounds = 0;
  for (bool changed = true; changed;) {
    ++rounds;
    changed = false;
    lanes([&](int64_t i) {
      if (i && sl[i - 1].exit != sl[i].entry) {
        sl[i].entry = sl[i - 1].exit;
        sl[i].redo = 1;
      }
    });
    lanes([&](int64_t i) {
      if (!sl[i].redo) return;
      sl[i].redo = 0;
      jpeg::jpeg_sync_subseq(d, g, s, bytes, t, jpeg::sync_hi(i, n, sc.S), sl[i].entry, sl[i].exit, sl[i].sums, false, 0, nullptr, nullptr);
      changed = true;
    });
  }
  head.rounds = rounds;
  head.subseqs = (uint32_t)n;
  head.wrong = 0;
  for (int64_t i = 0; i < n; ++i) head.wrong += first[(size_t)i] != sl[i].exit;
  jpeg::SyncSums run = {0, {0, 0, 0}, 0};
  for (int64_t i = 0; i < n; ++i) {
    const jpeg::SyncSums own = sl[i].sums;
    sl[i].sums = run;
    run.blocks += own.blocks;
    for (int c = 0; c < 3; ++c) run.dc[c] = (uint16_t)(run.dc[c] + own.dc[c]);
    run.hit = (uint16_t)(run.hit || own.hit);
  }
  Guarded block(64 * sizeof(int16_t));
  int err = 0;
  lanes([&](int64_t i) { err |= jpeg::jpeg_sync_final(d, g, s, bytes, t, i, n, sc.S, sl[i], coef, (int16_t*)block.data()); });
  if (!block.intact()) abort();
  st.subseqs += head.subseqs;
  st.wrong += head.wrong;
  st.rounds = st.rounds > head.rounds ? st.rounds : head.rounds;
  st.serial += (err & jpeg::SYNC_SERIAL) != 0;
  return err & ~jpeg::SYNC_SERIAL;
}

// what the launches of hrp_jpeg_decode (sc == nullptr) or hrp_jpeg_decode_sync do, for one image
int decode(const hrp_jpeg_image& d, const std::vector<hrp_jpeg_segment>& segs, const uint8_t* bytes, size_t nbytes, int16_t* coef,
           size_t ncoef, uint8_t* planes, size_t nplanes, uint8_t* frame, size_t nframe, const Sched* sc, uint8_t* scratch, size_t nscratch,
           Stats& st) {
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
    for (size_t j = 0; j < segs.size(); ++j) {
      const hrp_jpeg_segment& s = segs[j];
      if (!jpeg::jpeg_segment_fits(s, d, g)) {
        status |= HRP_JPEG_ERR_DESC;
      } else if (!sc) {
        status |= jpeg::jpeg_decode_segment(d, g, s, bytes, t, coef + d.coef_off);
      } else {
        const uint64_t base = jpeg::sync_region((uint64_t)s.off, j, (uint64_t)sc->S), n = ((uint64_t)s.len + sc->S - 1) / sc->S;
        if ((base + 1 + n) * sizeof(jpeg::SyncSlot) > nscratch) status |= HRP_JPEG_ERR_DESC;
        else status |= sync_segment(d, g, s, bytes, t, coef + d.coef_off, *sc, (jpeg::SyncSlot*)scratch + base, st);
      }
    }
  for (int j = 0; j < g.blocks; ++j) jpeg::jpeg_idct_image_block(d, g, j, coef + d.coef_off, planes + d.plane_off);
  for (int y = 0; y < d.height; ++y)
    for (int x = 0; x < d.width; ++x)
      jpeg::jpeg_pixel(d, g, planes + d.plane_off, x, y, frame + d.frame_off + ((size_t)y * d.width + x) * 3);
  return status;
}

struct Run {
  int status;          // of the sync decode
  bool guards;
  bool same;           // coefficients, status and frame equal to the serial decoder's on the same bytes
  bool golden;         // the frame equals the recorded one
  Stats st;
};

// the case with `file` (nfile bytes) in buffers of exactly the needed sizes; grow: bytes at the end of the file that belong to the
// last segment as well
Run run(const Case& c, const uint8_t* file, size_t nfile, const Sched& sc, int64_t grow = 0) {
  hrp_jpeg_image d = c.d;
  std::vector<hrp_jpeg_segment> segs = c.segs;
  const int64_t n = (int64_t)nfile;
  if (grow) {
    d.scan_len += grow;
    d.sum_len = d.scan_len;
    segs.back().len += grow;
  }
  if (d.scan_off > n) d.scan_off = n;
  if (d.scan_off + d.scan_len > n) d.scan_len = n - d.scan_off;
  if (d.scan_off + d.sum_len > n) d.sum_len = n - d.scan_off;
  for (hrp_jpeg_segment& s : segs) {
    if (s.off > n) s.off = n;
    if (s.off + s.len > n) s.len = n - s.off;
  }
  Run r = {HRP_JPEG_ERR_DESC, true, false, false, {}};
  jpeg::Geom g;
  if (!jpeg::jpeg_geom(d, g)) return r;
  const size_t ncoef = (size_t)g.blocks * 64, nframe = (size_t)d.width * d.height * 3;
  const size_t nscratch = (size_t)jpeg::sync_slots(nfile, segs.size(), (uint64_t)sc.S) * sizeof(jpeg::SyncSlot);
  Guarded in(nfile), coef(ncoef * sizeof(int16_t)), planes(ncoef), frame(nframe), scratch(nscratch);
  Guarded coef0(ncoef * sizeof(int16_t)), planes0(ncoef), frame0(nframe);
  memcpy(in.data(), file, nfile);
  for (Guarded* p : {&planes, &frame, &planes0, &frame0}) memset(p->data(), 0, p->n);
  memset(scratch.data(), 0x5A, nscratch);      // whatever an earlier call left there
  Stats none;
  const int want = decode(d, segs, in.data(), nfile, (int16_t*)coef0.data(), ncoef, planes0.data(), ncoef, frame0.data(), nframe, nullptr,
                          nullptr, 0, none);
  r.status = decode(d, segs, in.data(), nfile, (int16_t*)coef.data(), ncoef, planes.data(), ncoef, frame.data(), nframe, &sc, scratch.data(),
                    nscratch, r.st);
  r.guards = in.intact() && coef.intact() && planes.intact() && frame.intact() && scratch.intact() && memcmp(in.data(), file, nfile) == 0;
  r.same = r.status == want && memcmp(coef.data(), coef0.data(), coef.n) == 0 && memcmp(frame.data(), frame0.data(), nframe) == 0;
  r.golden = nframe == c.rgb.size() && memcmp(frame.data(), c.rgb.data(), nframe) == 0;
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
    if (!read_exact(f, &damage, 4) || !read_exact(f, &c.d, sizeof c.d) || !read_exact(f, &nseg, 4) || nseg < 1 || nseg > 100000) return 2;
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

  int valid = 0, mismatch = 0, order = 0, order_differ = 0, runs = 0, guard = 0, differ = 0, serial = 0, looped = 0;
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    for (int64_t S : {16, 64, 4096}) {
      const Run r = run(c, c.file.data(), c.file.size(), {S, 0, 0, false});
      ++valid;
      if (!r.same || !r.golden || r.status != 0 || !r.guards) {
        printf("case %zu S %d: same %d golden %d status %d guards %d\n", i, (int)S, (int)r.same, (int)r.golden, r.status, (int)r.guards);
        ++mismatch;
      }
      if (S == 16) {
        printf("case %zu subseq %u rounds %u wrong %u\n", i, r.st.subseqs, r.st.rounds, r.st.wrong);
        looped += r.st.wrong > 0 && r.st.rounds >= 2;
      }
    }
    const int last_unit = c.d.hsamp * c.d.vsamp + 1;
    for (int gi = 0; gi < 3; ++gi)
      for (int desc = 0; desc < 2; ++desc) {
        const Sched sc = {16, gi == 0 ? 0 : (gi == 1 ? last_unit : 1), gi == 0 ? 0 : (gi == 1 ? 63 : 1), desc != 0};
        const Run r = run(c, c.file.data(), c.file.size(), sc);
        ++order;
        if (!r.same || !r.golden || r.status != 0 || !r.guards) {
          printf("case %zu guess (%d, %d) descending %d: same %d golden %d status %d guards %d\n", i, sc.guess_unit, sc.guess_k, desc,
                 (int)r.same, (int)r.golden, r.status, (int)r.guards);
          ++order_differ;
        }
      }
  }
  uint64_t rng = 0x9E3779B97F4A7C15ull;      // seeded: the corpus of jpeg_host_check.cpp
  auto next = [&rng]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng >> 33);
  };
  auto account = [&](const Run& r, size_t i, int64_t S, const char* what, size_t at) {
    ++runs;
    serial += (int)r.st.serial;
    if (!r.guards) {
      printf("case %zu S %d %s %zu: guard bytes overwritten\n", i, (int)S, what, at);
      ++guard;
    }
    if (!r.same) {
      printf("case %zu S %d %s %zu: differs from the serial decoder (status %d)\n", i, (int)S, what, at, r.status);
      ++differ;
    }
  };
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    if (!c.damage) continue;
    for (size_t len = 0; len < c.file.size(); len += 97)
      for (int64_t S : {16, 128}) account(run(c, c.file.data(), len, {S, 0, 0, false}), i, S, "truncated at", len);
    for (int k = 0; k < 200 && c.d.scan_len > 0; ++k) {
      std::vector<uint8_t> copy = c.file;
      const size_t at = (size_t)c.d.scan_off + next() % (size_t)c.d.scan_len;
      uint8_t v = (uint8_t)next();
      if (v == copy[at]) v ^= 0x40;
      copy[at] = v;
      for (int64_t S : {16, 128}) account(run(c, copy.data(), copy.size(), {S, 0, 0, false}), i, S, "byte changed at", at);
    }
    // the scan up to its EOI, 0 .. 9 more bytes and an EOI, all of it inside the last segment
    const size_t end = (size_t)(c.segs.back().off + c.segs.back().len);
    for (size_t k = 0; k < 10; ++k) {
      std::vector<uint8_t> copy(c.file.begin(), c.file.begin() + (long)end);
      for (size_t j = 0; j < k; ++j) copy.push_back((uint8_t)(0x11 * (j + 1)));
      copy.push_back(0xFF);
      copy.push_back(0xD9);
      for (int64_t S : {16, 128}) account(run(c, copy.data(), copy.size(), {S, 0, 0, false}, (int64_t)k + 2), i, S, "marker behind", k);
    }
  }
  printf("valid %d mismatch %d | order %d differ %d | damaged %d guard %d differ %d serial %d | looped %d\n", valid, mismatch, order,
         order_differ, runs, guard, differ, serial, looped);
  return mismatch || order_differ || guard || differ ? 1 : 0;
}
