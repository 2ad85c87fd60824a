// Host check of the kinematic smoother: csrc/kin_smooth_core.h's link_one / walk_one are the loops the kernels of csrc/kin_smooth.hip run;
// here they run on the host, one lane after another, under -fsanitize=address,undefined (tests/test_kinsmooth_host.py builds and runs
// this program).  Every buffer has its exact size, so the sanitizer sees any access past one.
//   kinsmooth_host_check run <in> <out>   every call of <in> (tests/kinsmooth_oracle.py pack_case) through hrp::kins; the outputs to <out>
//   kinsmooth_host_check self             hostile inputs; prints one line per input and "failures N"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "kin_smooth_core.h"

namespace kin = hrp::kin;
namespace kins = hrp::kins;

struct HostLanes {      // lanes 0..255 one after another; nothing to wait for
  int lo() const { return 0; }
  int hi() const { return kins::SMOOTH_LANES; }
  int lanes() const { return kins::SMOOTH_LANES; }
  void sync() const {}
};

struct Case {
  int nkp = 0, dof = 0, rot_dim = 3, free_pose = 0, root = 0, has_limits = 0, cap = 0, first = 0, L = 0, want_cov = 1, has_pose = 0;
  uint32_t free_q = 0;
  hrp_fk_chain chain;
  std::vector<double> mean, cov, dt, q_acc;
  std::vector<int32_t> valid, flags;
  std::vector<float> q_in, rot, trans, lo, hi;
};
struct Result {
  std::vector<float> q, rot, trans, vel, xyz, cov_p;
  std::vector<int32_t> status;
  std::vector<double> mean_s, cov_s;
  const char* refused = nullptr;
};

static int npar_of(const Case& c) { return kin::kin_npar(c.free_q, c.dof, c.free_pose); }

static Result smooth(const Case& c) {
  const int n = npar_of(c), N = 2 * n, L = c.L > 0 ? c.L : 0;
  Result r;
  r.q.assign((size_t)L * c.dof, -7.f); r.rot.assign((size_t)L * c.rot_dim, -7.f); r.trans.assign((size_t)L * 3, -7.f);
  r.vel.assign((size_t)L * n, -7.f); r.xyz.assign((size_t)L * c.nkp * 3, -7.f); r.status.assign((size_t)L * 2, -7);
  r.mean_s.assign((size_t)L * N, -7.0);
  if (c.want_cov) {
    r.cov_p.assign((size_t)L * n * n, -7.f);
    r.cov_s.assign((size_t)L * N * N, -7.0);
  }
  std::vector<double> gain((size_t)L * N * N, std::numeric_limits<double>::quiet_NaN());
  std::vector<int32_t> link(L, -1);
  hrp_kin_smooth_desc d;
  memset(&d, 0, sizeof d);
  d.chain = &c.chain;
  d.mean = c.mean.data(); d.cov = c.cov.data(); d.valid = c.valid.data(); d.flags = c.flags.data(); d.dt = c.dt.data();
  d.q_in = c.q_in.data();
  d.rot_fixed = c.has_pose ? c.rot.data() : nullptr; d.trans_fixed = c.has_pose ? c.trans.data() : nullptr;
  d.q_lo = c.has_limits ? c.lo.data() : nullptr; d.q_hi = c.has_limits ? c.hi.data() : nullptr;
  d.q_acc = c.q_acc.data();
  d.gain = gain.data(); d.link = link.data();
  d.free_q = c.free_q; d.free_pose = c.free_pose; d.root = c.root; d.B = 1; d.dof = c.dof; d.nkp = c.nkp; d.rot_dim = c.rot_dim;
  d.cap = c.cap; d.first = c.first; d.L = c.L; d.want_cov = c.want_cov;
  d.q = r.q.data(); d.rot = r.rot.data(); d.trans = r.trans.data(); d.vel = r.vel.data(); d.xyz = r.xyz.data();
  d.cov_p = c.want_cov ? r.cov_p.data() : nullptr; d.status = r.status.data(); d.mean_s = r.mean_s.data();
  d.cov_s = c.want_cov ? r.cov_s.data() : nullptr;
  if ((r.refused = kins::refusal(&d))) return r;
  std::vector<double> la(kins::link_doubles(N), std::numeric_limits<double>::quiet_NaN());
  std::vector<double> lb(kins::walk_doubles(n, c.nkp), std::numeric_limits<double>::quiet_NaN());
  if (la.size() * sizeof(double) > 64 * 1024 || lb.size() * sizeof(double) > 64 * 1024) {
    r.refused = "LDS";
    return r;
  }
  for (int t = 0; t < c.L; ++t) kins::link_one(HostLanes{}, d, t, 0, la.data());
  kins::walk_one(HostLanes{}, d, 0, lb.data());
  return r;
}

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return read_exact(f, v.data(), sizeof(T) * n);
}
template <class T>
static void put(FILE* g, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), g);
}

static int run(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  FILE* g = fopen(out, "wb");
  if (!f || !g) return 2;
  int32_t count = 0;
  if (!read_exact(f, &count, 4)) return 2;
  for (int i = 0; i < count; ++i) {
    int32_t h[12];
    Case c;
    if (!read_exact(f, h, sizeof h)) return 2;
    c.nkp = h[0]; c.dof = h[1]; c.rot_dim = h[2]; c.free_pose = h[3]; c.root = h[4]; c.free_q = (uint32_t)h[5]; c.has_limits = h[6];
    c.cap = h[7]; c.first = h[8]; c.L = h[9]; c.want_cov = h[10]; c.has_pose = h[11];
    if (c.nkp < 1 || c.nkp > HRP_FK_MAX_KP || c.dof < 0 || c.dof > HRP_FK_MAX_JOINTS || (c.rot_dim != 3 && c.rot_dim != 6) || c.cap < 1 ||
        c.cap > 4096)
      return 2;
    const int n = npar_of(c);
    if (n < 1 || n > HRP_KIN_FILTER_MAX_N) return 2;
    const size_t N = 2 * (size_t)n, cap = (size_t)c.cap;
    bool ok = read_exact(f, &c.chain, sizeof c.chain) && read_vec(f, c.mean, cap * N) && read_vec(f, c.cov, cap * N * N) &&
              read_vec(f, c.valid, cap) && read_vec(f, c.flags, cap) && read_vec(f, c.dt, cap) && read_vec(f, c.q_in, cap * c.dof) &&
              read_vec(f, c.rot, c.rot_dim) && read_vec(f, c.trans, 3) && read_vec(f, c.lo, c.dof) && read_vec(f, c.hi, c.dof) &&
              read_vec(f, c.q_acc, n);
    if (!ok) return 2;
    const Result r = smooth(c);
    if (r.refused) {
      fprintf(stderr, "refused: %s\n", r.refused);
      return 3;
    }
    put(g, r.q); put(g, r.rot); put(g, r.trans); put(g, r.vel); put(g, r.xyz); put(g, r.status); put(g, r.mean_s); put(g, r.cov_p); put(g, r.cov_s);
  }
  fclose(f);
  fclose(g);
  return 0;
}

// a serial chain of `nj` revolute joints with alternating axes and `nkp` key-points along it (tests/kinfilter_host_check.cpp's), and a
// history of L frames in a ring of cap slots from slot first: a slowly moving mean, a covariance with correlated (p, v) blocks
static Case synthetic(int nj, int nkp, int free_pose, int L, int cap, int first) {
  Case c;
  memset(&c.chain, 0, sizeof c.chain);
  c.nkp = nkp; c.dof = nj; c.free_pose = free_pose; c.cap = cap; c.first = first; c.L = L; c.has_limits = 1; c.has_pose = !free_pose;
  c.chain.njoints = nj; c.chain.dof = nj; c.chain.nkp = nkp;
  for (int j = 0; j < nj; ++j) {
    c.chain.parent[j] = j - 1; c.chain.type[j] = 1; c.chain.cfg[j] = j; c.chain.mimic_mul[j] = 1.f;
    float* o = c.chain.origin[j];
    o[0] = o[5] = o[10] = 1.f;
    o[3] = 0.03f * (float)((j * 7) % 5 - 2); o[7] = 0.02f * (float)((j * 3) % 7 - 3); o[11] = 0.05f;
    c.chain.axis[j][j % 3 == 0 ? 2 : (j % 3 == 1 ? 1 : 0)] = 1.f;
  }
  for (int k = 0; k < nkp; ++k) {
    c.chain.kp_frame[k] = nj ? (k * nj) / nkp : -1;
    c.chain.kp_offset[k][0] = 0.05f * (float)(k % 3 - 1); c.chain.kp_offset[k][1] = 0.04f * (float)(k % 4 - 2); c.chain.kp_offset[k][2] = 0.03f * (float)(k % 5);
  }
  c.free_q = nj >= 32 ? 0xffffffffu : ((1u << nj) - 1u);
  c.rot = {0.3f, -0.2f, 0.1f};
  c.trans = {0.05f, -0.1f, 1.5f};
  c.lo.assign(nj, -3.f); c.hi.assign(nj, 3.f);
  const int n = npar_of(c);
  if (n < 1 || n > HRP_KIN_FILTER_MAX_N || cap < 1) return c;
  const int N = 2 * n;
  c.q_acc.assign(n, 4.0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  c.mean.assign((size_t)cap * N, nan); c.cov.assign((size_t)cap * N * N, nan); c.dt.assign(cap, nan);
  c.valid.assign(cap, 7); c.flags.assign(cap, -1);
  c.q_in.assign((size_t)cap * nj, 0.1f);
  for (int t = 0; t < L && t < cap; ++t) {
    const size_t s = (size_t)((first + t) % cap);
    c.valid[s] = 1; c.flags[s] = t == 0 ? (HRP_KF_INIT | HRP_KF_CONVERGED) : HRP_KF_CONVERGED; c.dt[s] = 1.0 / 30;
    for (int i = 0; i < n; ++i) {
      c.mean[s * N + i] = 0.1 + 0.01 * t + 0.02 * i;
      c.mean[s * N + n + i] = 0.3 - 0.01 * i;
    }
    double* P = &c.cov[s * N * N];
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        const int a = i % n, b = j % n;
        double v = a == b ? (i < n && j < n ? 0.01 : (i >= n && j >= n ? 0.5 : 0.02)) : 0.0;
        if (a != b && (i < n) == (j < n)) v = (i < n ? 0.001 : 0.02) / (1.0 + (a > b ? a - b : b - a));
        P[i * N + j] = v;
      }
  }
  return c;
}

static int failures = 0;
static Result report(const char* name, const Case& c) {
  const Result r = smooth(c);
  if (r.refused) {
    printf("hostile %s: refused 1 (%s)\n", name, r.refused);
    return r;
  }
  const int n = npar_of(c), N = 2 * n;
  bool fin = true, sym = true, untouched = false;
  for (float v : r.q) fin = fin && kin::finite64(v), untouched = untouched || v == -7.f;
  for (float v : r.rot) fin = fin && kin::finite64(v), untouched = untouched || v == -7.f;
  for (float v : r.trans) fin = fin && kin::finite64(v), untouched = untouched || v == -7.f;
  for (float v : r.vel) fin = fin && kin::finite64(v), untouched = untouched || v == -7.f;
  for (float v : r.xyz) fin = fin && kin::finite64(v), untouched = untouched || v == -7.f;
  for (float v : r.cov_p) fin = fin && kin::finite64(v), untouched = untouched || v == -7.f;
  for (double v : r.mean_s) untouched = untouched || v == -7.0;
  for (double v : r.cov_s) untouched = untouched || v == -7.0;
  for (int32_t v : r.status) untouched = untouched || v == -7;
  if (c.want_cov)
    for (int t = 0; t < c.L; ++t)
      for (int i = 0; i < N; ++i)
        for (int j = 0; j < i; ++j)
          sym = sym && memcmp(&r.cov_s[((size_t)t * N + i) * N + j], &r.cov_s[((size_t)t * N + j) * N + i], 8) == 0;
  std::string fl;
  for (int t = 0; t < c.L; ++t) fl += (t ? "," : "") + std::to_string(r.status[2 * t]) + "/" + std::to_string(r.status[2 * t + 1]);
  if (untouched) ++failures;
  printf("hostile %s: refused 0 status %s finite32 %d symmetric %d written %d\n", name, fl.c_str(), (int)fin, (int)sym, (int)!untouched);
  return r;
}

static int self() {
  const double dnan = std::numeric_limits<double>::quiet_NaN();
  const int N = 12;
  auto slot = [](const Case& c, int t) { return (size_t)((c.first + t) % c.cap); };
  report("plain", synthetic(6, 7, 0, 6, 6, 0));
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.mean[slot(c, 3) * N + 2] = dnan; report("NaN mean", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); for (int j = 0; j < N; ++j) c.cov[(slot(c, 3) * N + 4) * N + j] = dnan; report("NaN row in cov", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.cov[(slot(c, 3) * N + 4) * N + 1] = dnan; report("NaN off the diagonal of cov", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0);
    for (int j = 0; j < N; ++j) c.cov[(slot(c, 3) * N + 4) * N + j] = c.cov[(slot(c, 3) * N + j) * N + 4] = 0.0;
    report("zero row in cov", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); std::fill(c.cov.begin() + slot(c, 2) * N * N, c.cov.begin() + (slot(c, 2) + 1) * N * N, 0.0);
    c.q_acc.assign(6, 0.0); report("zero pivot in P-", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.dt[slot(c, 3)] = 4.9e-324; report("dt denormal", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.dt[slot(c, 3)] = 1e300; report("dt 1e300", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.dt[slot(c, 3)] = dnan; report("dt NaN", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.valid.assign(6, 0); report("every frame invalid", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); for (int t = 0; t < 6; ++t) c.mean[slot(c, t) * N] = 5.0; report("beyond a bound", c); }
  report("L 1", synthetic(6, 7, 0, 1, 1, 0));
  report("first = cap - 1", synthetic(6, 7, 1, 5, 8, 7));
  report("n 1", synthetic(1, 3, 0, 4, 4, 0));
  report("n 20 nkp 24", synthetic(14, 24, 1, 4, 4, 0));
  { Case c = synthetic(14, 24, 1, 4, 4, 0); c.rot_dim = 6; c.root = 23; c.want_cov = 0; report("n 20 rot_dim 6 root 23 no cov", c); }
  { Case c = synthetic(0, 5, 1, 3, 3, 0); report("dof 0", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.chain.parent[3] = 5; c.chain.kp_frame[2] = 40; c.chain.cfg[1] = 77; report("broken chain table", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.L = 0; report("L 0", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.L = 7; report("L > cap", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.first = 6; report("first = cap", c); }
  { Case c = synthetic(15, 7, 1, 2, 2, 0); report("n 21", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.free_q = 0; report("n 0", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.rot_dim = 4; report("rot_dim 4", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.nkp = 25; report("nkp 25", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.free_q = 1u << 6; report("free_q beyond dof", c); }
  { Case c = synthetic(6, 7, 0, 6, 6, 0); c.has_pose = 0; report("no fixed pose", c); }
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "self")) return self();
  fprintf(stderr, "usage: kinsmooth_host_check run <in> <out> | self\n");
  return 2;
}
