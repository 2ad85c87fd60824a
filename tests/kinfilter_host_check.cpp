// Host check of the kinematic filter: csrc/kin_filter_core.h's step_one is the loop the kernel of csrc/kin_filter.hip runs; here it runs
// on the host, one lane after another, under -fsanitize=address,undefined (tests/test_kinfilter_host.py builds and runs this program).
//   kinfilter_host_check run <in> <out>   every step of <in> (tests/kinfilter_oracle.py pack_step) through hrp::kinf::step_one; the state
//                                         after it and the outputs to <out>.  A step marked `chained` starts from the state the step
//                                         before it left, not from the one in the file
//   kinfilter_host_check self             hostile inputs; prints one line per input and "failures N"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "kin_filter_core.h"

namespace kin = hrp::kin;
namespace kinf = hrp::kinf;

struct HostLanes {      // lanes 0..63 one after another; nothing to wait for
  int lo() const { return 0; }
  int hi() const { return kin::KIN_LANES; }
  void sync() const {}
};

struct Step {
  int nkp = 0, dof = 0, rot_dim = 3, free_pose = 0, root = 0, present = 0, max_coast = 5, keep = 1;
  uint32_t free_q = 0;
  double dt = 1.0 / 30, gate = 0.0;
  hrp_fk_chain chain;
  std::vector<float> pts2d, w2d, K, q_in, rot_in, trans_in, lo, hi, w_q, q_meas;
  std::vector<double> q_acc, p0_var, mean, cov;
  int32_t valid = 0, coast = 0;
};
struct Result {
  std::vector<double> mean, cov;
  int32_t valid = 0, coast = 0, status[4] = {0, 0, 0, 0};
  std::vector<float> q, rot, trans, xyz, uv, vel, cov_p, xyz_next, d2;
  const char* refused = nullptr;
};

static int npar_of(const Step& s) { return kin::kin_npar(s.free_q, s.dof, s.free_pose); }

static Result step(const Step& s) {
  const int n = npar_of(s);
  Result r;
  // exact sizes, so that the sanitizer sees any access past a buffer
  r.mean = s.mean; r.cov = s.cov; r.valid = s.valid; r.coast = s.coast;
  r.q.assign(s.dof, -7.f); r.rot.assign(s.rot_dim, -7.f); r.trans.assign(3, -7.f);
  r.xyz.assign(3 * s.nkp, -7.f); r.uv.assign(2 * s.nkp, -7.f); r.vel.assign(n, -7.f); r.cov_p.assign((size_t)n * n, -7.f);
  r.xyz_next.assign(3 * s.nkp, -7.f); r.d2.assign(s.nkp, -7.f);
  hrp_kin_filter_desc d;
  memset(&d, 0, sizeof d);
  d.chain = &s.chain;
  d.pts2d = s.pts2d.data();
  d.w2d = (s.present & 1) ? s.w2d.data() : nullptr;
  d.K = s.K.data(); d.K_stride = 9; d.nkp = s.nkp;
  d.q_in = s.q_in.data(); d.rot_in = s.rot_in.data(); d.trans_in = s.trans_in.data();
  d.rot_dim = s.rot_dim; d.pose_stride = 1;
  d.q_lo = (s.present & 2) ? s.lo.data() : nullptr;
  d.q_hi = (s.present & 2) ? s.hi.data() : nullptr;
  d.w_q = (s.present & 4) ? s.w_q.data() : nullptr;
  d.q_meas = (s.present & 4) ? s.q_meas.data() : nullptr;
  d.keep = (s.present & 8) ? &s.keep : nullptr;
  d.q_acc = s.q_acc.data(); d.p0_var = s.p0_var.data();
  d.free_q = s.free_q; d.free_pose = s.free_pose; d.root = s.root; d.B = 1; d.dof = s.dof; d.max_coast = s.max_coast;
  d.dt = s.dt; d.gate_chi2 = s.gate;
  d.mean = r.mean.data(); d.cov = r.cov.data(); d.valid = &r.valid; d.coast = &r.coast;
  d.q = r.q.data(); d.rot = r.rot.data(); d.trans = r.trans.data(); d.xyz = r.xyz.data(); d.uv = r.uv.data();
  d.vel = r.vel.data(); d.cov_p = r.cov_p.data(); d.xyz_next = r.xyz_next.data(); d.d2 = r.d2.data(); d.status = r.status;
  if ((r.refused = kinf::refusal(&d))) return r;
  std::vector<double> lds(kinf::shared_doubles(n, s.nkp, s.dof), std::numeric_limits<double>::quiet_NaN());
  if (lds.size() * sizeof(double) > 64 * 1024) {
    r.refused = "LDS";
    return r;
  }
  kinf::step_one(HostLanes{}, kinf::stream_of(d, 0), lds.data());
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
  Result prev;
  for (int i = 0; i < count; ++i) {
    int32_t h[12];
    Step s;
    if (!read_exact(f, h, sizeof h)) return 2;
    s.nkp = h[0]; s.dof = h[1]; s.rot_dim = h[2]; s.free_pose = h[3]; s.root = h[4]; s.free_q = (uint32_t)h[5]; s.present = h[6];
    s.max_coast = h[7]; s.valid = h[8]; s.coast = h[9]; s.keep = h[10];
    if (s.nkp < 1 || s.nkp > HRP_FK_MAX_KP || s.dof < 0 || s.dof > HRP_FK_MAX_JOINTS || (s.rot_dim != 3 && s.rot_dim != 6)) return 2;
    const int n = npar_of(s);
    if (n < 1 || n > HRP_KIN_FILTER_MAX_N) return 2;
    double sc[2];
    bool ok = read_exact(f, sc, sizeof sc) && read_exact(f, &s.chain, sizeof s.chain) && read_vec(f, s.pts2d, 2 * s.nkp) &&
              read_vec(f, s.w2d, s.nkp) && read_vec(f, s.K, 9) && read_vec(f, s.q_in, s.dof) && read_vec(f, s.rot_in, s.rot_dim) &&
              read_vec(f, s.trans_in, 3) && read_vec(f, s.lo, s.dof) && read_vec(f, s.hi, s.dof) && read_vec(f, s.w_q, s.dof) &&
              read_vec(f, s.q_meas, s.dof) && read_vec(f, s.q_acc, n) && read_vec(f, s.p0_var, 2 * n) && read_vec(f, s.mean, 2 * n) &&
              read_vec(f, s.cov, (size_t)4 * n * n);
    if (!ok) return 2;
    s.dt = sc[0]; s.gate = sc[1];
    if (h[11] && i > 0 && prev.mean.size() == s.mean.size()) {      // a free run: the state the previous step left
      s.mean = prev.mean; s.cov = prev.cov; s.valid = prev.valid; s.coast = prev.coast;
    }
    const Result r = step(s);
    prev = r;
    if (r.refused) {
      fprintf(stderr, "refused: %s\n", r.refused);
      return 3;
    }
    put(g, r.mean); put(g, r.cov);
    fwrite(&r.valid, 4, 1, g); fwrite(&r.coast, 4, 1, g); fwrite(r.status, 4, 4, g);
    put(g, r.q); put(g, r.rot); put(g, r.trans); put(g, r.xyz); put(g, r.uv); put(g, r.vel); put(g, r.cov_p); put(g, r.xyz_next); put(g, r.d2);
  }
  fclose(f);
  fclose(g);
  return 0;
}

// a serial chain of `nj` revolute joints with alternating axes and `nkp` key-points spread along it, about 1.5 m in front of the camera;
// the points are the projections at q = 0.1 moved by one pixel, the state is a filter one frame old
static Step synthetic(int nj, int nkp, int free_pose) {
  Step s;
  memset(&s.chain, 0, sizeof s.chain);
  s.nkp = nkp; s.dof = nj;
  s.chain.njoints = nj; s.chain.dof = nj; s.chain.nkp = nkp;
  for (int j = 0; j < nj; ++j) {
    s.chain.parent[j] = j - 1; s.chain.type[j] = 1; s.chain.cfg[j] = j; s.chain.mimic_mul[j] = 1.f;
    float* o = s.chain.origin[j];
    o[0] = o[5] = o[10] = 1.f;
    o[3] = 0.03f * (float)((j * 7) % 5 - 2); o[7] = 0.02f * (float)((j * 3) % 7 - 3); o[11] = 0.05f;
    s.chain.axis[j][j % 3 == 0 ? 2 : (j % 3 == 1 ? 1 : 0)] = 1.f;
  }
  for (int k = 0; k < nkp; ++k) {
    s.chain.kp_frame[k] = nj ? (k * nj) / nkp : -1;
    s.chain.kp_offset[k][0] = 0.05f * (float)(k % 3 - 1); s.chain.kp_offset[k][1] = 0.04f * (float)(k % 4 - 2); s.chain.kp_offset[k][2] = 0.03f * (float)(k % 5);
  }
  s.K = {600.f, 0.f, 320.f, 0.f, 600.f, 240.f, 0.f, 0.f, 1.f};
  s.q_in.assign(nj, 0.1f);
  s.rot_in = {0.3f, -0.2f, 0.1f};
  s.trans_in = {0.05f, -0.1f, 1.5f};
  s.w2d.assign(nkp, 1.f);
  s.lo.assign(nj, -3.f); s.hi.assign(nj, 3.f); s.w_q.assign(nj, 1.f); s.q_meas.assign(nj, 0.1f);
  s.free_q = nj >= 32 ? 0xffffffffu : ((1u << nj) - 1u);
  s.free_pose = free_pose;
  s.present = 1 | 2 | 4 | 8;
  const int n = npar_of(s);
  s.q_acc.assign(n, 4.0);
  s.p0_var.assign(2 * n, 0.04);
  s.mean.assign(2 * n, 0.0);
  s.cov.assign((size_t)4 * n * n, 0.0);
  s.pts2d.assign(2 * nkp, 300.f);
  if (n < 1 || n > HRP_KIN_FILTER_MAX_N) return s;
  // the first frame: start at the inputs, no point used, so the state becomes (inputs, 0, diag p0_var) and the key-points are reported
  Step first = s;
  first.w2d.assign(nkp, 0.f);
  const Result r = step(first);
  s.mean = r.mean; s.cov = r.cov; s.valid = r.valid; s.coast = 0;
  for (int k = 0; k < nkp; ++k) {
    s.pts2d[2 * k] = r.uv[2 * k] + 1.f;
    s.pts2d[2 * k + 1] = r.uv[2 * k + 1] - 1.f;
  }
  return s;
}

static int failures = 0;
static bool all_finite(const std::vector<double>& v) {
  for (double x : v)
    if (!kin::finite64(x)) return false;
  return true;
}
static Result report(const char* name, const Step& s) {
  const Result r = step(s);
  if (r.refused) {
    printf("hostile %s: refused 1 (%s)\n", name, r.refused);
    return r;
  }
  bool in = (s.dof == 0 || memcmp(r.q.data(), s.q_in.data(), 4 * s.dof) == 0) && memcmp(r.rot.data(), s.rot_in.data(), 4 * s.rot_dim) == 0 &&
            memcmp(r.trans.data(), s.trans_in.data(), 12) == 0;
  bool same = r.mean.size() == s.mean.size() && memcmp(r.mean.data(), s.mean.data(), 8 * r.mean.size()) == 0 &&
              memcmp(r.cov.data(), s.cov.data(), 8 * r.cov.size()) == 0;
  bool sym = true;
  const size_t n2 = r.mean.size();
  for (size_t i = 0; i < n2; ++i)
    for (size_t j = 0; j < i; ++j) sym = sym && memcmp(&r.cov[i * n2 + j], &r.cov[j * n2 + i], 8) == 0;
  printf("hostile %s: refused 0 flags %d trials %d used %d gated %d valid %d coast %d inputs %d state_kept %d finite %d symmetric %d\n", name,
         r.status[0], r.status[1], r.status[2], r.status[3], r.valid, r.coast, (int)in, (int)same, (int)(all_finite(r.mean) && all_finite(r.cov)),
         (int)sym);
  return r;
}

static int self() {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const double dnan = std::numeric_limits<double>::quiet_NaN();
  report("plain", synthetic(7, 7, 0));
  {
    Step s = synthetic(7, 7, 0);
    s.pts2d.assign(14, nan);
    report("NaN points", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    for (auto* v : {&s.pts2d, &s.w2d, &s.K, &s.q_in, &s.rot_in, &s.trans_in, &s.lo, &s.hi, &s.w_q, &s.q_meas}) v->assign(v->size(), nan);
    s.mean.assign(s.mean.size(), dnan); s.cov.assign(s.cov.size(), dnan);
    s.q_acc.assign(s.q_acc.size(), dnan); s.p0_var.assign(s.p0_var.size(), dnan);
    report("NaN everywhere", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    s.mean.assign(s.mean.size(), dnan);
    report("NaN state, good inputs", s);
  }
  {
    Step s = synthetic(7, 7, 0);      // a zero row and column of cov: with q_acc > 0 the prediction is still positive definite
    const int n2 = 14;
    for (int j = 0; j < n2; ++j) s.cov[2 * n2 + j] = s.cov[j * n2 + 2] = 0.0;
    report("zero row and column in cov", s);
  }
  {
    Step s = synthetic(7, 7, 0);      // and with q_acc = 0 as well: A has a zero pivot, the stream starts again
    const int n2 = 14;
    for (int j = 0; j < n2; ++j) s.cov[2 * n2 + j] = s.cov[j * n2 + 2] = s.cov[9 * n2 + j] = s.cov[j * n2 + 9] = 0.0;
    s.q_acc.assign(7, 0.0);
    report("zero pivot in the prediction", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    s.cov.assign(s.cov.size(), 0.0); s.p0_var.assign(14, 0.0); s.q_acc.assign(7, 0.0);
    report("zero cov and zero p0_var", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    for (int k = 0; k < 7; ++k) s.pts2d[2 * k] += 500.f;
    s.gate = 30.0;
    report("all points gated", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    for (int k = 0; k < 7; ++k) s.pts2d[2 * k] += 500.f;
    s.gate = 30.0; s.coast = 5; s.max_coast = 5;
    report("all points gated, coast at max_coast", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    s.w2d.assign(7, 0.f); s.coast = 0x7fffffff; s.max_coast = 0x7fffffff;
    report("coast at INT_MAX", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    s.trans_in[2] = -1.5f; s.valid = 0;
    report("start behind the camera", s);
  }
  {
    Step s = synthetic(7, 7, 0);
    s.lo.assign(7, 1.f); s.hi.assign(7, -1.f);
    report("lo > hi", s);
  }
  for (double dt : {0.0, -1.0, (double)std::numeric_limits<float>::infinity(), dnan}) {
    Step s = synthetic(7, 7, 0);
    s.dt = dt;
    const Result r = report("dt refused", s);
    if (!r.refused) ++failures;
  }
  {
    Step s = synthetic(7, 7, 0);
    s.dt = 4.9406564584124654e-324;      // the smallest positive double passes the refusal: P- = P, a plain update
    const Result r = report("dt denormal", s);
    if (r.refused) ++failures;
  }
  {
    Step s = synthetic(7, 7, 0);
    s.dt = 1e300;
    const Result r = report("dt huge", s);
    if (r.refused) ++failures;
  }
  {
    Step s = synthetic(7, 7, 0);
    s.max_coast = -1;
    if (!report("max_coast -1", s).refused) ++failures;
  }
  {
    Step s = synthetic(1, 3, 0);      // n = 1
    const Result r = report("n 1", s);
    if (r.refused || r.mean.size() != 2) ++failures;
  }
  {
    Step s = synthetic(14, 24, 1);      // n = 20, the largest, with 24 key-points: every buffer at its limit
    const Result r = report("n 20 nkp 24", s);
    if (r.refused || r.mean.size() != 40) ++failures;
  }
  {
    Step s = synthetic(14, 24, 1);
    s.rot_dim = 6; s.rot_in = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f}; s.root = 23; s.valid = 0;
    report("n 20 rot_dim 6 root 23 start", s);
  }
  {
    Step s = synthetic(15, 24, 1);      // n = 21
    if (!report("n 21", s).refused) ++failures;
  }
  {
    Step s = synthetic(3, 5, 0);
    s.free_q = 0;      // n = 0
    if (!report("n 0", s).refused) ++failures;
  }
  {
    Step s = synthetic(0, 5, 1);      // no joints at all: the pose alone is filtered
    const Result r = report("dof 0", s);
    if (r.refused || r.mean.size() != 12) ++failures;
  }
  {
    Step s = synthetic(0, 5, 1);      // |w| > pi after the update: the rotation is wrapped
    s.valid = 0; s.rot_in = {0.f, 0.f, 3.2f};
    report("rotation beyond pi", s);
  }
  {
    Step s = synthetic(7, 7, 0);      // a table that is no tree must not hang the walk
    s.chain.parent[3] = 5; s.chain.parent[5] = 3; s.chain.kp_frame[2] = 31; s.chain.cfg[1] = 40;
    report("broken chain table", s);
  }
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "self")) return self();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: kinfilter_host_check self | run <in> <out>\n");
  return 2;
}
