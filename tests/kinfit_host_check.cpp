// Host check of the kinematic refit: csrc/kin_core.h's solve_one is the loop the kernel of csrc/kin.hip runs; here it runs on the host,
// one lane after another, under -fsanitize=address,undefined (tests/test_kinfit_host.py builds and runs this program).
//   kinfit_host_check run <in> <out>   every case of <in> (tests/kinfit_oracle.py pack_case) through hrp::kin::solve_one; results to <out>
//   kinfit_host_check self             hostile inputs; prints one line per input and "failures N"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "kin_core.h"

namespace kin = hrp::kin;

struct HostLanes {      // lanes 0..63 one after another; nothing to wait for
  int lo() const { return 0; }
  int hi() const { return kin::KIN_LANES; }
  void sync() const {}
};

struct Case {
  int nkp = 0, dof = 0, rot_dim = 3, free_pose = 0, root = 0, present = 0;
  uint32_t free_q = 0;
  hrp_fk_chain chain;
  std::vector<float> pts2d, w2d, pts3d, w3d, K, q0, rot0, trans0, lo, hi, prior;
};
struct Result {
  std::vector<float> q, rot, trans, xyz, uv, cov;
  float rms = 0.f;
  int32_t status[4] = {0, 0, 0, 0};
};

static Result solve(const Case& c) {
  const int npar = kin::kin_npar(c.free_q, c.dof, c.free_pose);
  Result r;
  // exact sizes, so that the sanitizer sees any access past an output or past the shared buffer
  r.q.assign(c.dof, -7.f);
  r.rot.assign(c.rot_dim, -7.f);
  r.trans.assign(3, -7.f);
  r.xyz.assign(3 * c.nkp, -7.f);
  r.uv.assign(2 * c.nkp, -7.f);
  r.cov.assign((size_t)npar * npar, -7.f);
  const bool has3d = (c.present & 2) && (c.present & 4);
  hrp_kin_desc d;
  memset(&d, 0, sizeof d);
  d.chain = &c.chain;
  d.pts2d = c.pts2d.data();
  d.w2d = (c.present & 1) ? c.w2d.data() : nullptr;
  d.pts3d = has3d ? c.pts3d.data() : nullptr;
  d.w3d = has3d ? c.w3d.data() : nullptr;
  d.K = c.K.data();
  d.K_stride = 9;
  d.nkp = c.nkp;
  d.dof = c.dof;
  d.q0 = c.q0.data();
  d.rot0 = c.rot0.data();
  d.trans0 = c.trans0.data();
  d.rot_dim = c.rot_dim;
  d.pose_stride = 1;
  d.q_lo = (c.present & 8) ? c.lo.data() : nullptr;
  d.q_hi = (c.present & 16) ? c.hi.data() : nullptr;
  d.prior_q = (c.present & 32) ? c.prior.data() : nullptr;
  d.free_q = c.free_q;
  d.free_pose = c.free_pose;
  d.root = c.root;
  d.B = 1;
  d.q = r.q.data();
  d.rot = r.rot.data();
  d.trans = r.trans.data();
  d.xyz = r.xyz.data();
  d.uv = r.uv.data();
  d.rms = &r.rms;
  d.status = r.status;
  d.cov = r.cov.data();
  if (const char* why = kin::refusal(&d)) {
    fprintf(stderr, "refused: %s\n", why);
    exit(3);
  }
  std::vector<double> lds(kin::shared_doubles(npar, c.nkp, has3d), std::numeric_limits<double>::quiet_NaN());
  if (lds.size() * sizeof(double) > 64 * 1024) {
    fprintf(stderr, "LDS %zu bytes\n", lds.size() * sizeof(double));
    exit(3);
  }
  kin::solve_one(HostLanes{}, kin::problem_of(d, 0), lds.data());
  return r;
}

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool read_floats(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  return read_exact(f, v.data(), 4 * n);
}

static int run(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  FILE* g = fopen(out, "wb");
  if (!f || !g) return 2;
  int32_t n = 0;
  if (!read_exact(f, &n, 4)) return 2;
  for (int i = 0; i < n; ++i) {
    int32_t h[8];
    Case c;
    if (!read_exact(f, h, sizeof h)) return 2;
    c.nkp = h[0]; c.dof = h[1]; c.rot_dim = h[2]; c.free_pose = h[3]; c.root = h[4]; c.free_q = (uint32_t)h[5]; c.present = h[6];
    if (c.nkp < 1 || c.nkp > HRP_FK_MAX_KP || c.dof < 0 || c.dof > HRP_FK_MAX_JOINTS || (c.rot_dim != 3 && c.rot_dim != 6)) return 2;
    bool ok = read_exact(f, &c.chain, sizeof c.chain) && read_floats(f, c.pts2d, 2 * c.nkp) && read_floats(f, c.w2d, c.nkp) &&
              read_floats(f, c.pts3d, 3 * c.nkp) && read_floats(f, c.w3d, c.nkp) && read_floats(f, c.K, 9) && read_floats(f, c.q0, c.dof) &&
              read_floats(f, c.rot0, c.rot_dim) && read_floats(f, c.trans0, 3) && read_floats(f, c.lo, c.dof) && read_floats(f, c.hi, c.dof) &&
              read_floats(f, c.prior, c.dof);
    if (!ok) return 2;
    const Result r = solve(c);
    fwrite(r.q.data(), 4, r.q.size(), g);
    fwrite(r.rot.data(), 4, r.rot.size(), g);
    fwrite(r.trans.data(), 4, 3, g);
    fwrite(&r.rms, 4, 1, g);
    fwrite(r.status, 4, 4, g);
    fwrite(r.xyz.data(), 4, r.xyz.size(), g);
    fwrite(r.uv.data(), 4, r.uv.size(), g);
    fwrite(r.cov.data(), 4, r.cov.size(), g);
  }
  fclose(f);
  fclose(g);
  return 0;
}

// a serial chain of `nj` revolute joints with alternating axes and `nkp` key-points spread along it, about 1.5 m in front of the camera
static Case synthetic(int nj, int nkp) {
  Case c;
  memset(&c.chain, 0, sizeof c.chain);
  c.nkp = nkp; c.dof = nj;
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
  c.K = {600.f, 0.f, 320.f, 0.f, 600.f, 240.f, 0.f, 0.f, 1.f};
  c.q0.assign(nj, 0.1f);
  c.rot0 = {0.3f, -0.2f, 0.1f};
  c.trans0 = {0.05f, -0.1f, 1.5f};
  c.pts2d.assign(2 * nkp, 300.f);
  c.w2d.assign(nkp, 1.f); c.pts3d.assign(3 * nkp, 0.f); c.w3d.assign(nkp, 0.f);
  c.lo.assign(nj, -3.f); c.hi.assign(nj, 3.f); c.prior.assign(nj, 1.f);
  c.free_q = nj >= 32 ? 0xffffffffu : ((1u << nj) - 1u);
  c.free_pose = 1;
  c.present = 1 | 8 | 16 | 32;
  return c;
}

static int failures = 0;
static void report(const char* name, const Case& c, const Result& r) {
  bool start = true;
  for (int j = 0; j < c.dof; ++j) start = start && memcmp(&r.q[j], &c.q0[j], 4) == 0;
  start = start && memcmp(r.rot.data(), c.rot0.data(), 4 * c.rot_dim) == 0 && memcmp(r.trans.data(), c.trans0.data(), 12) == 0;
  bool cov0 = true;
  for (float v : r.cov) cov0 = cov0 && v == 0.f;
  printf("hostile %s: flags %d trials %d rows %d npar %d start %d cov0 %d\n", name, r.status[0], r.status[1], r.status[2], r.status[3], (int)start,
         (int)cov0);
}

static int self() {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  {
    Case c = synthetic(7, 7);
    c.w2d.assign(7, 0.f);
    c.present &= ~32;
    report("all weights 0", c, solve(c));
  }
  {
    Case c = synthetic(7, 7);
    for (auto* v : {&c.pts2d, &c.w2d, &c.K, &c.q0, &c.rot0, &c.trans0, &c.lo, &c.hi, &c.prior}) v->assign(v->size(), nan);
    report("NaN everywhere", c, solve(c));
  }
  {
    Case c = synthetic(7, 7);
    c.pts2d.assign(14, nan);
    c.q0.assign(7, nan);
    report("NaN points and q0, weights 1", c, solve(c));
  }
  {
    Case c = synthetic(7, 7);
    c.free_q = 0; c.free_pose = 0;
    report("nothing free", c, solve(c));
  }
  {
    Case c = synthetic(7, 7);
    c.trans0[2] = -1.5f;
    report("start behind the camera", c, solve(c));
  }
  {
    Case c = synthetic(7, 7);
    c.lo.assign(7, 1.f); c.hi.assign(7, -1.f);
    const Result r = solve(c);
    report("lo > hi", c, r);
    for (int j = 0; j < 7; ++j)
      if (!(r.q[j] == -1.f || r.q[j] == c.q0[j])) { printf("lo > hi: q[%d] = %g\n", j, r.q[j]); ++failures; }
  }
  {
    Case c = synthetic(32, 24);      // npar 38, the largest: every buffer at its limit
    c.pts3d.assign(72, 0.5f); c.w3d.assign(24, 1.f); c.present |= 2 | 4;
    const Result r = solve(c);
    report("dof 32 nkp 24 with 3-D targets", c, r);
    if (r.status[3] != 38 || r.status[2] != 48 + 72 + 32) ++failures;
  }
  {
    Case c = synthetic(32, 24);
    c.rot_dim = 6;
    c.rot0 = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    c.root = 23;
    report("dof 32 nkp 24 rot_dim 6 root 23", c, solve(c));
  }
  {
    Case c = synthetic(0, 5);      // no joints at all: a pose-only problem
    report("dof 0", c, solve(c));
  }
  {
    Case c = synthetic(7, 7);      // a table that is no tree must not hang the walk
    c.chain.parent[3] = 5; c.chain.parent[5] = 3; c.chain.kp_frame[2] = 31; c.chain.cfg[1] = 40;
    report("broken chain table", c, solve(c));
  }
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "self")) return self();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: kinfit_host_check self | run <in> <out>\n");
  return 2;
}
