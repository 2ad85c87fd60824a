// Host check of the multi-view kinematic refit: csrc/kin_views_core.h's solve_one is the loop the kernel of csrc/kin_views.hip runs;
// here it runs on the host, one lane after another, under -fsanitize=address,undefined (tests/test_kinviews_host.py builds and runs
// this program).  Every buffer has its exact size, so the sanitizer sees any access past an input, an output or the shared buffer.
//   kinviews_host_check run <in> <out>   every case of <in> (tests/kinviews_oracle.py pack_case) through hrp::kinv::solve_one
//   kinviews_host_check self             hostile inputs; prints one line per input and "failures N"
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "kin_views_core.h"

namespace kin = hrp::kin;
namespace kinv = hrp::kinv;

struct HostLanes {      // lanes 0..63 one after another; nothing to wait for
  int lo() const { return 0; }
  int hi() const { return kin::KIN_LANES; }
  void sync() const {}
};

struct Case {
  int nkp = 0, dof = 0, V = 1, present = 0;      // present: 1 w2d, 2 lo, 4 hi, 8 prior
  uint32_t free_q = 0;
  hrp_fk_chain chain;
  std::vector<float> pts2d, w2d, K, poses, q0, lo, hi, prior;
};
struct Result {
  std::vector<float> q, rms_view, xyz, uv, cov;
  std::vector<int32_t> used_view;
  float rms = 0.f;
  int32_t status[4] = {0, 0, 0, 0};
};

static Result solve(const Case& c) {
  const int npar = kin::kin_npar(c.free_q, c.dof, 0);
  Result r;
  r.q.assign(c.dof, -7.f);
  r.rms_view.assign(c.V, -7.f);
  r.used_view.assign(c.V, -7);
  r.xyz.assign((size_t)3 * c.V * c.nkp, -7.f);
  r.uv.assign((size_t)2 * c.V * c.nkp, -7.f);
  r.cov.assign((size_t)npar * npar, -7.f);
  hrp_kin_views_desc d;
  memset(&d, 0, sizeof d);
  d.chain = &c.chain;
  d.pts2d = c.pts2d.data();
  d.w2d = (c.present & 1) ? c.w2d.data() : nullptr;
  d.K = c.K.data();
  d.K_stride = 9;
  d.nkp = c.nkp;
  d.q0 = c.q0.data();
  d.poses = c.poses.data();
  d.pose_stride = 1;
  d.V = c.V;
  d.q_lo = (c.present & 2) ? c.lo.data() : nullptr;
  d.q_hi = (c.present & 4) ? c.hi.data() : nullptr;
  d.prior_q = (c.present & 8) ? c.prior.data() : nullptr;
  d.free_q = c.free_q;
  d.B = 1;
  d.dof = c.dof;
  d.q = r.q.data();
  d.xyz = r.xyz.data();
  d.uv = r.uv.data();
  d.rms = &r.rms;
  d.rms_view = r.rms_view.data();
  d.status = r.status;
  d.used_view = r.used_view.data();
  d.cov = r.cov.data();
  if (const char* why = kinv::refusal(&d)) {
    fprintf(stderr, "refused: %s\n", why);
    exit(3);
  }
  std::vector<double> lds(kinv::shared_doubles(npar, c.nkp, c.V), std::numeric_limits<double>::quiet_NaN());
  kinv::solve_one(HostLanes{}, kinv::problem_of(d, 0), lds.data());
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
    c.nkp = h[0]; c.dof = h[1]; c.V = h[2]; c.free_q = (uint32_t)h[3]; c.present = h[4];
    if (c.nkp < 1 || c.nkp > HRP_FK_MAX_KP || c.dof < 0 || c.dof > HRP_FK_MAX_JOINTS || c.V < 1 || c.V > HRP_KIN_MAX_VIEWS) return 2;
    const size_t pairs = (size_t)c.V * c.nkp;
    bool ok = read_exact(f, &c.chain, sizeof c.chain) && read_floats(f, c.pts2d, 2 * pairs) && read_floats(f, c.w2d, pairs) &&
              read_floats(f, c.K, 9 * (size_t)c.V) && read_floats(f, c.poses, 6 * (size_t)c.V) && read_floats(f, c.q0, c.dof) &&
              read_floats(f, c.lo, c.dof) && read_floats(f, c.hi, c.dof) && read_floats(f, c.prior, c.dof);
    if (!ok) return 2;
    const Result r = solve(c);
    fwrite(r.q.data(), 4, r.q.size(), g);
    fwrite(&r.rms, 4, 1, g);
    fwrite(r.rms_view.data(), 4, r.rms_view.size(), g);
    fwrite(r.status, 4, 4, g);
    fwrite(r.used_view.data(), 4, r.used_view.size(), g);
    fwrite(r.xyz.data(), 4, r.xyz.size(), g);
    fwrite(r.uv.data(), 4, r.uv.size(), g);
    fwrite(r.cov.data(), 4, r.cov.size(), g);
  }
  fclose(f);
  fclose(g);
  return 0;
}

// a serial chain of `nj` revolute joints with alternating axes and `nkp` key-points spread along it, seen by V cameras about 1.5 m away
static Case synthetic(int nj, int nkp, int V) {
  Case c;
  memset(&c.chain, 0, sizeof c.chain);
  c.nkp = nkp; c.dof = nj; c.V = V;
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
  for (int v = 0; v < V; ++v) {
    const float K[9] = {600.f, 0.f, 320.f, 0.f, 600.f, 240.f, 0.f, 0.f, 1.f};
    const float pose[6] = {0.3f + 0.4f * (float)v, -0.2f - 0.1f * (float)v, 0.1f + 0.2f * (float)(v % 3), 0.05f, -0.1f, 1.5f + 0.1f * (float)v};
    c.K.insert(c.K.end(), K, K + 9);
    c.poses.insert(c.poses.end(), pose, pose + 6);
  }
  c.q0.assign(nj, 0.1f);
  c.pts2d.assign((size_t)2 * V * nkp, 300.f);
  c.w2d.assign((size_t)V * nkp, 1.f);
  c.lo.assign(nj, -3.f); c.hi.assign(nj, 3.f); c.prior.assign(nj, 1.f);
  c.free_q = nj >= 32 ? 0xffffffffu : ((1u << nj) - 1u);
  c.present = 1 | 2 | 4 | 8;
  return c;
}

static int failures = 0;
static void report(const char* name, const Case& c, const Result& r) {
  bool start = true, cov0 = true;
  for (int j = 0; j < c.dof; ++j) start = start && memcmp(&r.q[j], &c.q0[j], 4) == 0;
  for (float v : r.cov) cov0 = cov0 && v == 0.f;
  int used = 0;
  for (int v : r.used_view) used += v;
  printf("hostile %s: flags %d trials %d rows %d npar %d start %d cov0 %d used %d\n", name, r.status[0], r.status[1], r.status[2], r.status[3],
         (int)start, (int)cov0, used);
}

static int self() {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  {
    Case c = synthetic(7, 7, 3);
    c.w2d.assign(c.w2d.size(), 0.f);
    c.present &= ~8;
    report("all views unusable", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 3);
    for (auto* v : {&c.pts2d, &c.w2d, &c.K, &c.poses, &c.q0, &c.lo, &c.hi, &c.prior}) v->assign(v->size(), nan);
    report("NaN everywhere", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 2);
    for (int i = 0; i < 14; ++i) c.pts2d[i] = nan;      // view 0 is gone, view 1 is whole
    const Result r = solve(c);
    report("NaN points in one view", c, r);
    if (r.used_view[0] != 0 || r.used_view[1] != 7 || r.rms_view[0] != 0.f) ++failures;
  }
  {
    Case c = synthetic(7, 7, 2);
    for (int i = 0; i < 7; ++i) c.w2d[7 + i] = nan;      // a NaN weight is not > 0
    const Result r = solve(c);
    report("NaN weights in one view", c, r);
    if (r.used_view[0] != 7 || r.used_view[1] != 0) ++failures;
  }
  {
    Case c = synthetic(7, 7, 2);      // the pose and K of a view without a used point are never part of the cost
    for (int i = 0; i < 7; ++i) c.w2d[7 + i] = 0.f;
    for (int i = 0; i < 6; ++i) c.poses[6 + i] = nan;
    for (int i = 0; i < 9; ++i) c.K[9 + i] = nan;
    report("NaN pose and K of an unused view", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 2);
    c.poses[7] = nan;
    report("NaN pose of a used view", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 2);
    c.K[9 + 4] = nan;
    report("NaN K of a used view", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 3);
    c.poses[6 * 1 + 5] = -1.5f;
    report("a view behind its camera", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 2);
    c.lo.assign(7, 1.f); c.hi.assign(7, -1.f);
    const Result r = solve(c);
    report("lo > hi", c, r);
    for (int j = 0; j < 7; ++j)
      if (!(r.q[j] == -1.f || r.q[j] == c.q0[j])) { printf("lo > hi: q[%d] = %g\n", j, r.q[j]); ++failures; }
  }
  {
    Case c = synthetic(7, 7, 2);      // 7 parameters: 3 points of view 0 and 1 prior are 7 rows, without the prior 6
    c.w2d.assign(14, 0.f);
    c.w2d[0] = c.w2d[1] = c.w2d[2] = 1.f;
    c.prior.assign(7, 0.f);
    c.prior[2] = 1.f;
    report("rows == npar", c, solve(c));
    c.present &= ~8;
    report("rows == npar - 1", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 1);
    report("V 1", c, solve(c));
  }
  {
    Case c = synthetic(32, 24, 8);      // the largest: every buffer at its limit
    const Result r = solve(c);
    report("dof 32 nkp 24 V 8", c, r);
    if (r.status[3] != 32 || r.status[2] != 2 * 8 * 24 + 32) ++failures;
  }
  {
    Case c = synthetic(32, 24, 8);
    c.free_q = 1u << 31;
    report("dof 32 nkp 24 V 8 npar 1", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 2);
    c.free_q = 0;
    report("nothing free", c, solve(c));
  }
  {
    Case c = synthetic(7, 7, 2);      // a table that is no tree must not hang the walk
    c.chain.parent[3] = 5; c.chain.parent[5] = 3; c.chain.kp_frame[2] = 31; c.chain.cfg[1] = 40;
    report("broken chain table", c, solve(c));
  }
  printf("failures %d\n", failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "self")) return self();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  fprintf(stderr, "usage: kinviews_host_check self | run <in> <out>\n");
  return 2;
}
