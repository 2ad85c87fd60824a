// Host check of csrc/pnp_minimal.h (the per-hypothesis core of hrp_pnp_solve_robust), built by tests/test_pnp_minimal_host.py with the
// host compiler under -fsanitize=address,undefined -fno-sanitize-recover.
//   self               P3P on exact triples and on degenerate ones, the unranking, the sampled triples; prints "failures N"
//   loop <in> <out>    the hypothesise / score / re-score loop of the kernel on the samples of <in>, the LM refit replaced by the pose
//                      that <in> carries; writes hypotheses, the winner's count, rounds, the winner's mask and the final mask per sample
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnp_minimal.h"

using namespace pnpmin;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
    }                                    \
  } while (0)

static uint64_t rng_state = 0x1234567ull;
static double urand() {      // [0, 1)
  rng_state += 0x9E3779B97F4A7C15ull;
  return (double)(splitmix64(rng_state) >> 11) / 9007199254740992.0;
}

static bool all_finite(const double (&R)[3][3], const double (&t)[3]) {
  for (int r = 0; r < 3; ++r) {
    if (!finite64(t[r])) return false;
    for (int k = 0; k < 3; ++k)
      if (!finite64(R[r][k])) return false;
  }
  return true;
}

static void test_p3p_exact() {
  const double K[9] = {615.0, 0.0, 320.0, 0.0, 612.0, 240.0, 0.0, 0.0, 1.0};
  double worst_pose = 0.0, worst_px = 0.0;
  int total_roots = 0;
  for (int trial = 0; trial < 2000; ++trial) {
    double w[3], Rt[3][3], tt[3], X[3][3], f[3][3], x[3][2];
    for (int k = 0; k < 3; ++k) w[k] = (urand() - 0.5) * 4.0;
    aa_to_rot(w, Rt);
    tt[0] = (urand() - 0.5) * 0.4; tt[1] = (urand() - 0.5) * 0.3; tt[2] = 0.8 + urand() * 1.5;
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) X[i][k] = (urand() - 0.5) * 0.8;
      double c[3];
      for (int r = 0; r < 3; ++r) c[r] = Rt[r][0] * X[i][0] + Rt[r][1] * X[i][1] + Rt[r][2] * X[i][2] + tt[r];
      x[i][0] = K[0] * c[0] / c[2] + K[2];
      x[i][1] = K[4] * c[1] / c[2] + K[5];
      CHECK(bearing(K, x[i], f[i]), "bearing");
    }
    // skip triangles the solver calls degenerate on purpose (thin ones): the test is about exactness, not conditioning
    double e1[3], e2[3], nn[3];
    for (int k = 0; k < 3; ++k) { e1[k] = X[1][k] - X[0][k]; e2[k] = X[2][k] - X[0][k]; }
    cross3(e1, e2, nn);
    if (dot3(nn, nn) < 1e-2 * dot3(e1, e1) * dot3(e2, e2)) continue;
    double R[4][3][3], t[4][3];
    const int cnt = p3p_solve(X, f, R, t);
    CHECK(cnt >= 1 && cnt <= 4, "trial %d: %d roots", trial, cnt);
    total_roots += cnt;
    double best = 1e300;
    for (int s = 0; s < cnt; ++s) {
      CHECK(all_finite(R[s], t[s]), "trial %d root %d not finite", trial, s);
      double d = 0.0;
      for (int r = 0; r < 3; ++r) {
        d = fmax(d, fabs(t[s][r] - tt[r]));
        for (int k = 0; k < 3; ++k) d = fmax(d, fabs(R[s][r][k] - Rt[r][k]));
      }
      best = fmin(best, d);
      for (int i = 0; i < 3; ++i) {
        double e2v;
        const bool front = reproj_e2(R[s], t[s], K, X[i], x[i], e2v);
        CHECK(front, "trial %d root %d: point %d behind the camera", trial, s, i);
        worst_px = fmax(worst_px, sqrt(e2v));
      }
      // a rotation: R R^T = I, det = +1
      double det = R[s][0][0] * (R[s][1][1] * R[s][2][2] - R[s][1][2] * R[s][2][1]) - R[s][0][1] * (R[s][1][0] * R[s][2][2] - R[s][1][2] * R[s][2][0]) +
                   R[s][0][2] * (R[s][1][0] * R[s][2][1] - R[s][1][1] * R[s][2][0]);
      CHECK(fabs(det - 1.0) < 1e-9, "trial %d root %d: det %g", trial, s, det);
    }
    worst_pose = fmax(worst_pose, best);
  }
  std::printf("p3p exact: worst pose error %.3e, worst reprojection %.3e px, %d roots\n", worst_pose, worst_px, total_roots);
  CHECK(worst_pose < 1e-9, "pose error %g", worst_pose);
  CHECK(worst_px < 1e-6, "reprojection %g px", worst_px);
  // angle-axis round trip, through pi and zero
  for (int trial = 0; trial < 1000; ++trial) {
    double w[3], R[3][3], w2[3], R2[3][3];
    const double scale = trial % 3 == 0 ? 1e-6 : (trial % 3 == 1 ? 3.14159 : 1.0);
    for (int k = 0; k < 3; ++k) w[k] = (urand() - 0.5) * 2.0 * scale;
    aa_to_rot(w, R);
    rot_to_aa(R, w2);
    aa_to_rot(w2, R2);
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) CHECK(fabs(R[r][k] - R2[r][k]) < 1e-12, "angle-axis round trip %g", fabs(R[r][k] - R2[r][k]));
  }
}

static void test_p3p_degenerate() {
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const double good_f[3][3] = {{0.1, 0.0, 1.0}, {-0.1, 0.05, 1.0}, {0.0, -0.1, 1.0}};
  const double good_X[3][3] = {{0.1, 0.0, 0.0}, {-0.1, 0.1, 0.0}, {0.0, -0.2, 0.1}};
  struct Case { const char* name; double X[3][3]; double f[3][3]; };
  std::vector<Case> cases;
  auto add = [&](const char* name, const double (&X)[3][3], const double (&f)[3][3]) {
    Case c;
    c.name = name;
    std::memcpy(c.X, X, sizeof(c.X));
    std::memcpy(c.f, f, sizeof(c.f));
    cases.push_back(c);
  };
  { double X[3][3] = {{0, 0, 0}, {0.1, 0.1, 0.1}, {0.2, 0.2, 0.2}}; add("collinear", X, good_f); }
  { double X[3][3] = {{0, 0, 0}, {0.1, 0.1, 0.1}, {0.2, 0.2, 0.2 + 1e-9}}; add("near_collinear", X, good_f); }
  { double X[3][3] = {{0.1, 0, 0}, {0.1, 0, 0}, {0, -0.2, 0.1}}; add("coincident_points", X, good_f); }
  { double X[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}; add("all_coincident", X, good_f); }
  { double f[3][3] = {{0.1, 0, 1}, {0.1, 0, 1}, {0, -0.1, 1}}; add("coincident_bearings", good_X, f); }
  { double f[3][3] = {{0, 0, 0}, {-0.1, 0.05, 1}, {0, -0.1, 1}}; add("zero_bearing", good_X, f); }
  { double X[3][3] = {{nan, 0, 0}, {-0.1, 0.1, 0}, {0, -0.2, 0.1}}; add("nan_point", X, good_f); }
  { double X[3][3] = {{inf, 0, 0}, {-0.1, 0.1, 0}, {0, -0.2, 0.1}}; add("inf_point", X, good_f); }
  { double X[3][3] = {{1e300, 0, 0}, {-1e300, 0.1, 0}, {0, -0.2, 0.1}}; add("huge_point", X, good_f); }
  { double f[3][3] = {{nan, 0, 1}, {-0.1, 0.05, 1}, {0, -0.1, 1}}; add("nan_bearing", good_X, f); }
  { double f[3][3] = {{0.1, 0, 1}, {-0.1, inf, 1}, {0, -0.1, 1}}; add("inf_bearing", good_X, f); }
  for (const Case& c : cases) {
    double R[4][3][3], t[4][3];
    const int cnt = p3p_solve(c.X, c.f, R, t);
    std::printf("degenerate %s roots %d\n", c.name, cnt);
    CHECK(cnt == 0, "%s: %d roots", c.name, cnt);
  }
  // the well-formed triple of the cases above has poses, all finite
  double R[4][3][3], t[4][3];
  const int cnt = p3p_solve(good_X, good_f, R, t);
  CHECK(cnt >= 1, "good triple: %d roots", cnt);
  for (int s = 0; s < cnt; ++s) CHECK(all_finite(R[s], t[s]), "good triple root %d", s);
}

static void test_enumeration() {
  const int sizes[5] = {4, 7, 8, 17, 19};
  for (int m : sizes) {
    const int total = ncomb3(m);
    CHECK(hypothesis_count(m, 1024) == total, "count %d", m);
    std::vector<char> seen((size_t)m * m * m, 0);
    int pi = -1, pj = -1, pk = -1;
    for (int h = 0; h < total; ++h) {
      int i, j, k;
      hypothesis_triple(h, m, 1024, 7u, i, j, k);
      CHECK(0 <= i && i < j && j < k && k < m, "m %d h %d: (%d %d %d)", m, h, i, j, k);
      if (!(0 <= i && i < j && j < k && k < m)) continue;
      char& s = seen[((size_t)i * m + j) * m + k];
      CHECK(!s, "m %d h %d: triple repeated", m, h);
      s = 1;
      CHECK(h == 0 || i > pi || (i == pi && (j > pj || (j == pj && k > pk))), "m %d h %d: not lexicographic", m, h);
      pi = i; pj = j; pk = k;
    }
    std::printf("unrank m %d: %d triples\n", m, total);
  }
  CHECK(ncomb3(19) == 969 && ncomb3(20) == 1140 && ncomb3(24) == 2024 && ncomb3(64) == 41664, "ncomb3");
  CHECK(hypothesis_count(3, 1024) == 0 && hypothesis_count(24, 1024) == 1024 && hypothesis_count(64, 100) == 100, "hypothesis_count");
  // sampled path
  const int ms[4] = {20, 24, 33, 64};
  for (int m : ms) {
    int differ = 0;
    std::vector<int> hits(m, 0);
    for (uint32_t seed = 0; seed < 3; ++seed)
      for (int h = 0; h < 1024; ++h) {
        int i, j, k, i2, j2, k2, i3, j3, k3;
        hypothesis_triple(h, m, 1024, seed, i, j, k);
        hypothesis_triple(h, m, 1024, seed, i2, j2, k2);
        hypothesis_triple(h, m, 1024, seed + 1, i3, j3, k3);
        CHECK(0 <= i && i < j && j < k && k < m, "sampled m %d h %d: (%d %d %d)", m, h, i, j, k);
        CHECK(i == i2 && j == j2 && k == k2, "sampled m %d h %d: not a function of (seed, h)", m, h);
        differ += i != i3 || j != j3 || k != k3;
        if (0 <= i && k < m) { ++hits[i]; ++hits[j]; ++hits[k]; }
      }
    CHECK(differ > 2500, "sampled m %d: the seed changes only %d of 3072 triples", m, differ);
    for (int p = 0; p < m; ++p) CHECK(hits[p] > 0, "sampled m %d: index %d never drawn", m, p);
  }
}

// ---- the kernel's loop on one sample ------------------------------------------------------------------------------------------------
struct Sample {
  int n, max_hyp, seed, min_inliers;
  double thr, K[9];
  std::vector<double> X, x, pose;     // n x 3, n x 2, 6
};

static unsigned long long score_mask(const Sample& s, const double (&R)[3][3], const double (&t)[3], const std::vector<int>& idx,
                                     int& count, double& ssq) {
  unsigned long long mask = 0;
  count = 0;
  ssq = 0.0;
  for (int p : idx) {
    const double X[3] = {s.X[3 * p], s.X[3 * p + 1], s.X[3 * p + 2]}, x[2] = {s.x[2 * p], s.x[2 * p + 1]};
    double e2;
    if (reproj_e2(R, t, s.K, X, x, e2) && e2 < s.thr * s.thr) {
      mask |= 1ull << p;
      ++count;
      ssq += e2;
    }
  }
  return mask;
}

static void run_loop(const Sample& s, std::FILE* out) {
  std::vector<int> idx;
  std::vector<double> F(3 * s.n, 0.0);
  for (int p = 0; p < s.n; ++p) {
    const double X[3] = {s.X[3 * p], s.X[3 * p + 1], s.X[3 * p + 2]}, x[2] = {s.x[2 * p], s.x[2 * p + 1]};
    double f[3];
    if (point_valid(nullptr, X, x) && bearing(s.K, x, f)) {
      idx.push_back(p);
      for (int k = 0; k < 3; ++k) F[3 * p + k] = f[k];
    }
  }
  const int m = (int)idx.size(), H = hypothesis_count(m, s.max_hyp);
  int best_count = -1;
  double best_ssq = 0.0;
  unsigned long long best_mask = 0;
  for (int h = 0; h < H; ++h) {
    int tri[3];
    hypothesis_triple(h, m, s.max_hyp, (uint32_t)s.seed, tri[0], tri[1], tri[2]);
    double X3[3][3], f3[3][3];
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < 3; ++k) {
        X3[a][k] = s.X[3 * idx[tri[a]] + k];
        f3[a][k] = F[3 * idx[tri[a]] + k];
      }
    P3P S;
    p3p_prepare(X3, f3, S);
    for (int slot = 0; slot < 4; ++slot) {
      double R[3][3], t[3];
      if (!p3p_pose(S, slot, R, t)) continue;
      int count;
      double ssq;
      const unsigned long long mask = score_mask(s, R, t, idx, count, ssq);
      if (score_better(count, ssq, best_count, best_ssq)) {
        best_count = count;
        best_ssq = ssq;
        best_mask = mask;
      }
    }
  }
  // local optimisation with the refit replaced by the carried pose
  unsigned long long fit = best_mask, fin = best_mask;
  int rounds = 0;
  if (best_count >= s.min_inliers) {
    double w[3] = {s.pose[0], s.pose[1], s.pose[2]}, t[3] = {s.pose[3], s.pose[4], s.pose[5]}, R[3][3];
    aa_to_rot(w, R);
    for (; rounds < 3;) {
      ++rounds;
      int count;
      double ssq;
      fin = score_mask(s, R, t, idx, count, ssq);
      if (fin == fit) break;
      fit = fin;
    }
  }
  const int32_t head[3] = {H, best_count, rounds};
  std::fwrite(head, sizeof(head), 1, out);
  std::vector<unsigned char> m0(s.n), m1(s.n);
  for (int p = 0; p < s.n; ++p) {
    m0[p] = (best_mask >> p) & 1;
    m1[p] = (fin >> p) & 1;
  }
  std::fwrite(m0.data(), 1, s.n, out);
  std::fwrite(m1.data(), 1, s.n, out);
}

static bool read_exact(void* dst, size_t bytes, std::FILE* f) { return std::fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "self")) {
    test_p3p_exact();
    test_p3p_degenerate();
    test_enumeration();
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
  }
  if (argc >= 4 && !std::strcmp(argv[1], "loop")) {
    std::FILE* in = std::fopen(argv[2], "rb");
    std::FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int32_t cases = 0;
    if (!read_exact(&cases, 4, in)) return 2;
    for (int c = 0; c < cases; ++c) {
      Sample s;
      int32_t head[4];
      if (!read_exact(head, sizeof(head), in) || head[0] < 4 || head[0] > 64) return 2;
      s.n = head[0]; s.max_hyp = head[1]; s.seed = head[2]; s.min_inliers = head[3];
      s.X.resize(3 * s.n); s.x.resize(2 * s.n); s.pose.resize(6);
      if (!read_exact(&s.thr, 8, in) || !read_exact(s.K, sizeof(s.K), in) || !read_exact(s.X.data(), 8 * s.X.size(), in) ||
          !read_exact(s.x.data(), 8 * s.x.size(), in) || !read_exact(s.pose.data(), 48, in))
        return 2;
      run_loop(s, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
  }
  std::fprintf(stderr, "usage: %s self | loop <in> <out>\n", argv[0]);
  return 2;
}
