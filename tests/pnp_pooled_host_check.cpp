// Host check of the pooled robust PnP's loop (csrc/pnp_pooled.hip over csrc/pnp_minimal.h), built by tests/test_pnp_pooled_host.py with
// the host compiler under -fsanitize=address,undefined -fno-sanitize-recover and run as a plain executable.
//   self               the capped 64-bit hypothesis count, the sampled triples at m = 16384, hostile inputs; prints "failures N"
//   loop <in> <out>    compaction, hypothesis count and triples, scoring, the winner, and the re-score loop of the fit launch on the
//                      problems of <in>, the LM refit replaced by the pose that <in> carries; writes m, H, the winner's count, the
//                      rounds, the winner's mask and the final mask per problem
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hrp.h"
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

struct Problem {
  int n, max_hyp, seed, min_inliers;
  double thr, K[9];
  std::vector<double> X, x, pose;        // n x 3, n x 2, 6
  std::vector<unsigned char> valid;      // n
};
struct Outcome {
  int m, H, best_count, rounds;
  std::vector<unsigned char> winner, final_mask;     // n each
};

static int score(const Problem& s, const double (&R)[3][3], const double (&t)[3], const std::vector<int>& idx, double& ssq,
                 std::vector<unsigned char>* mask) {
  int count = 0;
  ssq = 0.0;
  if (mask) mask->assign(s.n, 0);
  for (int p : idx) {
    const double X[3] = {s.X[3 * p], s.X[3 * p + 1], s.X[3 * p + 2]}, x[2] = {s.x[2 * p], s.x[2 * p + 1]};
    double e2;
    if (reproj_e2(R, t, s.K, X, x, e2) && e2 < s.thr * s.thr) {
      if (mask) (*mask)[p] = 1;
      ++count;
      ssq += e2;
    }
  }
  return count;
}

static Outcome run_loop(const Problem& s) {
  Outcome o;
  // 1. the usable points in index order
  std::vector<int> idx;
  for (int p = 0; p < s.n; ++p) {
    const double X[3] = {s.X[3 * p], s.X[3 * p + 1], s.X[3 * p + 2]}, x[2] = {s.x[2 * p], s.x[2 * p + 1]};
    double f[3];
    if (point_valid(&s.valid[p], X, x) && bearing(s.K, x, f)) idx.push_back(p);
  }
  // 2. hypotheses
  o.m = (int)idx.size();
  o.H = pooled_hypothesis_count(o.m, s.max_hyp);
  // 3. one record per hypothesis: its best root, ties to the lower slot; 4. the winner: ties to the lower hypothesis
  int best_count = -1;
  double best_ssq = 0.0, bR[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, bt[3] = {0, 0, 0};
  for (int h = 0; h < o.H; ++h) {
    int tri[3];
    pooled_hypothesis_triple(h, o.m, s.max_hyp, (uint32_t)s.seed, tri[0], tri[1], tri[2]);
    double X3[3][3], f3[3][3];
    for (int a = 0; a < 3; ++a) {
      const int p = idx[tri[a]];
      const double x[2] = {s.x[2 * p], s.x[2 * p + 1]};
      for (int k = 0; k < 3; ++k) X3[a][k] = s.X[3 * p + k];
      bearing(s.K, x, f3[a]);
    }
    P3P S;
    p3p_prepare(X3, f3, S);
    int rc = -1;
    double rs = 0.0, rR[3][3], rt[3];
    for (int slot = 0; slot < 4; ++slot) {
      double R[3][3], t[3], ssq;
      if (!p3p_pose(S, slot, R, t)) continue;
      const int count = score(s, R, t, idx, ssq, nullptr);
      if (score_better(count, ssq, rc, rs)) {
        rc = count;
        rs = ssq;
        std::memcpy(rR, R, sizeof(R));
        std::memcpy(rt, t, sizeof(t));
      }
    }
    if (rc >= 0 && score_better(rc, rs, best_count, best_ssq)) {
      best_count = rc;
      best_ssq = rs;
      std::memcpy(bR, rR, sizeof(rR));
      std::memcpy(bt, rt, sizeof(rt));
    }
  }
  o.best_count = best_count;
  double ssq;
  score(s, bR, bt, idx, ssq, &o.winner);
  if (best_count < 0) o.winner.assign(s.n, 0);
  // 5. re-score, with the carried pose standing in for the LM refit
  o.final_mask = o.winner;
  o.rounds = 0;
  if (best_count >= s.min_inliers) {
    const double w[3] = {s.pose[0], s.pose[1], s.pose[2]}, t[3] = {s.pose[3], s.pose[4], s.pose[5]};
    double R[3][3];
    aa_to_rot(w, R);
    std::vector<unsigned char> fit = o.winner;
    while (o.rounds < HRP_PNP_POOLED_REFITS) {
      ++o.rounds;
      score(s, R, t, idx, ssq, &o.final_mask);
      if (o.final_mask == fit) break;
      fit = o.final_mask;
    }
  }
  return o;
}

static void test_count() {
  for (int m = 0; m <= 64; ++m) {
    CHECK(ncomb3_capped(m, INT64_MAX) == ncomb3(m), "m %d: %lld", m, (long long)ncomb3_capped(m, INT64_MAX));
    CHECK(ncomb3_capped(m, 1024) == (ncomb3(m) < 1024 ? ncomb3(m) : 1024), "m %d capped", m);
    CHECK(pooled_hypothesis_count(m, 1024) == hypothesis_count(m, 1024), "m %d hypotheses", m);
  }
  const int big[3] = {2343, 2344, 16384};
  for (int m : big) {
    const int64_t want = (int64_t)m * (m - 1) * (m - 2) / 6;      // 7.3e11 at most: fits
    CHECK(ncomb3_capped(m, INT64_MAX) == want, "m %d: %lld != %lld", m, (long long)ncomb3_capped(m, INT64_MAX), (long long)want);
    CHECK(ncomb3_capped(m, want) == want && ncomb3_capped(m, want - 1) == want - 1 && ncomb3_capped(m, want + 1) == want, "m %d at its cap", m);
    CHECK(pooled_hypothesis_count(m, 1024) == 1024 && pooled_hypothesis_count(m, 1 << 20) == (1 << 20), "m %d budget", m);
    std::printf("count m %d: %lld\n", m, (long long)ncomb3_capped(m, INT64_MAX));
  }
  CHECK(ncomb3_capped(2147483647, INT64_MAX) == INT64_MAX && ncomb3_capped(2147483647, 1024) == 1024, "m = INT_MAX");
  CHECK(ncomb3_capped(2, 10) == 0 && ncomb3_capped(10, 0) == 0 && pooled_hypothesis_count(3, 1024) == 0, "small");
  // enumerated where C(m, 3) fits the budget: the triples of unrank_triple
  int i, j, k, i2, j2, k2;
  pooled_hypothesis_triple(30, 7, 1024, 5u, i, j, k);
  unrank_triple(30, 7, i2, j2, k2);
  CHECK(i == i2 && j == j2 && k == k2, "enumerated triple");
  pooled_hypothesis_triple(30, 185, 1 << 20, 5u, i, j, k);        // C(185, 3) = 1038220 <= 2^20
  unrank_triple(30, 185, i2, j2, k2);
  CHECK(i == i2 && j == j2 && k == k2, "enumerated triple at the budget");
}

static void test_sampled() {
  const int m = 16384;
  std::vector<int> hits(m, 0);
  int differ = 0, bad = 0;
  for (uint32_t seed = 0; seed < 3; ++seed)
    for (int h = 0; h < 4096; ++h) {
      int i, j, k, i2, j2, k2, i3, j3, k3;
      pooled_hypothesis_triple(h, m, 1024, seed, i, j, k);
      pooled_hypothesis_triple(h, m, 1024, seed, i2, j2, k2);
      pooled_hypothesis_triple(h, m, 1024, seed + 1, i3, j3, k3);
      if (!(0 <= i && i < j && j < k && k < m)) { ++bad; continue; }
      CHECK(i == i2 && j == j2 && k == k2, "sampled h %d: not a function of (seed, h)", h);
      differ += i != i3 || j != j3 || k != k3;
      ++hits[i]; ++hits[j]; ++hits[k];
    }
  int touched = 0;
  for (int p = 0; p < m; ++p) touched += hits[p] > 0;
  std::printf("sampled m %d: %d triples out of order or range, %d differ under the next seed, %d indices drawn\n", m, bad, differ, touched);
  CHECK(bad == 0, "%d sampled triples not distinct, ascending and within [0, m)", bad);
  CHECK(differ > 12000 && touched > 12000, "sampling too narrow");
}

static uint64_t rng_state = 0x7654321ull;
static double urand() {
  rng_state += 0x9E3779B97F4A7C15ull;
  return (double)(splitmix64(rng_state) >> 11) / 9007199254740992.0;
}

static void test_hostile() {
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  Problem s;
  s.n = 70; s.max_hyp = 1024; s.seed = 0; s.min_inliers = 4; s.thr = 3.0;
  const double K[9] = {615.0, 0.0, 320.0, 0.0, 615.0, 240.0, 0.0, 0.0, 1.0};
  std::memcpy(s.K, K, sizeof(K));
  const double w[3] = {0.3, -0.2, 0.1}, t[3] = {0.05, -0.1, 2.0};
  double R[3][3];
  aa_to_rot(w, R);
  s.pose = {w[0], w[1], w[2], t[0], t[1], t[2]};
  s.X.resize(3 * s.n); s.x.resize(2 * s.n); s.valid.assign(s.n, 1);
  for (int p = 0; p < s.n; ++p) {
    double c[3];
    for (int k = 0; k < 3; ++k) s.X[3 * p + k] = (urand() - 0.5) * 0.9;
    for (int r = 0; r < 3; ++r) c[r] = R[r][0] * s.X[3 * p] + R[r][1] * s.X[3 * p + 1] + R[r][2] * s.X[3 * p + 2] + t[r];
    s.x[2 * p] = K[0] * c[0] / c[2] + K[2];
    s.x[2 * p + 1] = K[4] * c[1] / c[2] + K[5];
  }
  Outcome o = run_loop(s);
  CHECK(o.m == 70 && o.H == 1024 && o.best_count == 70 && o.rounds == 1, "clean: m %d H %d count %d rounds %d", o.m, o.H, o.best_count, o.rounds);
  Problem h = s;
  h.x[0] = nan; h.x[2 * 5 + 1] = inf; h.x[2 * 9] = -inf; h.X[3 * 11 + 2] = nan; h.X[3 * 64] = -inf; h.X[3 * 69 + 1] = inf;
  o = run_loop(h);
  std::printf("hostile non-finite: m %d H %d count %d\n", o.m, o.H, o.best_count);
  CHECK(o.m == 64 && o.H == 1024 && o.best_count == 64, "non-finite: m %d H %d count %d", o.m, o.H, o.best_count);
  const int gone[6] = {0, 5, 9, 11, 64, 69};
  for (int p : gone) CHECK(!o.winner[p] && !o.final_mask[p], "unusable point %d reported", p);
  h.valid.assign(h.n, 0);
  h.valid[1] = h.valid[2] = h.valid[3] = 1;
  o = run_loop(h);
  std::printf("hostile three points: m %d H %d count %d rounds %d\n", o.m, o.H, o.best_count, o.rounds);
  CHECK(o.m == 3 && o.H == 0 && o.best_count == -1 && o.rounds == 0, "three points: m %d H %d", o.m, o.H);
  h.valid[0] = 1;                                         // a fourth flag, on the NaN key-point: still three
  o = run_loop(h);
  CHECK(o.m == 3 && o.H == 0, "flag on a NaN point: m %d", o.m);
  h.valid[4] = 1;
  o = run_loop(h);
  CHECK(o.m == 4 && o.H == 4 && o.best_count == 4, "four points: m %d H %d count %d", o.m, o.H, o.best_count);
}

static bool read_exact(void* dst, size_t bytes, std::FILE* f) { return std::fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "self")) {
    test_count();
    test_sampled();
    test_hostile();
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
      Problem s;
      int32_t head[4];
      if (!read_exact(head, sizeof(head), in) || head[0] < 4 || head[0] > HRP_PNP_POOLED_MAX_N) return 2;
      s.n = head[0]; s.max_hyp = head[1]; s.seed = head[2]; s.min_inliers = head[3];
      s.X.resize(3 * s.n); s.x.resize(2 * s.n); s.pose.resize(6); s.valid.resize(s.n);
      if (!read_exact(&s.thr, 8, in) || !read_exact(s.K, sizeof(s.K), in) || !read_exact(s.X.data(), 8 * s.X.size(), in) ||
          !read_exact(s.x.data(), 8 * s.x.size(), in) || !read_exact(s.pose.data(), 48, in) || !read_exact(s.valid.data(), s.n, in))
        return 2;
      const Outcome o = run_loop(s);
      const int32_t res[4] = {o.m, o.H, o.best_count, o.rounds};
      std::fwrite(res, sizeof(res), 1, out);
      std::fwrite(o.winner.data(), 1, s.n, out);
      std::fwrite(o.final_mask.data(), 1, s.n, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
  }
  std::fprintf(stderr, "usage: %s self | loop <in> <out>\n", argv[0]);
  return 2;
}
