// A stand-alone run of the pose graph's host twins for the pairs -- rdm_pose_graph_pair_covariances_host and
// rdm_pose_graph_pair_terms_host -- on three small chains with chords, meant to be built with the host sanitizers (no GPU is used):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Irdmnet_amd/csrc \
//         tools/pose_graph_pairs_host_check.cpp rdmnet_amd/csrc/pose_graph.hip -x hip rdmnet_amd/csrc/capi.cpp -o pairs_host_check
//   ./pairs_host_check
//
// It checks that Sigma_st of every ordered pair is the transpose of Sigma_ts to 1e-9 of the two nodes' marginals and prints one
// line per system; exit status 0 when all hold.  It is not part of the test suite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/rdmnet_hip.h"

namespace {

struct Rng {  // a small generator of its own, so the systems are the same everywhere
  uint64_t s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(s >> 11) / 9007199254740992.0 - 0.5;
  }
};

// A chain of n nodes with chords: per edge a positive semi-definite 12 x 12 term J^T J, J = [A | -A + small], and a positive
// definite term on every diagonal block.
bool run(int n, const std::vector<std::pair<int, int>>& chords, uint64_t seed) {
  Rng rng{seed};
  std::vector<int64_t> edges;
  for (int i = 0; i + 1 < n; ++i) {
    edges.push_back(i % 2 ? i : i + 1);
    edges.push_back(i % 2 ? i + 1 : i);
  }
  for (const auto& c : chords) {
    edges.push_back(c.first);
    edges.push_back(c.second);
  }
  const int64_t E = static_cast<int64_t>(edges.size() / 2);
  std::vector<double> diag(36 * n, 0.0), off(36 * E, 0.0);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 6; ++k) diag[36 * i + 7 * k] = 1.0 + rng.next();
  for (int64_t e = 0; e < E; ++e) {
    double J[6][12];
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        J[r][c] = 3.0 * rng.next();
        J[r][6 + c] = -J[r][c] + 0.3 * rng.next();
      }
    const int64_t s = edges[2 * e], t = edges[2 * e + 1];
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) {
        double ss = 0.0, st = 0.0, tt = 0.0;
        for (int r = 0; r < 6; ++r) {
          ss += J[r][a] * J[r][b];
          st += J[r][a] * J[r][6 + b];
          tt += J[r][6 + a] * J[r][6 + b];
        }
        diag[36 * s + 6 * a + b] += ss;
        diag[36 * t + 6 * a + b] += tt;
        off[36 * e + 6 * a + b] = st;
      }
  }
  std::vector<int64_t> pairs;
  for (int s = 0; s < n; ++s)
    for (int t = 0; t < n; ++t)
      if (s != t) {
        pairs.push_back(s);
        pairs.push_back(t);
      }
  const int64_t P = static_cast<int64_t>(pairs.size() / 2);
  std::vector<double> cross(36 * P, -7.0), cov(36 * n, -7.0);
  if (rdm_pose_graph_marginals_host(n, E, edges.data(), diag.data(), off.data(), cov.data()) != 0 ||
      rdm_pose_graph_pair_covariances_host(n, E, edges.data(), diag.data(), off.data(), P, pairs.data(), cross.data()) != 0) {
    std::printf("n %d: %s\n", n, rdm_last_error());
    return false;
  }
  auto at = [&](int s, int t) { return cross.data() + 36 * (static_cast<int64_t>(s) * (n - 1) + (t > s ? t - 1 : t)); };
  double worst = 0.0, d2_sum = 0.0;
  int not_fine = 0;
  const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int s = 0; s < n; ++s)
    for (int t = 0; t < n; ++t) {
      if (s == t) continue;
      double big_s = 0.0, big_t = 0.0;
      for (int k = 0; k < 36; ++k) {
        big_s = std::fmax(big_s, std::fabs(cov[36 * s + k]));
        big_t = std::fmax(big_t, std::fabs(cov[36 * t + k]));
      }
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
          const double d = std::fabs(at(s, t)[6 * a + b] - at(t, s)[6 * b + a]);
          if (d > 0.0) worst = std::fmax(worst, d / std::sqrt(big_s * big_t));
        }
      double T[16], out[44];  // a candidate edge 0.1 m off the identity between two poses at the identity
      for (int k = 0; k < 16; ++k) T[k] = eye[k];
      T[3] = 0.1;
      if (rdm_pose_graph_pair_terms_host(eye, eye, T, nullptr, cov.data() + 36 * s, cov.data() + 36 * t, at(s, t), out) != 0) return false;
      if (s != 0 && t != 0) {
        not_fine += out[43] != 0.0;
        d2_sum += out[42];
      }
    }
  std::printf("n %d, %lld edges, %lld pairs: Sigma_st against Sigma_ts^T %.2e, %d pairs not positive definite, mean d2 %.4g\n", n,
              static_cast<long long>(E), static_cast<long long>(P), worst, not_fine, d2_sum / static_cast<double>((n - 1) * (n - 2) + (n < 3)));
  return worst <= 1e-9 && not_fine == 0;
}

}  // namespace

int main() {
  bool ok = run(3, {}, 1);
  ok = run(14, {{3, 6}, {3, 8}, {12, 7}, {12, 9}}, 2) && ok;
  ok = run(46, {{1, 22}, {2, 24}, {3, 26}, {4, 28}, {5, 30}, {6, 32}, {7, 34}, {8, 36}, {9, 38}, {10, 40}, {11, 42}, {12, 44}, {45, 0}}, 3) && ok;
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
