// Pose-graph optimisation on SE(3): damped Gauss-Newton with information-matrix weights and a line process for uncertain
// (loop-closure) edges -- what Open3D's global_optimization does; Open3D is not part of the reference tree, so the definition
// is this project's and is pinned to tests/pose_graph_restatement.py.
//
// A call takes a batch of graphs (concatenated arrays with node / edge offsets).  Everything is float64, there are no float
// atomics and every sum has a fixed order that depends on the graph alone (per-edge terms land in per-edge slots; a node's block
// is the sum over its incidence list in ascending edge order; dot products go per thread in node order, lanes by butterfly,
// wavefronts in order through LDS; a graph's cost is added in edge order by one thread), so a graph's result is the same bits
// alone, in any batch, at any position and from run to run.
//
// Per outer iteration the host launches a fixed sequence: pg_linearize_kernel (one thread per edge), pg_solve_kernel (one
// workgroup per graph: conjugate gradients, matrix-free over the incidence lists, preconditioned by the node blocks (block-Jacobi,
// the default) or, on request, by the exactly factored block tridiagonal part along the odometry chain; or, with the direct solve
// selected, in its place pg_direct_blocks / _factor / _border / _schur / _solve_kernel: a separator of the loop closures is taken out,
// the chain's runs between its nodes are factored exactly and the separator's dense Schur complement is factored in 6 x 6 blocks),
// pg_update_kernel
// (candidate poses), pg_cost_kernel (candidate cost terms), pg_step_kernel (accept / reject, damping, stopping tests) and
// pg_commit_kernel.  All decisions are taken on the device; the host reads one word every kChunk iterations.
//
// Every sum has ONE place: assemble_nodes (node blocks, gradient and the chain's off-diagonal sums, for pg_solve_kernel and
// pg_direct_blocks_kernel), add_block and block_mul (a sum of Hab blocks or their transposes; t = B z or B^T z), precondition<kPre>
// (z = M^-1 r, before the conjugate-gradient loop and in it), direct_run_factor / direct_run_back (a run of the direct solve, and the
// whole chain of rdm_pose_graph_chain_host), dense_factor (the Schur complement's block Cholesky, for pg_direct_solve_kernel and
// pg_marg_separator_kernel).  The fixed order above holds because there is no second copy to edit another way.
//
// rdm_pose_graph_marginals (the marginal covariance of every pose at given poses and weights) is a second, single-pass caller of the
// same pieces: edge_terms with the given weight in the line process's place, assemble_nodes, the direct solve's factors at lambda = 0,
// then a selected inversion (pg_marg_separator_kernel, pg_marg_sweep_kernel) under the same guarantee.  rdm_pose_graph_consistency
// launches exactly that (enqueue_marginals) and then, for a list of pairs of nodes, solves for the columns of H^-1 that the pairs
// need from the same factors (pg_cons_*_kernel): cross covariances, the covariance of a candidate edge's residual and its squared
// Mahalanobis distance, a pair's rows the same bits whatever else the call holds.
#include "common.h"
#include "../../include/rdmnet_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

namespace rdm {
namespace {

constexpr int kBlock = 256;          // threads of every kernel here; pg_solve_kernel: one workgroup of kBlock per graph
constexpr int kWaves = kBlock / kWave;
constexpr int kChunk = 8;            // outer iterations between two reads of the status word
constexpr int64_t kMaxNodes = 65536;    // per graph
constexpr int64_t kMaxEdges = 1048576;  // per graph
constexpr int64_t kMaxTotal = (1ll << 31) - 64;  // nodes / edges of one call
constexpr int kReport = 8;           // doubles per graph in the read-back

// ---- thresholds and factors of the definition ----------------------------------------------------------
constexpr double kSmallSin = 1e-3;        // |sin(angle)| below which (cos > 0) the rotation vector uses the series of asin(s) / s
constexpr double kSmallAngle2 = 1e-2;     // angle^2 below which the inverse right Jacobian's coefficient uses its series
constexpr double kMaxCos = -0.99;         // residual rotations with cos(angle) < kMaxCos (angle > ~171.9 deg) are refused
constexpr double kSymTol = 1e-12;         // |L_ij - L_ji| <= kSymTol * max|L| or the information matrix is refused
constexpr double kLambda0 = 1e-6;         // initial damping
constexpr double kLambdaDown = 0.1;       // after an accepted step
constexpr double kLambdaUp = 10.0;        // after a rejected step
constexpr double kLambdaMin = 1e-12;
constexpr double kLambdaMax = 1e12;       // a rejection above it ends the solve (no decrease is left: stop reason `cost`)

enum : int { STOP_NONE = 0, STOP_GRADIENT = 1, STOP_COST = 2, STOP_MAX_ITERATIONS = 3, STOP_EMPTY = 4 };
enum : int { ST_OK = 0, ST_NONFINITE = 1, ST_ASYMMETRIC = 2, ST_ANGLE = 3, ST_SINGULAR = 4, ST_WEIGHT = 5 };  // (5: the marginals' weights)

struct GraphState {
  double lambda, cost, cost0, cand_cost, grad_max;
  int iterations, pcg_total, stop, status, accepted, done;
};

struct Params {
  double mu;            // line process weight; <= 0: no line process
  double prune;         // edge_prune_threshold
  double gtol, ctol;
  double pcg_tol;
  int max_iterations, pcg_cap;
};

// ---- 3 x 3 helpers (row-major) ---------------------------------------------------------------------------------------------
struct M3 {
  double m[9];
};
struct V3 {
  double v[3];
};

__host__ __device__ inline M3 mul(const M3& a, const M3& b) {  // a b
  M3 c;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c.m[3 * i + j] = (a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j]) + a.m[3 * i + 2] * b.m[6 + j];
  return c;
}
__host__ __device__ inline M3 tmul(const M3& a, const M3& b) {  // a^T b
  M3 c;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c.m[3 * i + j] = (a.m[i] * b.m[j] + a.m[3 + i] * b.m[3 + j]) + a.m[6 + i] * b.m[6 + j];
  return c;
}
__host__ __device__ inline M3 add(const M3& a, const M3& b) {
  M3 c;
  for (int i = 0; i < 9; ++i) c.m[i] = a.m[i] + b.m[i];
  return c;
}
__host__ __device__ inline M3 neg(const M3& a) {
  M3 c;
  for (int i = 0; i < 9; ++i) c.m[i] = -a.m[i];
  return c;
}
__host__ __device__ inline M3 transpose(const M3& a) {
  M3 c;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c.m[3 * i + j] = a.m[3 * j + i];
  return c;
}
__host__ __device__ inline V3 mulv(const M3& a, const V3& x) {  // a x
  V3 y;
  for (int i = 0; i < 3; ++i) y.v[i] = (a.m[3 * i] * x.v[0] + a.m[3 * i + 1] * x.v[1]) + a.m[3 * i + 2] * x.v[2];
  return y;
}
__host__ __device__ inline V3 tmulv(const M3& a, const V3& x) {  // a^T x
  V3 y;
  for (int i = 0; i < 3; ++i) y.v[i] = (a.m[i] * x.v[0] + a.m[3 + i] * x.v[1]) + a.m[6 + i] * x.v[2];
  return y;
}
__host__ __device__ inline M3 skew(const V3& w) {
  M3 s = {{0.0, -w.v[2], w.v[1], w.v[2], 0.0, -w.v[0], -w.v[1], w.v[0], 0.0}};
  return s;
}
__host__ __device__ inline M3 rot_of(const double* X) {  // rotation block of a row-major 4 x 4
  M3 r = {{X[0], X[1], X[2], X[4], X[5], X[6], X[8], X[9], X[10]}};
  return r;
}
__host__ __device__ inline V3 trans_of(const double* X) {
  V3 t = {{X[3], X[7], X[11]}};
  return t;
}

// The residual of an edge: E = T^-1 Xt^-1 Xs with closed-form inverses; w = Log(R_E), v = t_E.  Also R_E, Rst = Rt^T Rs and
// u = Rt^T (ts - tt), which the Jacobians use.  Returns false when the angle is beyond the supported limit.
struct Residual {
  V3 w, v, u;
  M3 Re, Rst;
  double theta2;
};
__host__ __device__ inline bool edge_residual(const double* Xs, const double* Xt, const double* T, Residual& r) {
  const M3 Rs = rot_of(Xs), Rt = rot_of(Xt), RT = rot_of(T);
  const V3 ts = trans_of(Xs), tt = trans_of(Xt), tT = trans_of(T);
  V3 d = {{ts.v[0] - tt.v[0], ts.v[1] - tt.v[1], ts.v[2] - tt.v[2]}};
  r.u = tmulv(Rt, d);
  V3 e = {{r.u.v[0] - tT.v[0], r.u.v[1] - tT.v[1], r.u.v[2] - tT.v[2]}};
  r.v = tmulv(RT, e);
  r.Rst = tmul(Rt, Rs);
  r.Re = tmul(RT, r.Rst);
  const M3& R = r.Re;
  const double a0 = 0.5 * (R.m[7] - R.m[5]), a1 = 0.5 * (R.m[2] - R.m[6]), a2 = 0.5 * (R.m[3] - R.m[1]);  // sin(angle) * axis
  const double s = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  const double c = 0.5 * (((R.m[0] + R.m[4]) + R.m[8]) - 1.0);
  double f, theta;
  if (s < kSmallSin && c > 0.0) {
    const double s2 = s * s;
    f = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0));  // asin(s) / s
    theta = s * f;
  } else {
    theta = atan2(s, c);
    f = s > 0.0 ? theta / s : 0.0;
  }
  r.w.v[0] = a0 * f;
  r.w.v[1] = a1 * f;
  r.w.v[2] = a2 * f;
  r.theta2 = theta * theta;
  return c >= kMaxCos && c == c;
}

// Inverse right Jacobian of SO(3): I + 1/2 [w]x + k(theta) [w]x^2, k = 1/theta^2 - (1 + cos theta) / (2 theta sin theta).
__host__ __device__ inline M3 jr_inv(const V3& w, double theta2) {
  double k;
  if (theta2 < kSmallAngle2) {
    k = 1.0 / 12.0 + theta2 * (1.0 / 720.0 + theta2 * (1.0 / 30240.0 + theta2 * (1.0 / 1209600.0)));
  } else {
    const double theta = sqrt(theta2);
    k = 1.0 / theta2 - (1.0 + cos(theta)) / (2.0 * theta * sin(theta));
  }
  const M3 W = skew(w), W2 = mul(W, W);
  M3 J;
  for (int i = 0; i < 9; ++i) J.m[i] = 0.5 * W.m[i] + k * W2.m[i];
  J.m[0] += 1.0;
  J.m[4] += 1.0;
  J.m[8] += 1.0;
  return J;
}

// q = r^T L r with the symmetrised information matrix (rotation first, then translation); y = L r.
__host__ __device__ inline double quad_form(const double* L, const Residual& r, double* y) {
  const double x[6] = {r.w.v[0], r.w.v[1], r.w.v[2], r.v.v[0], r.v.v[1], r.v.v[2]};
  double q = 0.0;
  for (int i = 0; i < 6; ++i) {
    double a = 0.0;
    for (int j = 0; j < 6; ++j) a += (0.5 * (L[6 * i + j] + L[6 * j + i])) * x[j];
    y[i] = a;
    q += x[i] * a;
  }
  return q;
}

// Line-process weight and cost term of an edge with q = r^T L r.
__host__ __device__ inline double line_weight(double q, double mu, bool uncertain) {
  if (!uncertain || !(mu > 0.0)) return 1.0;
  const double s = mu / (mu + q);
  return s * s;
}
__host__ __device__ inline double cost_term(double q, double l, double mu, bool uncertain) {
  if (!uncertain || !(mu > 0.0)) return q;
  const double sl = sqrt(l) - 1.0;
  return l * q + mu * (sl * sl);
}

__host__ __device__ inline void put_block(double* H, int br, int bc, const M3& a, double l) {  // 3 x 3 block of a row-major 6 x 6
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) H[6 * (3 * br + i) + 3 * bc + j] = l * a.m[3 * i + j];
}

// The non-zero 3 x 3 blocks of an edge's Jacobians (below): A = [[Ja, 0], [0, Ra]], B = [[B11, 0], [B21, B22]].
struct EdgeJacobians {
  M3 Ja, Ra, B11, B21, B22;
};
__host__ __device__ inline EdgeJacobians edge_jacobians(const Residual& r, const double* T) {
  EdgeJacobians j;
  j.Ja = jr_inv(r.w, r.theta2);
  j.Ra = r.Re;
  const M3 RT = rot_of(T);
  j.B11 = neg(mul(j.Ja, transpose(r.Rst)));
  j.B21 = tmul(RT, skew(r.u));
  j.B22 = neg(transpose(RT));
  return j;
}

// Everything one edge contributes: l, its cost term, and (times l) Haa = A^T L A, Hab = A^T L B, Hbb = B^T L B, ga = A^T L r,
// gb = B^T L r (and r itself into r_out, also beyond the limit), where A = d r / d(source perturbation) = [[Jr^-1, 0], [0, R_E]] and B = d r / d(target perturbation) =
// [[-Jr^-1 Rst^T, 0], [R_T^T [u]x, -R_T^T]] (right perturbations X <- X [Exp(dw) | dt]).  Returns false beyond the angle limit.
// given_l: a weight that takes the line process's place (the marginal covariances' per-edge weights).
__host__ __device__ inline bool edge_terms(const double* Xs, const double* Xt, const double* T, const double* L, double mu,
                                           bool uncertain, double* l_out, double* term, double* Haa, double* Hab, double* Hbb,
                                           double* ga, double* gb, double* r_out = nullptr, const double* given_l = nullptr) {
  Residual r;
  const bool ok = edge_residual(Xs, Xt, T, r);
  if (r_out)
    for (int i = 0; i < 3; ++i) {
      r_out[i] = r.w.v[i];
      r_out[3 + i] = r.v.v[i];
    }
  if (!ok) return false;
  double y[6];
  const double q = quad_form(L, r, y);
  const double l = given_l != nullptr ? *given_l : line_weight(q, mu, uncertain);
  *l_out = l;
  *term = cost_term(q, l, mu, uncertain);
  M3 L11, L12, L21, L22;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      L11.m[3 * i + j] = 0.5 * (L[6 * i + j] + L[6 * j + i]);
      L12.m[3 * i + j] = 0.5 * (L[6 * i + 3 + j] + L[6 * (3 + j) + i]);
      L22.m[3 * i + j] = 0.5 * (L[6 * (3 + i) + 3 + j] + L[6 * (3 + j) + 3 + i]);
    }
  L21 = transpose(L12);
  const EdgeJacobians J = edge_jacobians(r, T);
  const M3 &Ja = J.Ja, &Ra = J.Ra, &B11 = J.B11, &B21 = J.B21, &B22 = J.B22;
  // L A and L B by blocks
  const M3 LA11 = mul(L11, Ja), LA12 = mul(L12, Ra), LA21 = mul(L21, Ja), LA22 = mul(L22, Ra);
  const M3 LB11 = add(mul(L11, B11), mul(L12, B21)), LB12 = mul(L12, B22);
  const M3 LB21 = add(mul(L21, B11), mul(L22, B21)), LB22 = mul(L22, B22);
  put_block(Haa, 0, 0, tmul(Ja, LA11), l);
  put_block(Haa, 0, 1, tmul(Ja, LA12), l);
  put_block(Haa, 1, 0, tmul(Ra, LA21), l);
  put_block(Haa, 1, 1, tmul(Ra, LA22), l);
  put_block(Hab, 0, 0, tmul(Ja, LB11), l);
  put_block(Hab, 0, 1, tmul(Ja, LB12), l);
  put_block(Hab, 1, 0, tmul(Ra, LB21), l);
  put_block(Hab, 1, 1, tmul(Ra, LB22), l);
  put_block(Hbb, 0, 0, add(tmul(B11, LB11), tmul(B21, LB21)), l);
  put_block(Hbb, 0, 1, add(tmul(B11, LB12), tmul(B21, LB22)), l);
  put_block(Hbb, 1, 0, tmul(B22, LB21), l);
  put_block(Hbb, 1, 1, tmul(B22, LB22), l);
  const V3 y1 = {{y[0], y[1], y[2]}}, y2 = {{y[3], y[4], y[5]}};
  const V3 ga1 = tmulv(Ja, y1), ga2 = tmulv(Ra, y2);
  const V3 gb1a = tmulv(B11, y1), gb1b = tmulv(B21, y2), gb2 = tmulv(B22, y2);
  for (int i = 0; i < 3; ++i) {
    ga[i] = l * ga1.v[i];
    ga[3 + i] = l * ga2.v[i];
    gb[i] = l * (gb1a.v[i] + gb1b.v[i]);
    gb[3 + i] = l * gb2.v[i];
  }
  return true;
}

// X [Exp(dw) | dt] -> Y (row-major 4 x 4); Exp by Rodrigues with the series of its two coefficients below kSmallAngle2.
__host__ __device__ inline void retract(const double* X, const double* d, double* Y) {
  const V3 w = {{d[0], d[1], d[2]}}, dt = {{d[3], d[4], d[5]}};
  const double t2 = (w.v[0] * w.v[0] + w.v[1] * w.v[1]) + w.v[2] * w.v[2];
  double a, b;  // Exp = I + a [w]x + b [w]x^2
  if (t2 < kSmallAngle2) {
    a = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0 - t2 * (1.0 / 362880.0))));
    b = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0 - t2 * (1.0 / 3628800.0))));
  } else {
    const double t = sqrt(t2);
    a = sin(t) / t;
    const double h = sin(0.5 * t);
    b = 2.0 * h * h / t2;
  }
  const M3 W = skew(w), W2 = mul(W, W);
  M3 Ex;
  for (int i = 0; i < 9; ++i) Ex.m[i] = a * W.m[i] + b * W2.m[i];
  Ex.m[0] += 1.0;
  Ex.m[4] += 1.0;
  Ex.m[8] += 1.0;
  const M3 R = rot_of(X), Rn = mul(R, Ex);
  const V3 rt = mulv(R, dt);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Y[4 * i + j] = Rn.m[3 * i + j];
    Y[4 * i + 3] = X[4 * i + 3] + rt.v[i];
  }
  Y[12] = 0.0;
  Y[13] = 0.0;
  Y[14] = 0.0;
  Y[15] = 1.0;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------

struct Graphs {            // device arrays of the call
  const int* node_off;     // [G + 1]
  const int* edge_off;     // [G + 1]
  const int* edge_graph;   // [E]
  const int* node_graph;   // [N]
  const int* es;           // [E] global source node
  const int* et;           // [E] global target node
  const uint8_t* uncertain;  // [E] or null
  const int* inc_off;      // [N + 1] incidence lists: entries 2 * edge + side (0: the node is the source), ascending
  const int* inc;          // [2 E]
};

// A workgroup has nothing to do for its graph g: the input check refused the call, or the graph is done.  (The kernels that map
// threads to edges, nodes, runs or couplings test *bad before they look their graph up.)
__device__ __forceinline__ bool skip(const GraphState* gs, int g, const int* bad) { return *bad != 0 || gs[g].done; }
// Graph g ends with a failure, by a whole workgroup.
__device__ __forceinline__ void end_graph(GraphState* gs, int g, int status) {
  if (threadIdx.x == 0) {
    gs[g].status = status;
    gs[g].done = 1;
  }
}

// Inputs: every entry finite, information matrices symmetric.  One flag for the call, and the cause in the status of the graph that
// holds the entry (after pg_init_kernel).
__global__ __launch_bounds__(kBlock) void pg_check_kernel(Graphs gr, const double* __restrict__ nodes, int n,
                                                          const double* __restrict__ T, const double* __restrict__ L, int e,
                                                          GraphState* __restrict__ gs, int* __restrict__ bad) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  int b = 0;
  if (i < n) {
    const double* X = nodes + 16 * i;
    for (int k = 0; k < 16; ++k)
      if (!isfinite(X[k])) b = ST_NONFINITE;
    if (b != 0) gs[gr.node_graph[i]].status = b;  // (any writer's value names a cause that is present)
  }
  const int b_node = b;
  b = 0;
  if (i < e) {
    const double* X = T + 16 * i;
    for (int k = 0; k < 16; ++k)
      if (!isfinite(X[k])) b = ST_NONFINITE;
    const double* M = L + 36 * i;
    double big = 0.0;
    for (int k = 0; k < 36; ++k) {
      if (!isfinite(M[k])) b = ST_NONFINITE;
      big = fmax(big, fabs(M[k]));
    }
    if (b == 0)
      for (int r = 0; r < 6; ++r)
        for (int c = r + 1; c < 6; ++c)
          if (fabs(M[6 * r + c] - M[6 * c + r]) > kSymTol * big) b = ST_ASYMMETRIC;
    if (b != 0) gs[gr.edge_graph[i]].status = b;
  }
  if (b_node != 0 || b != 0) *bad = b_node != 0 ? b_node : b;
}

__global__ __launch_bounds__(kBlock) void pg_init_kernel(const double* __restrict__ nodes, int n, double* __restrict__ X,
                                                         double* __restrict__ Xc, GraphState* __restrict__ gs, int g,
                                                         const int* __restrict__ node_off, const int* __restrict__ edge_off) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < 16ll * n) {
    X[i] = nodes[i];
    Xc[i] = nodes[i];
  }
  if (i < g) {
    GraphState s;
    s.lambda = kLambda0;
    s.cost = s.cost0 = s.cand_cost = s.grad_max = 0.0;
    s.iterations = s.pcg_total = s.accepted = 0;
    s.status = ST_OK;
    const bool empty = node_off[i + 1] == node_off[i] || edge_off[i + 1] == edge_off[i];
    s.stop = empty ? STOP_EMPTY : STOP_NONE;
    s.done = empty ? 1 : 0;
    gs[i] = s;
  }
}

// One thread per edge: weight, cost term and the weighted blocks at the current poses, each into the edge's own slot.
__global__ __launch_bounds__(kBlock) void pg_linearize_kernel(Graphs gr, int e_total, const double* __restrict__ X,
                                                              const double* __restrict__ T, const double* __restrict__ L,
                                                              Params p, const GraphState* __restrict__ gs,
                                                              double* __restrict__ lw, double* __restrict__ Haa,
                                                              double* __restrict__ Hab, double* __restrict__ Hbb,
                                                              double* __restrict__ ga, double* __restrict__ gb,
                                                              const int* __restrict__ bad) {
  const long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= e_total || *bad != 0) return;
  if (gs[gr.edge_graph[e]].done) return;
  double l, term;
  const bool unc = gr.uncertain != nullptr && gr.uncertain[e] != 0;
  // (the angle limit was checked when these poses were a candidate, or by the initial cost)
  edge_terms(X + 16ll * gr.es[e], X + 16ll * gr.et[e], T + 16 * e, L + 36 * e, p.mu, unc, &l, &term, Haa + 36 * e, Hab + 36 * e,
             Hbb + 36 * e, ga + 6 * e, gb + 6 * e);
  lw[e] = l;
}

// One thread per edge: the cost term at poses Y (+inf beyond the angle limit) and the weight there.  force: also for graphs that
// are done (the weights at the final poses).
__global__ __launch_bounds__(kBlock) void pg_cost_kernel(Graphs gr, int e_total, const double* __restrict__ Y,
                                                         const double* __restrict__ T, const double* __restrict__ L, Params p,
                                                         const GraphState* __restrict__ gs, int force, double* __restrict__ term,
                                                         double* __restrict__ lw, const int* __restrict__ bad) {
  const long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= e_total || *bad != 0) return;
  if (!force && gs[gr.edge_graph[e]].done) return;
  const bool unc = gr.uncertain != nullptr && gr.uncertain[e] != 0;
  Residual r;
  double y[6];
  if (!edge_residual(Y + 16ll * gr.es[e], Y + 16ll * gr.et[e], T + 16 * e, r)) {
    term[e] = INFINITY;
    if (lw) lw[e] = 1.0;
    return;
  }
  const double q = quad_form(L + 36 * e, r, y);
  const double l = line_weight(q, p.mu, unc);
  term[e] = cost_term(q, l, p.mu, unc);
  if (lw) lw[e] = l;
}

// Sum of one value per thread over the workgroup, the same in every thread: lanes by butterfly, wavefronts in order.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();  // (the previous use of red is over)
  if (lane_id() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < kWaves; ++w) s += red[w];
  return s;
}
__device__ __forceinline__ double block_max(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if (lane_id() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < kWaves; ++w) s = fmax(s, red[w]);
  return s;
}

__host__ __device__ __forceinline__ bool finite_value(double v) {
#ifdef __HIP_DEVICE_COMPILE__
  return isfinite(v);
#else
  return std::isfinite(v);
#endif
}
// In-place Cholesky of a symmetric 6 x 6 (lower triangle of a[36] is read and replaced by the factor).  false: not positive.
__host__ __device__ __forceinline__ bool cholesky6(double* a) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = a[6 * j + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= a[6 * j + k] * a[6 * j + k];
    if (!(d > 0.0) || !finite_value(d)) {
      ok = false;
      d = 1.0;
    }
    const double s = sqrt(d);
    a[6 * j + j] = s;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = a[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= a[6 * i + k] * a[6 * j + k];
      a[6 * i + j] = v / s;
    }
  }
  return ok;
}
// z = (F F^T)^-1 r, F the lower factor stored as 21 values in row order
__device__ __forceinline__ void chol_solve6(const double* __restrict__ f, const double* r, double* z) {
  double c[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) c[k] = f[k];
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= c[i * (i + 1) / 2 + k] * y[k];
    y[i] = v / c[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= c[k * (k + 1) / 2 + i] * z[k];
    z[i] = v / c[i * (i + 1) / 2 + i];
  }
}

// The two operations on an edge's 6 x 6 block Hab, whose rows are the edge's source: every sum over such blocks goes through them, so
// that it has one order and one shape wherever it is formed.
// acc += H, or acc += H^T for the end of the edge that is its target.
__host__ __device__ __forceinline__ void add_block(double* acc, const double* H, bool transposed) {
  if (transposed) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[6 * r + c] += H[6 * c + r];
  } else {
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] += H[k];
  }
}
// t = B z, or t = B^T z: every entry from 0.0 in ascending k.  The caller adds or subtracts t as a step of its own.
__host__ __device__ __forceinline__ void block_mul(const double* B, const double* z, bool transposed, double* t) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) a += (transposed ? B[6 * k + i] : B[6 * i + k]) * z[k];
    t[i] = a;
  }
}
// r <- r - B z and r <- r - B^T z (r is neither B nor z)
__host__ __device__ __forceinline__ void dense_sub_mul(const double* b, const double* z, double* r, bool transposed) {
  double t[6];
  block_mul(b, z, transposed, t);
#pragma unroll
  for (int i = 0; i < 6; ++i) r[i] -= t[i];
}

// ---- the odometry-chain preconditioner -----------------------------------------------------------------
// M is block tridiagonal over the free nodes 1 .. n - 1: the damped node blocks on the diagonal, and between nodes i - 1 and i the
// sum of the Hab blocks of the edges that join the two.  M = L L^T by a block Cholesky along the chain; kept per node are
// G_i = L_ii^-1 (lower triangle, 21 values in row order, in the block-Jacobi factor's slot) and W_i = G_i L_{i,i-1} (6 x 6).
// z = M^-1 r in four steps: c_i = G_i r_i (a thread per node), y_i = c_i - W_i y_{i-1} (forward sweep), q_i = y_i - W_{i+1}^T q_{i+1}
// (backward sweep; q_i = L_ii^T z_i, so the same W serves both sweeps), z_i = G_i^T q_i (a thread per node).

// One node of the factorisation.  d: the node's damped block (its lower triangle is read); m: M_{i,i-1}, or null at the chain's first
// node; gp: G_{i-1}.  -> g = G_i and x = L_{i,i-1} = M_{i,i-1} G_{i-1}^T (zeros without m).  false: a pivot is not positive.
__host__ __device__ __forceinline__ bool chain_factor_node(const double* d, const double* m, const double* gp, double* g, double* x) {
  double s[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) s[k] = d[k];
  if (m != nullptr) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double mr[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) mr[k] = m[6 * r + k];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k <= c; ++k) a += mr[k] * gp[c * (c + 1) / 2 + k];
        x[6 * r + c] = a;
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        double a = s[6 * r + c];
#pragma unroll
        for (int k = 0; k < 6; ++k) a -= x[6 * r + k] * x[6 * c + k];
        s[6 * r + c] = a;
      }
  } else {
#pragma unroll
    for (int k = 0; k < 36; ++k) x[k] = 0.0;
  }
  const bool ok = cholesky6(s);
#pragma unroll
  for (int j = 0; j < 6; ++j) {  // G = L^-1, column by column
    g[j * (j + 1) / 2 + j] = 1.0 / s[6 * j + j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double a = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) a += s[6 * i + k] * g[k * (k + 1) / 2 + j];
      g[i * (i + 1) / 2 + j] = -a / s[6 * i + i];
    }
  }
  return ok;
}
// w = G x (6 x 6; w may be x)
__host__ __device__ __forceinline__ void chain_w(const double* g, const double* x, double* w) {
  double t[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) t[k] = x[k];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k <= r; ++k) a += g[r * (r + 1) / 2 + k] * t[6 * k + c];
      w[6 * r + c] = a;
    }
}
// c = G r and z = G^T q
__host__ __device__ __forceinline__ void chain_g_mul(const double* g, const double* r, double* c) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k <= i; ++k) a += g[i * (i + 1) / 2 + k] * r[k];
    c[i] = a;
  }
}
__host__ __device__ __forceinline__ void chain_gt_mul(const double* g, const double* q, double* z) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double a = 0.0;
#pragma unroll
    for (int i = k; i < 6; ++i) a += g[i * (i + 1) / 2 + k] * q[i];
    z[k] = a;
  }
}
// One row of a sweep step: c - w . y, the six products added as three pairs (a short dependent chain, a fixed order).
__host__ __device__ __forceinline__ double chain_row(double c, const double* w, const double* y) {
  return c - (((w[0] * y[0] + w[1] * y[1]) + (w[2] * y[2] + w[3] * y[3])) + (w[4] * y[4] + w[5] * y[5]));
}
// M_{node, node-1}: the sum of the blocks of the edges that join the two, in edge order (rows: node).
__host__ __device__ __forceinline__ void chain_off_block(const int* __restrict__ es, const int* __restrict__ et,
                                                         const int* __restrict__ inc_off, const int* __restrict__ inc,
                                                         const double* __restrict__ Hab, long long node, double* off) {
#pragma unroll
  for (int k = 0; k < 36; ++k) off[k] = 0.0;
  for (int q = inc_off[node]; q < inc_off[node + 1]; ++q) {
    const int code = inc[q];
    const long long e = code >> 1;
    const long long other = (code & 1) ? es[e] : et[e];
    if (other == node - 1) add_block(off, Hab + 36 * e, code & 1);
  }
}

__device__ __forceinline__ double read_lane(double v, int lane) {  // lane: a constant
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// The two sweeps of one graph, in place on its rows of zv, by ONE wavefront (all 64 lanes call it).  Wg, zg: the graph's rows of
// W [n, 36] and zv [n, 6].  Lane 8 k + r holds row r (sweep back: column r of the next node's W) of the k-th node of a group of
// eight consecutive nodes; the eight steps of a group run one after the other, every lane evaluating chain_row and the step's
// six lanes handing their results to all lanes through v_readlane (scalar registers: no LDS round trip on the dependent path);
// the next group's rows are loaded before the current group's steps, so their latency lies under about eight steps.  A lane
// reads back in the second sweep only what it wrote itself in the first.
__device__ __forceinline__ void chain_sweeps(const double* __restrict__ Wg, double* __restrict__ zg, int n) {
  const int lane = threadIdx.x & 63, k = lane >> 3, r = lane & 7;
  const int m = n - 1, groups = (m + 7) >> 3;  // free nodes j = 0 .. m - 1 are the graph's nodes j + 1
  if (groups == 0) return;
  double w[6], c, wn[6], cn = 0.0, y[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) y[q] = wn[q] = 0.0;
  // (every lane loads from an address inside the graph, clamped, and lanes without a row take zeros when the group becomes the
  // current one: no branch around the loads and no use of them before the steps they lie under)
  const int rc = r < 6 ? r : 5;
  auto load_forward = [&](int g, double* ww, double& cc) {
    const int j = 8 * g + k;
    const long long node = (j < m ? j : m - 1) + 1;
#pragma unroll
    for (int q = 0; q < 6; ++q) ww[q] = Wg[36 * node + 6 * rc + q];
    cc = zg[6 * node + rc];
  };
  auto load_backward = [&](int g, double* ww, double& cc) {
    const int j = 8 * g + k;
    const long long node = (j < m ? j : m - 1) + 1, next = node < m ? node + 1 : m;
#pragma unroll
    for (int q = 0; q < 6; ++q) ww[q] = Wg[36 * next + 6 * q + rc];
    cc = zg[6 * node + rc];
  };
  auto take = [&](int g, bool forward) {  // group g becomes the current one
    const int j = 8 * g + k;
    const bool on = r < 6 && j >= 0 && j < m, has_w = on && (forward || j + 1 < m);
#pragma unroll
    for (int q = 0; q < 6; ++q) w[q] = has_w ? wn[q] : 0.0;
    c = on ? cn : 0.0;
  };
  auto steps = [&](bool forward) -> double {  // the eight nodes of a group; -> this lane's own entry
    double mine = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int kk = forward ? s : 7 - s;
      const double t = chain_row(c, w, y);
      if (k == kk) mine = t;
#pragma unroll
      for (int q = 0; q < 6; ++q) y[q] = read_lane(t, 8 * kk + q);
    }
    return mine;
  };
  load_forward(0, wn, cn);
  take(0, true);
  for (int g = 0; g < groups; ++g) {
    if (g + 1 < groups) load_forward(g + 1, wn, cn);
    const double mine = steps(true);
    const int j = 8 * g + k;
    if (r < 6 && j < m) zg[6ll * (j + 1) + r] = mine;
    take(g + 1, true);
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) y[q] = 0.0;
  load_backward(groups - 1, wn, cn);
  take(groups - 1, false);
  for (int g = groups - 1; g >= 0; --g) {
    if (g > 0) load_backward(g - 1, wn, cn);
    const double mine = steps(false);
    const int j = 8 * g + k;
    if (r < 6 && j < m) zg[6ll * (j + 1) + r] = mine;
    take(g - 1, false);
  }
}

// The chain preconditioner after c_i = G_i r_i was written to zv by the nodes' threads: the sweeps, then z_i = G_i^T q_i into zv.
// -> this thread's part of r^T z (its nodes in order).
__device__ __forceinline__ double chain_finish(const double* __restrict__ F, const double* __restrict__ Wc, const double* rv,
                                               double* zv, int n0, int n) {
  __syncthreads();
  if (threadIdx.x < kWave) chain_sweeps(Wc + 36ll * n0, zv + 6ll * n0, n);
  __syncthreads();
  double part = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) {
    if (i == 0) continue;
    const long long node = n0 + i;
    double q[6], z[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = zv[6 * node + k];
    chain_gt_mul(F + 21 * node, q, z);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      zv[6 * node + k] = z[k];
      part += rv[6 * node + k] * z[k];
    }
  }
  return part;
}

enum : int { PRE_BLOCK_JACOBI = 0, PRE_CHAIN = 1 };
enum : int { SOLVER_PCG = 0, SOLVER_DIRECT = 1 };

// The node assembly, for the calling thread's nodes tid, tid + kBlock, ... of the graph at n0 with n nodes: D = the sum of the node's
// Haa / Hbb blocks and b = the sum of its ga / gb over the incidence list in ascending order (zeros for the fixed node 0), written with
// x = 0 and r = -b; with kOff, the chain's off-diagonal sum M_{i,i-1} into Wc by a second pass over the list (zeros for i <= 1).
// -> the thread's gradient maximum.
template <bool kOff>
__device__ __forceinline__ double assemble_nodes(const Graphs& gr, int n0, int n, const double* __restrict__ Haa,
                                                 const double* __restrict__ Hab, const double* __restrict__ Hbb,
                                                 const double* __restrict__ ga, const double* __restrict__ gb, double* __restrict__ D,
                                                 double* __restrict__ bv, double* __restrict__ xv, double* __restrict__ rv,
                                                 double* __restrict__ Wc) {
  double gmax = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) {
    const long long node = n0 + i;
    double d[36], b[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) d[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = 0.0;
    if (i > 0) {
      for (int q = gr.inc_off[node]; q < gr.inc_off[node + 1]; ++q) {
        const int code = gr.inc[q];
        const long long e = code >> 1;
        const double* H = (code & 1) ? Hbb + 36 * e : Haa + 36 * e;
        const double* v = (code & 1) ? gb + 6 * e : ga + 6 * e;
#pragma unroll
        for (int k = 0; k < 36; ++k) d[k] += H[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] += v[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 36; ++k) D[36 * node + k] = d[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      bv[6 * node + k] = b[k];
      gmax = fmax(gmax, fabs(2.0 * b[k]));  // the gradient of F is 2 b
      xv[6 * node + k] = 0.0;
      rv[6 * node + k] = -b[k];
    }
    if constexpr (kOff) {
      if (i > 1) {
        chain_off_block(gr.es, gr.et, gr.inc_off, gr.inc, Hab, node, d);
      } else {
#pragma unroll
        for (int k = 0; k < 36; ++k) d[k] = 0.0;
      }
#pragma unroll
      for (int k = 0; k < 36; ++k) Wc[36 * node + k] = d[k];
    }
  }
  return gmax;
}

// The gradient test on the workgroup's gradient maximum.  -> it ends the graph (the same in every thread).
__device__ __forceinline__ bool gradient_stop(GraphState* gs, int g, double gmax, double gtol) {
  if (threadIdx.x == 0) {
    gs[g].grad_max = gmax;
    if (gmax <= gtol) {
      gs[g].stop = STOP_GRADIENT;
      gs[g].done = 1;
    }
  }
  return gmax <= gtol;
}

// z = M^-1 r for the calling thread's nodes, into zv (zeros for node 0).  kPre 0: the nodes' factored blocks; 1: c = G r per node, then
// the sweeps and z = G^T q by chain_finish (whose barriers every thread of the workgroup passes).  -> this thread's part of r^T z, its
// nodes in order.
template <int kPre>
__device__ __forceinline__ double precondition(const double* __restrict__ F, const double* __restrict__ Wc, const double* rv, double* zv,
                                               int n0, int n) {
  double part = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) {
    const long long node = n0 + i;
    double r[6], z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) r[k] = rv[6 * node + k];
    if constexpr (kPre == PRE_CHAIN) {
      if (i > 0) chain_g_mul(F + 21 * node, r, z);
    } else {
      if (i > 0) chol_solve6(F + 21 * node, r, z);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      zv[6 * node + k] = z[k];
      if constexpr (kPre != PRE_CHAIN) {
        if (i > 0) part += r[k] * z[k];
      }
    }
  }
  if constexpr (kPre == PRE_CHAIN) part = chain_finish(F, Wc, rv, zv, n0, n);
  return part;
}

// One workgroup per graph: node blocks and gradient in incidence order, the gradient test, the preconditioner's factors (kPre 0:
// damped block-Jacobi; 1: the odometry chain, factored along the chain by thread 0 from blocks that 72 threads stage in LDS one
// node ahead), then preconditioned conjugate gradients on (H + lambda blockdiag(H)) x = -b with a matrix-free product.  A thread
// owns nodes tid, tid + kBlock, ...; node 0 is fixed (its rows are left out: x_0 = 0).  D [N, 36], F [N, 21], b, x, r, z, pv, Ap
// [N, 6] are global, and so is Wc [N, 36] (kPre 1 only; else null).
template <int kPre>
__global__ __launch_bounds__(kBlock) void pg_solve_kernel(Graphs gr, Params p, GraphState* __restrict__ gs,
                                                          const double* __restrict__ Haa, const double* __restrict__ Hab,
                                                          const double* __restrict__ Hbb, const double* __restrict__ ga,
                                                          const double* __restrict__ gb, double* __restrict__ D,
                                                          double* __restrict__ F, double* __restrict__ bv, double* __restrict__ xv,
                                                          double* __restrict__ rv, double* __restrict__ zv, double* __restrict__ pv,
                                                          const int* __restrict__ bad, double* __restrict__ Wc) {
  __shared__ double red[kWaves];
  __shared__ int fail;
  const int g = blockIdx.x;
  if (skip(gs, g, bad)) return;  // (uniform over the workgroup)
  const int n0 = gr.node_off[g], n = gr.node_off[g + 1] - n0;
  const double lambda = gs[g].lambda;
  if (threadIdx.x == 0) fail = 0;
  __syncthreads();
  // 1. blocks, gradient, factors
  double gmax = assemble_nodes<kPre == PRE_CHAIN>(gr, n0, n, Haa, Hab, Hbb, ga, gb, D, bv, xv, rv, Wc);
  if constexpr (kPre == PRE_BLOCK_JACOBI) {
    for (int i = threadIdx.x; i < n; i += kBlock) {
      if (i == 0) continue;
      const long long node = n0 + i;
      double d[36];  // (the thread's own writes of D)
#pragma unroll
      for (int k = 0; k < 36; ++k) d[k] = D[36 * node + k];
#pragma unroll
      for (int k = 0; k < 36; ++k) d[k] *= 1.0 + lambda;
      if (!cholesky6(d)) fail = 1;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) F[21 * node + r * (r + 1) / 2 + c] = d[6 * r + c];
    }
  }
  gmax = block_max(gmax, red);
  if (fail) {  // (block_max's barriers order the writes of `fail`)
    end_graph(gs, g, ST_SINGULAR);
    return;
  }
  if (gradient_stop(gs, g, gmax, p.gtol)) return;
  if constexpr (kPre == PRE_CHAIN) {
    // the chain's factors: node after node by thread 0; threads 0 .. 71 fetch the next node's damped block and M_{i,i-1} meanwhile
    __shared__ double stage[2][72];
    const int t = threadIdx.x;
    auto fetch = [&](int i) { return t < 36 ? (1.0 + lambda) * D[36ll * (n0 + i) + t] : Wc[36ll * (n0 + i) + t - 36]; };
    if (t < 72 && n > 1) stage[0][t] = fetch(1);
    double gp[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) gp[k] = 0.0;
    for (int i = 1; i < n; ++i) {
      const int buf = (i - 1) & 1;
      const bool more = t < 72 && i + 1 < n;
      double next = 0.0;
      if (more) next = fetch(i + 1);
      __syncthreads();  // stage[buf] is written; stage[buf ^ 1] is read no more
      if (t == 0) {
        const long long node = n0 + i;
        double gi[21], x[36];
        if (!chain_factor_node(stage[buf], i > 1 ? stage[buf] + 36 : nullptr, gp, gi, x)) fail = 1;
#pragma unroll
        for (int k = 0; k < 21; ++k) F[21 * node + k] = gp[k] = gi[k];
#pragma unroll
        for (int k = 0; k < 36; ++k) Wc[36 * node + k] = x[k];
      }
      if (more) stage[buf ^ 1][t] = next;
    }
    __syncthreads();
    if (fail) {
      end_graph(gs, g, ST_SINGULAR);
      return;
    }
    for (int i = threadIdx.x; i < n; i += kBlock)
      if (i > 1) chain_w(F + 21ll * (n0 + i), Wc + 36ll * (n0 + i), Wc + 36ll * (n0 + i));
  }
  // 2. z = M^-1 r, pv = z, rz
  double part = precondition<kPre>(F, Wc, rv, zv, n0, n);
  for (int i = threadIdx.x; i < n; i += kBlock)
#pragma unroll
    for (int k = 0; k < 6; ++k) pv[6ll * (n0 + i) + k] = zv[6ll * (n0 + i) + k];
  double rz = block_sum(part, red);
  const double rz0 = rz;
  int it = 0;
  // 3. iterations (every condition below is uniform over the workgroup: the sums are the same value in every thread)
  while (it < p.pcg_cap && rz > 0.0 && sqrt(rz) > p.pcg_tol * sqrt(rz0)) {
    // Ap into zv (z is rebuilt after the update), pAp
    part = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const long long node = n0 + i;
      double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (i > 0) {
        double x[6], t[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = pv[6 * node + k];
        block_mul(D + 36 * node, x, false, t);
#pragma unroll
        for (int r = 0; r < 6; ++r) y[r] = (1.0 + lambda) * t[r];
        for (int q = gr.inc_off[node]; q < gr.inc_off[node + 1]; ++q) {
          const int code = gr.inc[q];
          const long long e = code >> 1;
          if (code & 1) {  // this node is the target: Hab^T p_source
            block_mul(Hab + 36 * e, pv + 6ll * gr.es[e], true, t);
          } else {
            block_mul(Hab + 36 * e, pv + 6ll * gr.et[e], false, t);
          }
#pragma unroll
          for (int r = 0; r < 6; ++r) y[r] += t[r];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) part += x[k] * y[k];
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) zv[6 * node + k] = y[k];
    }
    const double pAp = block_sum(part, red);
    if (!(pAp > 0.0)) break;
    const double alpha = rz / pAp;
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const long long node = n0 + i;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        xv[6 * node + k] += alpha * pv[6 * node + k];
        rv[6 * node + k] = rv[6 * node + k] - alpha * zv[6 * node + k];
      }
    }
    const double rz_new = block_sum(precondition<kPre>(F, Wc, rv, zv, n0, n), red);
    const double beta = rz_new / rz;
    rz = rz_new;
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const long long node = n0 + i;
#pragma unroll
      for (int k = 0; k < 6; ++k) pv[6 * node + k] = zv[6 * node + k] + beta * pv[6 * node + k];
    }
    __syncthreads();  // pv of other threads is read by the next product
    ++it;
  }
  if (threadIdx.x == 0) gs[g].pcg_total += it;
}

// ---- the direct solve ----------------------------------------------------------------------------------
// The same system without conjugate gradients.  A separator S (a vertex cover of the off-chain edges, chosen by the host) is taken
// out; what is left falls into runs of consecutive nodes that are block tridiagonal and do not couple.  With A_II = L L^T along the
// runs (chain_factor_node): Y = L^-1 A_IS, C = A_SS - Y^T Y = L_S L_S^T (dense, in 6 x 6 blocks), y = L^-1 r_I,
// x_S = C^-1 (r_S - Y^T y), x_I = L^-T (y - Y x_S).  The functions below are one work item each and are compiled for the device
// (the kernels map threads to items) and for the host (rdm_pose_graph_direct_host runs the items in order).
constexpr int kMaxSeparator = 256;  // separator nodes per graph: the dense factor is [6 kMaxSeparator]^2

struct Direct {             // the host-built plan of a call (global node, separator, run and coupling numbers) and its arrays
  const int* sep_off;       // [G + 1] a graph's separator nodes
  const int* sep_node;      // [S] ascending inside a graph
  const int* run_off;       // [G + 1] a graph's runs
  const int* run_begin;     // [R] first node
  const int* run_len;       // [R]
  const int* run_graph;     // [R]
  const int* cpl_off;       // [R + 1] a run's couplings (run, separator node), ascending separator
  const int* cpl_sep;       // [K]
  const int* cpl_run;       // [K]
  const int* cpl_pos;       // [K] first position of the run that an edge joins to the separator node
  const int* cpl_y;         // [K] first 6 x 6 block of the coupling's part of Y (positions cpl_pos .. the run's end)
  const int* ent_off;       // [K + 1] a coupling's edges, by position, then ascending
  const int* ent_pos;       // [A]
  const int* ent_code;      // [A] 2 * edge + side of the separator node (0: it is the source)
  const int* sc_off;        // [S + 1] a separator node's couplings, ascending run
  const int* sc;            // [K]
  const long long* c_off;   // [G + 1] a graph's first block of C ([s, s] blocks, row-major; the lower triangle is used)
  const long long* item_off;  // [G + 1] a graph's Schur items: s * s blocks and s right-hand sides
  double* C;
  double* Y;
  int* fail;                // [G] a pivot was not positive
};

struct DirectSystem {       // the system: D, Hab and the incidence lists give A; rv the right-hand side
  const int *es, *et, *inc_off, *inc;
  const double *D, *Hab, *rv;
  double *F, *Wc, *zv, *xv;  // G [N, 21], W [N, 36] (on entry: the chain's off-diagonal sums), y [N, 6], x [N, 6]
};

// One run: the factors G_i and W_i = G_i L_{i,i-1} along it, and y = L^-1 r on its rows of zv.  false: a pivot is not positive.  With
// failed_at (the host's callers that name the node) the run ends at that position, which is written there; without it (the
// kernel) the run is factored to its end.
__host__ __device__ inline bool direct_run_factor(const Direct& dp, const DirectSystem& sy, double dscale, int run,
                                                  int* failed_at = nullptr) {
  const long long first = dp.run_begin[run];
  const int len = dp.run_len[run];
  bool ok = true;
  double gp[21], y[6];
#pragma unroll
  for (int k = 0; k < 21; ++k) gp[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) y[k] = 0.0;
  for (int i = 0; i < len; ++i) {
    const long long node = first + i;
    double d[36], m[36], gi[21], x[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) {
      d[k] = dscale * sy.D[36 * node + k];
      m[k] = sy.Wc[36 * node + k];
    }
    if (!chain_factor_node(d, i > 0 ? m : nullptr, gp, gi, x)) {
      ok = false;
      if (failed_at != nullptr) {
        *failed_at = i;
        return false;
      }
    }
    chain_w(gi, x, x);
    double r[6], c[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) r[k] = sy.rv[6 * node + k];
    chain_g_mul(gi, r, c);
#pragma unroll
    for (int k = 0; k < 6; ++k) r[k] = chain_row(c[k], x + 6 * k, y);
#pragma unroll
    for (int k = 0; k < 6; ++k) sy.zv[6 * node + k] = y[k] = r[k];
#pragma unroll
    for (int k = 0; k < 21; ++k) sy.F[21 * node + k] = gp[k] = gi[k];
#pragma unroll
    for (int k = 0; k < 36; ++k) sy.Wc[36 * node + k] = x[k];
  }
  return ok;
}

// One column (of the separator node's six) of one coupling: the run's forward sweep from the coupling's first position.
__host__ __device__ inline void direct_border_column(const Direct& dp, const DirectSystem& sy, int cpl, int col) {
  const int run = dp.cpl_run[cpl], p = dp.cpl_pos[cpl], len = dp.run_len[run];
  const long long first = dp.run_begin[run];
  double* Yc = dp.Y + 36ll * dp.cpl_y[cpl];
  int q = dp.ent_off[cpl];
  const int qe = dp.ent_off[cpl + 1];
  double y[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) y[k] = 0.0;
  for (int pos = p; pos < len; ++pos) {
    const long long node = first + pos;
    double a[6], c[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) a[k] = 0.0;
    for (; q < qe && dp.ent_pos[q] == pos; ++q) {  // block (node, separator node) of A, this column
      const int code = dp.ent_code[q];
      const double* H = sy.Hab + 36ll * (code >> 1);
      if (code & 1) {  // the separator node is the target: the rows of Hab are this node's
#pragma unroll
        for (int r = 0; r < 6; ++r) a[r] += H[6 * r + col];
      } else {
#pragma unroll
        for (int r = 0; r < 6; ++r) a[r] += H[6 * col + r];
      }
    }
    chain_g_mul(sy.F + 21 * node, a, c);
#pragma unroll
    for (int r = 0; r < 6; ++r) a[r] = chain_row(c[r], sy.Wc + 36 * node + 6 * r, y);
#pragma unroll
    for (int r = 0; r < 6; ++r) Yc[36ll * (pos - p) + 6 * r + col] = y[r] = a[r];
  }
}

// Block (u, v), v <= u, of C = A_SS - Y^T Y of graph g (s separator nodes): the nodes' own block or the edges that join them in
// edge order, then the runs both touch in ascending order, every position both columns cover, one position after the other.
__host__ __device__ inline void direct_schur_block(const Direct& dp, const DirectSystem& sy, double dscale, int g, int s, int u, int v) {
  const int su = dp.sep_off[g] + u, sv = dp.sep_off[g] + v;
  const long long a = dp.sep_node[su], b = dp.sep_node[sv];
  double acc[36];
  if (u == v) {
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = dscale * sy.D[36 * a + k];
  } else {
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
    for (int q = sy.inc_off[a]; q < sy.inc_off[a + 1]; ++q) {
      const int code = sy.inc[q];
      const long long e = code >> 1;
      if (((code & 1) ? sy.es[e] : sy.et[e]) == b) add_block(acc, sy.Hab + 36 * e, code & 1);
    }
  }
  int i = dp.sc_off[su], j = dp.sc_off[sv];
  const int ie = dp.sc_off[su + 1], je = dp.sc_off[sv + 1];
  while (i < ie && j < je) {
    const int ci = dp.sc[i], cj = dp.sc[j], ri = dp.cpl_run[ci], rj = dp.cpl_run[cj];
    if (ri < rj) {
      ++i;
    } else if (rj < ri) {
      ++j;
    } else {
      const int pi = dp.cpl_pos[ci], pj = dp.cpl_pos[cj], p = pi > pj ? pi : pj, len = dp.run_len[ri];
      const double* Yu = dp.Y + 36ll * (dp.cpl_y[ci] + (p - pi));
      const double* Yv = dp.Y + 36ll * (dp.cpl_y[cj] + (p - pj));
      for (int pos = p; pos < len; ++pos, Yu += 36, Yv += 36) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) t += Yu[6 * k + r] * Yv[6 * k + c];
            acc[6 * r + c] -= t;
          }
      }
      ++i;
      ++j;
    }
  }
  double* out = dp.C + 36ll * (dp.c_off[g] + static_cast<long long>(u) * s + v);
#pragma unroll
  for (int k = 0; k < 36; ++k) out[k] = acc[k];
}

// Rows u of r_S - Y^T y, into the separator node's rows of xv.
__host__ __device__ inline void direct_schur_rhs(const Direct& dp, const DirectSystem& sy, int g, int u) {
  const int su = dp.sep_off[g] + u;
  const long long a = dp.sep_node[su];
  double acc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = sy.rv[6 * a + k];
  for (int i = dp.sc_off[su]; i < dp.sc_off[su + 1]; ++i) {
    const int c = dp.sc[i], run = dp.cpl_run[c], p = dp.cpl_pos[c], len = dp.run_len[run];
    const double* Yu = dp.Y + 36ll * dp.cpl_y[c];
    const double* y = sy.zv + 6ll * (dp.run_begin[run] + p);
    for (int pos = p; pos < len; ++pos, Yu += 36, y += 6) dense_sub_mul(Yu, y, acc, true);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) sy.xv[6 * a + k] = acc[k];
}

// The dense factor's three block operations (right-looking, column k): the pivot is cholesky6; a panel block B <- B L_kk^-T; a
// trailing block C_ij <- C_ij - L_ik L_jk^T.  A block of C sees its updates in ascending k, whoever applies them.
__host__ __device__ __forceinline__ void dense_panel_block(const double* l, double* b) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double v = b[6 * r + c];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= b[6 * r + k] * l[6 * c + k];
      b[6 * r + c] = v / l[6 * c + c];
    }
}
__host__ __device__ __forceinline__ void dense_trailing_block(const double* __restrict__ li, const double* __restrict__ lj, double* c) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) t += li[6 * r + k] * lj[6 * q + k];
      c[6 * r + q] -= t;
    }
}
// z <- L^-1 z and z <- L^-T z with the lower triangle of a 6 x 6 block (r <- r - B z and r <- r - B^T z: dense_sub_mul)
__host__ __device__ __forceinline__ void dense_lower_solve(const double* l, double* z) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = z[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= l[6 * i + k] * z[k];
    z[i] = v / l[6 * i + i];
  }
}
__host__ __device__ __forceinline__ void dense_upper_solve(const double* l, double* z) {
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = z[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= l[6 * k + i] * z[k];
    z[i] = v / l[6 * i + i];
  }
}

// One run, backwards: x_I = L^-T (y - Y x_S) into its rows of xv; the separator nodes' rows of xv hold x_S.  A position's couplings
// are taken in ascending separator order.
__host__ __device__ inline void direct_run_back(const Direct& dp, const DirectSystem& sy, int run) {
  const long long first = dp.run_begin[run];
  const int len = dp.run_len[run];
  double y[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) y[k] = 0.0;
  for (int pos = len - 1; pos >= 0; --pos) {
    const long long node = first + pos;
    double t[6], q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = sy.zv[6 * node + k];
    for (int c = dp.cpl_off[run]; c < dp.cpl_off[run + 1]; ++c) {
      const int p = dp.cpl_pos[c];
      if (pos < p) continue;
      dense_sub_mul(dp.Y + 36ll * (dp.cpl_y[c] + (pos - p)), sy.xv + 6ll * dp.sep_node[dp.cpl_sep[c]], t, false);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (pos + 1 < len) {
#pragma unroll
        for (int c = 0; c < 6; ++c) col[c] = sy.Wc[36 * (node + 1) + 6 * c + r];
      }
      q[r] = chain_row(t[r], col, y);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) y[r] = q[r];
    chain_gt_mul(sy.F + 21 * node, q, t);
#pragma unroll
    for (int k = 0; k < 6; ++k) sy.xv[6 * node + k] = t[k];
  }
}

// One workgroup per graph: what phase 1 of pg_solve_kernel<PRE_CHAIN> leaves -- node blocks D, gradient b, x = 0, r = -b, the
// chain's off-diagonal sums in Wc (assemble_nodes, the same function), the gradient test.
__global__ __launch_bounds__(kBlock) void pg_direct_blocks_kernel(Graphs gr, Params p, GraphState* __restrict__ gs,
                                                                  const double* __restrict__ Haa, const double* __restrict__ Hab,
                                                                  const double* __restrict__ Hbb, const double* __restrict__ ga,
                                                                  const double* __restrict__ gb, double* __restrict__ D,
                                                                  double* __restrict__ bv, double* __restrict__ xv,
                                                                  double* __restrict__ rv, double* __restrict__ Wc,
                                                                  int* __restrict__ fail, const int* __restrict__ bad) {
  __shared__ double red[kWaves];
  const int g = blockIdx.x;
  if (skip(gs, g, bad)) return;  // (uniform over the workgroup)
  const int n0 = gr.node_off[g], n = gr.node_off[g + 1] - n0;
  if (threadIdx.x == 0) fail[g] = 0;
  const double gmax = assemble_nodes<true>(gr, n0, n, Haa, Hab, Hbb, ga, gb, D, bv, xv, rv, Wc);
  gradient_stop(gs, g, block_max(gmax, red), p.gtol);
}

// One thread per run of the call.
__global__ __launch_bounds__(kWave) void pg_direct_factor_kernel(Direct dp, DirectSystem sy, int runs, const GraphState* __restrict__ gs,
                                                                 const int* __restrict__ bad) {
  const int run = blockIdx.x * kWave + threadIdx.x;
  if (run >= runs || *bad != 0) return;
  const int g = dp.run_graph[run];
  if (gs[g].done) return;
  if (!direct_run_factor(dp, sy, 1.0 + gs[g].lambda, run)) dp.fail[g] = 1;  // (every writer writes 1)
}

// One thread per coupling and column.
__global__ __launch_bounds__(kBlock) void pg_direct_border_kernel(Direct dp, DirectSystem sy, int couplings,
                                                                  const GraphState* __restrict__ gs, const int* __restrict__ bad) {
  const int t = blockIdx.x * kBlock + threadIdx.x, cpl = t / 6;
  if (cpl >= couplings || *bad != 0) return;
  if (gs[dp.run_graph[dp.cpl_run[cpl]]].done) return;
  direct_border_column(dp, sy, cpl, t - 6 * cpl);
}

// One thread per Schur item: a graph's s * s blocks (those above the diagonal do nothing) and s right-hand sides.
__global__ __launch_bounds__(kBlock) void pg_direct_schur_kernel(Direct dp, DirectSystem sy, int g_total, long long items,
                                                                 const GraphState* __restrict__ gs, const int* __restrict__ bad) {
  const long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= items || *bad != 0) return;
  int lo = 0, hi = g_total;  // the graph whose items hold t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (dp.item_off[mid] <= t) lo = mid; else hi = mid;
  }
  const int g = lo;
  if (gs[g].done) return;
  const int s = dp.sep_off[g + 1] - dp.sep_off[g];
  const int q = static_cast<int>(t - dp.item_off[g]);
  if (q >= s * s) {
    direct_schur_rhs(dp, sy, g, q - s * s);
    return;
  }
  const int u = q / s, v = q - u * s;
  if (v <= u) direct_schur_block(dp, sy, 1.0 + gs[g].lambda, g, s, u, v);
}

// C = L_S L_S^T in place ([s, s] blocks, the lower triangle) by a whole workgroup, column after column: every thread factors the pivot
// for itself, a block row of the panel per thread, the trailing blocks dealt out by number.  A pivot that is not positive sets
// *fail (in LDS), which every thread may read after the call.
__device__ __forceinline__ void dense_factor(double* C, int s, int* fail) {
  const int tid = threadIdx.x;
  for (int k = 0; k < s; ++k) {
    double l[36];
    double* pivot = C + 36ll * (static_cast<long long>(k) * s + k);
#pragma unroll
    for (int q = 0; q < 36; ++q) l[q] = pivot[q];
    const bool ok = cholesky6(l);
    __syncthreads();  // every thread has read the pivot
    if (tid == 0) {
      if (!ok) *fail = 1;
#pragma unroll
      for (int q = 0; q < 36; ++q) pivot[q] = l[q];
    }
    for (int i = k + 1 + tid; i < s; i += kBlock) {
      double b[36];
      double* B = C + 36ll * (static_cast<long long>(i) * s + k);
#pragma unroll
      for (int q = 0; q < 36; ++q) b[q] = B[q];
      dense_panel_block(l, b);
#pragma unroll
      for (int q = 0; q < 36; ++q) B[q] = b[q];
    }
    __syncthreads();
    const int m = s - k - 1;
    for (int idx = tid; idx < m * m; idx += kBlock) {
      const int i = k + 1 + idx / m, j = k + 1 + idx % m;
      if (j > i) continue;
      double c[36];
      double* Cij = C + 36ll * (static_cast<long long>(i) * s + j);
#pragma unroll
      for (int q = 0; q < 36; ++q) c[q] = Cij[q];
      dense_trailing_block(C + 36ll * (static_cast<long long>(i) * s + k), C + 36ll * (static_cast<long long>(j) * s + k), c);
#pragma unroll
      for (int q = 0; q < 36; ++q) Cij[q] = c[q];
    }
    __syncthreads();
  }
}

// One workgroup per graph: C = L_S L_S^T in place (column after column: every thread factors the pivot for itself, a block row of
// the panel per thread, the trailing blocks dealt out by number), x_S by substitution with the right-hand side in LDS, then the
// graph's runs backwards, a run per thread.  A pivot that is not positive, here or in a run, ends the graph (ST_SINGULAR).
__global__ __launch_bounds__(kBlock) void pg_direct_solve_kernel(Direct dp, DirectSystem sy, GraphState* __restrict__ gs,
                                                                 const int* __restrict__ bad) {
  __shared__ double rs[6 * kMaxSeparator];
  __shared__ int fail;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (skip(gs, g, bad)) return;  // (uniform over the workgroup)
  const int s0 = dp.sep_off[g], s = dp.sep_off[g + 1] - s0;
  double* C = dp.C + 36ll * dp.c_off[g];
  if (tid == 0) fail = dp.fail[g];
  for (int u = tid; u < s; u += kBlock)
#pragma unroll
    for (int k = 0; k < 6; ++k) rs[6 * u + k] = sy.xv[6ll * dp.sep_node[s0 + u] + k];
  __syncthreads();
  dense_factor(C, s, &fail);
  if (fail) {  // (uniform: written before barriers that every thread passed)
    end_graph(gs, g, ST_SINGULAR);
    return;
  }
  for (int k = 0; k < s; ++k) {  // L_S z = r_S
    if (tid == 0) dense_lower_solve(C + 36ll * (static_cast<long long>(k) * s + k), rs + 6 * k);
    __syncthreads();
    for (int i = k + 1 + tid; i < s; i += kBlock) dense_sub_mul(C + 36ll * (static_cast<long long>(i) * s + k), rs + 6 * k, rs + 6 * i, false);
    __syncthreads();
  }
  for (int k = s - 1; k >= 0; --k) {  // L_S^T x_S = z
    if (tid == 0) dense_upper_solve(C + 36ll * (static_cast<long long>(k) * s + k), rs + 6 * k);
    __syncthreads();
    for (int j = tid; j < k; j += kBlock) dense_sub_mul(C + 36ll * (static_cast<long long>(k) * s + j), rs + 6 * k, rs + 6 * j, true);
    __syncthreads();
  }
  for (int u = tid; u < s; u += kBlock)
#pragma unroll
    for (int k = 0; k < 6; ++k) sy.xv[6ll * dp.sep_node[s0 + u] + k] = rs[6 * u + k];
  __syncthreads();
  for (int run = dp.run_off[g] + tid; run < dp.run_off[g + 1]; run += kBlock) direct_run_back(dp, sy, run);
}

// ---- marginal covariances --------------------------------------------------------------------------------
// Sigma_i = (H^-1)_ii of every free node from the direct solve's factors at lambda = 0, by a selected inversion: no dense inverse and
// no solves.  The separator part is Sigma_SS = C^-1 = Z^T Z with Z = L_S^-1.  Along a run, backwards from its last position, with
// Omega_jj = L_jj^T Sigma_jj L_jj and Psi_j = L_jj^T Sigma_{j,S} (the columns of the run's couplings):
//   Psi_j         = -W_{j+1}^T Psi_{j+1} - Y_j Sigma_SS
//   Omega_{j,j+1} = -W_{j+1}^T Omega_{j+1,j+1} - Y_j Psi_{j+1}^T
//   Omega_jj      = I - W_{j+1}^T Omega_{j,j+1}^T - Y_j Psi_j^T
//   Sigma_jj      = G_j^T Omega_jj G_j
// (no W terms at the last position; Y_j is zero for a coupling that begins behind j).  As above, one work item per function, for
// the device and for the host (rdm_pose_graph_marginals_host).
struct Marginals {
  double* Z;  // L_S^-1, a graph's [s, s] blocks at c_off like C; C itself ends as Sigma_SS, both triangles
  double* P;  // Psi: a coupling's 6 x 6 part at 36 * coupling, one column after the other (6 doubles each)
  double* S;  // [N, 36] every node's block before the output's symmetrisation
};

// Scalar column `col` of block column j of Z = L_S^-1 (block rows j .. s - 1) by forward substitution, a row's terms in ascending
// k.  The thread reads back only what it wrote.
__host__ __device__ inline void marg_inverse_column(const double* C, double* Z, int s, int j, int col) {
  for (int i = j; i < s; ++i) {
    double r[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) r[q] = (i == j && q == col) ? 1.0 : 0.0;
    for (int k = j; k < i; ++k) {
      const double* Zk = Z + 36ll * (static_cast<long long>(k) * s + j);
      double z[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) z[q] = Zk[6 * q + col];
      dense_sub_mul(C + 36ll * (static_cast<long long>(i) * s + k), z, r, false);
    }
    dense_lower_solve(C + 36ll * (static_cast<long long>(i) * s + i), r);
    double* Zi = Z + 36ll * (static_cast<long long>(i) * s + j);
#pragma unroll
    for (int q = 0; q < 6; ++q) Zi[6 * q + col] = r[q];
  }
}

// Block (u, v), v <= u, of Sigma_SS = Z^T Z: the sum of Z_ku^T Z_kv over k = u .. s - 1 in ascending k, into block (u, v) of `out`
// and transposed into block (v, u).
__host__ __device__ inline void marg_sigma_block(const double* Z, double* out, int s, int u, int v) {
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (int k = u; k < s; ++k) {
    const double* Zu = Z + 36ll * (static_cast<long long>(k) * s + u);
    const double* Zv = Z + 36ll * (static_cast<long long>(k) * s + v);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double t = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) t += Zu[6 * m + r] * Zv[6 * m + c];
        acc[6 * r + c] += t;
      }
  }
  double* low = out + 36ll * (static_cast<long long>(u) * s + v);
#pragma unroll
  for (int k = 0; k < 36; ++k) low[k] = acc[k];
  if (u != v) {
    double* up = out + 36ll * (static_cast<long long>(v) * s + u);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) up[6 * c + r] = acc[6 * r + c];
  }
}

// One scalar column (number col = 6 * (coupling inside the run) + column of the separator node) of a run's Psi at position pos:
// psi <- -W_{pos+1}^T psi - Y_pos Sigma_SS[:, column] (the run's couplings that have begun, in ascending separator order), in place
// in P; and the column's terms of the two 6 x 6 sums, a1 += y psi_old^T and a2 += y psi_new^T with y the column of Y_pos.  Sg: the
// graph's Sigma_SS ([s, s] blocks), s0 its first separator number.  At the run's last position nothing is read from P.
__host__ __device__ inline void marg_sweep_column(const Direct& dp, const DirectSystem& sy, const Marginals& mg, const double* Sg, int s,
                                                  int s0, int run, int pos, int col, double* a1, double* a2) {
  const int c0 = dp.cpl_off[run], c1 = dp.cpl_off[run + 1], len = dp.run_len[run];
  const int cu = c0 + col / 6, q = col - 6 * (col / 6), su = dp.cpl_sep[cu] - s0;
  double* p = mg.P + 36ll * cu + 6 * q;
  double old[6], now[6];
  if (pos + 1 < len) {
#pragma unroll
    for (int k = 0; k < 6; ++k) old[k] = p[k];
    block_mul(sy.Wc + 36ll * (dp.run_begin[run] + pos + 1), old, true, now);
#pragma unroll
    for (int k = 0; k < 6; ++k) now[k] = -now[k];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) old[k] = now[k] = 0.0;
  }
  for (int c = c0; c < c1; ++c) {
    const int pc = dp.cpl_pos[c];
    if (pos < pc) continue;
    const double* Sb = Sg + 36ll * (static_cast<long long>(dp.cpl_sep[c] - s0) * s + su);
    double sv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) sv[k] = Sb[6 * k + q];
    dense_sub_mul(dp.Y + 36ll * (dp.cpl_y[c] + (pos - pc)), sv, now, false);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) p[k] = now[k];
  const int pu = dp.cpl_pos[cu];
  if (pos >= pu) {
    const double* Yu = dp.Y + 36ll * (dp.cpl_y[cu] + (pos - pu));
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double y = Yu[6 * r + q];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        a1[6 * r + k] += y * old[k];
        a2[6 * r + k] += y * now[k];
      }
    }
  }
}

// The node's step after the columns': om holds Omega_{j+1,j+1} (unused at the run's last position) and leaves as Omega_jj; a1 = Y_j
// Psi_{j+1}^T and a2 = Y_j Psi_j^T summed over the columns (both are used up); out = G_j^T Omega_jj G_j.
__host__ __device__ inline void marg_sweep_node(const DirectSystem& sy, long long node, bool last, double* a1, double* a2, double* om,
                                                double* out) {
  if (!last) {
    const double* W = sy.Wc + 36 * (node + 1);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) t += W[6 * k + r] * om[6 * k + c];
        a1[6 * r + c] = -t - a1[6 * r + c];  // Omega_{j,j+1}
      }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) t += W[6 * k + r] * a1[6 * c + k];
        om[6 * r + c] = ((r == c ? 1.0 : 0.0) - t) - a2[6 * r + c];
      }
  } else {
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) om[6 * r + c] = (r == c ? 1.0 : 0.0) - a2[6 * r + c];
  }
  const double* G = sy.F + 21 * node;
  double g[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) g[k] = G[k];
#pragma unroll
  for (int r = 0; r < 6; ++r)  // a2 <- Omega G
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double t = 0.0;
#pragma unroll
      for (int k = c; k < 6; ++k) t += om[6 * r + k] * g[k * (k + 1) / 2 + c];
      a2[6 * r + c] = t;
    }
#pragma unroll
  for (int r = 0; r < 6; ++r)  // out <- G^T (Omega G)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double t = 0.0;
#pragma unroll
      for (int k = r; k < 6; ++k) t += g[k * (k + 1) / 2 + r] * a2[6 * k + c];
      out[6 * r + c] = t;
    }
}

// A node's block of the output: zeros for node 0, NaN for a graph whose factor failed, else the staged block with every entry above
// the diagonal a copy of the one below it.
__host__ __device__ inline void marg_write_block(const double* staged, bool first, bool failed, double* out) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) out[6 * r + c] = first ? 0.0 : failed ? NAN : staged[6 * (r > c ? r : c) + (r > c ? c : r)];
}

// One thread per graph: the state the direct solve's kernels read -- lambda = 0 (their diagonal scale 1 + lambda is exactly 1), not
// done unless the graph has no free node.
__global__ __launch_bounds__(kBlock) void pg_marg_init_kernel(GraphState* __restrict__ gs, int g, const int* __restrict__ node_off) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= g) return;
  GraphState s;
  s.lambda = s.cost = s.cost0 = s.cand_cost = s.grad_max = 0.0;
  s.iterations = s.pcg_total = s.accepted = 0;
  s.stop = STOP_NONE;
  s.status = ST_OK;
  s.done = node_off[i + 1] - node_off[i] <= 1 ? 1 : 0;
  gs[i] = s;
}

// One thread per edge: the edge's blocks at the given poses through edge_terms, the given weight (null: 1) in the line process's
// place.  A weight that is negative or not finite and a residual beyond the angle limit refuse the call through the graph's status;
// such an edge's slots are zeros.
__global__ __launch_bounds__(kBlock) void pg_marg_linearize_kernel(Graphs gr, int e_total, const double* __restrict__ X,
                                                                   const double* __restrict__ T, const double* __restrict__ L,
                                                                   const double* __restrict__ weights, GraphState* __restrict__ gs,
                                                                   double* __restrict__ Haa, double* __restrict__ Hab,
                                                                   double* __restrict__ Hbb, double* __restrict__ ga,
                                                                   double* __restrict__ gb, const int* __restrict__ bad) {
  const long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= e_total || *bad != 0) return;
  const double l = weights != nullptr ? weights[e] : 1.0;
  double l_out, term;
  int status = ST_OK;
  if (!(l >= 0.0) || !isfinite(l)) {
    status = ST_WEIGHT;
  } else if (!edge_terms(X + 16ll * gr.es[e], X + 16ll * gr.et[e], T + 16 * e, L + 36 * e, 0.0, false, &l_out, &term, Haa + 36 * e,
                         Hab + 36 * e, Hbb + 36 * e, ga + 6 * e, gb + 6 * e, nullptr, &l)) {
    status = ST_ANGLE;
  }
  if (status == ST_OK) return;
  gs[gr.edge_graph[e]].status = status;  // (any writer's value names a cause that is present)
  for (int k = 0; k < 36; ++k) Haa[36 * e + k] = Hab[36 * e + k] = Hbb[36 * e + k] = 0.0;
  for (int k = 0; k < 6; ++k) ga[6 * e + k] = gb[6 * e + k] = 0.0;
}

// One workgroup per graph: C = L_S L_S^T (dense_factor), Z = L_S^-1 a scalar column per thread, Sigma_SS = Z^T Z a block per
// thread into C, and the separator nodes' own blocks into S.
__global__ __launch_bounds__(kBlock) void pg_marg_separator_kernel(Direct dp, Marginals mg, const GraphState* __restrict__ gs,
                                                                   const int* __restrict__ bad) {
  __shared__ int fail;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (skip(gs, g, bad)) return;  // (uniform over the workgroup)
  const int s0 = dp.sep_off[g], s = dp.sep_off[g + 1] - s0;
  double* C = dp.C + 36ll * dp.c_off[g];
  double* Z = mg.Z + 36ll * dp.c_off[g];
  if (tid == 0) fail = dp.fail[g];
  __syncthreads();
  dense_factor(C, s, &fail);
  if (fail) {  // (uniform: written before barriers that every thread passed)
    if (tid == 0) dp.fail[g] = 1;
    return;
  }
  for (int t = tid; t < 6 * s; t += kBlock) marg_inverse_column(C, Z, s, t / 6, t % 6);
  __syncthreads();  // Z is whole, and L_S is read no more
  for (int idx = tid; idx < s * s; idx += kBlock) {
    const int u = idx / s, v = idx - u * s;
    if (v <= u) marg_sigma_block(Z, C, s, u, v);
  }
  __syncthreads();
  for (int u = tid; u < s; u += kBlock) {
    const double* d = C + 36ll * (static_cast<long long>(u) * s + u);
    double* o = mg.S + 36ll * dp.sep_node[s0 + u];
#pragma unroll
    for (int k = 0; k < 36; ++k) o[k] = d[k];
  }
}

// One wavefront per run, backwards along it.  Lane l owns the scalar columns l, l + 64, ... of the run's Psi (marg_sweep_column: a
// lane reads back only what it wrote); the two 6 x 6 sums over the columns are per-lane partial sums in ascending column, then
// wave_sum's butterfly, which leaves the same bits in every lane; every lane then takes the node's step (marg_sweep_node) on those
// wave-uniform values and lane 0 stores the block.  kTimed (the phase-timing build's entry): lane 0 adds the clock ticks spent in
// the columns, the butterflies and the node steps to ticks[3 run ..].
template <bool kTimed>
__global__ __launch_bounds__(kWave) void pg_marg_sweep_kernel(Direct dp, DirectSystem sy, Marginals mg, const GraphState* __restrict__ gs,
                                                              const int* __restrict__ bad, long long* __restrict__ ticks) {
  const int run = blockIdx.x, lane = threadIdx.x;
  if (*bad != 0) return;
  const int g = dp.run_graph[run];
  if (gs[g].done || dp.fail[g] != 0) return;  // (uniform over the wavefront)
  const int s0 = dp.sep_off[g], s = dp.sep_off[g + 1] - s0, len = dp.run_len[run];
  const int cols = 6 * (dp.cpl_off[run + 1] - dp.cpl_off[run]);
  const long long first = dp.run_begin[run];
  const double* Sg = dp.C + 36ll * dp.c_off[g];
  double om[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) om[k] = 0.0;
  long long t_cols = 0, t_sum = 0, t_node = 0, t0 = 0;
  for (int pos = len - 1; pos >= 0; --pos) {
    double a1[36], a2[36], out[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) a1[k] = a2[k] = 0.0;
    if constexpr (kTimed) t0 = wall_clock64();
    for (int col = lane; col < cols; col += kWave) marg_sweep_column(dp, sy, mg, Sg, s, s0, run, pos, col, a1, a2);
    if constexpr (kTimed) {
      const long long t = wall_clock64();
      t_cols += t - t0;
      t0 = t;
    }
    if (cols > 0) {
#pragma unroll
      for (int k = 0; k < 36; ++k) {
        a1[k] = wave_sum(a1[k]);
        a2[k] = wave_sum(a2[k]);
      }
    }
    if constexpr (kTimed) {
      const long long t = wall_clock64();
      t_sum += t - t0;
      t0 = t;
    }
    marg_sweep_node(sy, first + pos, pos + 1 == len, a1, a2, om, out);
    if (lane == 0) {
      double* o = mg.S + 36 * (first + pos);
#pragma unroll
      for (int k = 0; k < 36; ++k) o[k] = out[k];
    }
    if constexpr (kTimed) t_node += wall_clock64() - t0;
  }
  if constexpr (kTimed) {
    if (lane == 0 && ticks != nullptr) {
      ticks[3 * run] = t_cols;
      ticks[3 * run + 1] = t_sum;
      ticks[3 * run + 2] = t_node;
    }
  }
}

// One thread per node: the output (marg_write_block), only when the call is not refused.
__global__ __launch_bounds__(kBlock) void pg_marg_finish_kernel(Graphs gr, int n_total, const int* __restrict__ fail,
                                                                const int* __restrict__ failed, const double* __restrict__ S,
                                                                double* __restrict__ out) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_total || *failed != 0) return;
  const int g = gr.node_graph[i];
  marg_write_block(S + 36 * i, i == gr.node_off[g], fail[g] != 0, out + 36 * i);
}

// ---- cross covariances and loop-edge consistency -------------------------------------------------------------
// Sigma_st = (H^-1)_st for a list of pairs (s, t), from the same factors and Sigma_SS: the six columns of H^-1 that belong to the
// pair's COLUMN NODE t are solved for -- forwards along t's run (y = L^-1 e, then u_S = -Y^T y), through the separator
// (x_S = Sigma_SS u_S), backwards along the run of every row node asked for (x = L^-T (y - Y x_S)) -- and the rows of s are read off.
// A thread owns ONE of the six scalar columns of one column node: its recurrences need nothing from another thread, and every sum
// it forms has an order that the graph and the pair decide.  The columns of a call are taken kColumnsInFlight at a time; their y,
// u_S and x_S live in the workspace.  As above, one work item per function, for the device and for the host
// (rdm_pose_graph_pair_covariances_host).
constexpr int kColumnsInFlight = 128;  // column nodes whose forward vectors the workspace holds at a time

struct Pairs {             // the host-built plan of a call's pairs (global node, run, separator and coupling numbers) and its arrays
  const int* pair_s;       // [P] the pair's nodes
  const int* pair_t;       // [P]
  const int* col_node;     // [K] the distinct column nodes, ascending
  const int* col_run;      // [K] the column node's run, or -1: it is a separator node
  const int* col_pos;      // [K] its position in the run, or its separator number
  const int* grp_off;      // [R + 1] a group's items; a group is a column and a run that holds row nodes (or -1: rows in the separator)
  const int* grp_col;      // [R] ascending, so a chunk of columns is a range of groups
  const int* grp_run;      // [R]
  const int* item_pos;     // [I] the row node's position in the run, descending inside a group, or its separator number
  const int* item_pair;    // [I] the pair whose block the item is
  int y_stride, u_stride, x_stride;  // 6 x 6 blocks per column in flight: forward positions, couplings of its run, separator nodes
  double* yf;              // [kColumnsInFlight, y_stride, 36] a block is six scalar columns of 6 doubles each
  double* us;              // [kColumnsInFlight, u_stride, 36]
  double* xs;              // [kColumnsInFlight, x_stride, 36]
  double* cross;           // [P + 1, 36] Sigma_st of every pair, staged; block P is zeros (node 0's rows)
  unsigned long long* bad_pair;  // 8 * (the first refused pair) + its cause, or all ones
};

// Scalar column c of column k (in slot `slot` of the chunk), forwards: y_p = G_p e_c at the node's position, y_j = -W_j y_{j-1} to the
// run's end, as direct_run_factor carries its y; then the column's part of u_S = -Y^T y, a coupling of the run after the other, the
// positions in ascending order as direct_schur_rhs takes them.  The thread reads back only what it wrote.
__host__ __device__ inline void cons_forward_column(const Direct& dp, const DirectSystem& sy, const Pairs& pp, int k, int slot, int c) {
  const int run = pp.col_run[k];
  if (run < 0) return;
  const int p = pp.col_pos[k], len = dp.run_len[run];
  const long long first = dp.run_begin[run];
  double* yf = pp.yf + 36ll * slot * pp.y_stride + 6 * c;
  const double* G = sy.F + 21 * (first + p);
  double y[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) yf[r] = y[r] = r >= c ? G[r * (r + 1) / 2 + c] : 0.0;
  for (int pos = p + 1; pos < len; ++pos) {
    const double* W = sy.Wc + 36 * (first + pos);
    double t[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) t[r] = chain_row(0.0, W + 6 * r, y);
#pragma unroll
    for (int r = 0; r < 6; ++r) yf[36ll * (pos - p) + r] = y[r] = t[r];
  }
  const int c0 = dp.cpl_off[run], c1 = dp.cpl_off[run + 1];
  for (int cu = c0; cu < c1; ++cu) {
    const int pc = dp.cpl_pos[cu], b = pc > p ? pc : p;
    const double* Yc = dp.Y + 36ll * (dp.cpl_y[cu] + (b - pc));
    const double* yy = yf + 36ll * (b - p);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int pos = b; pos < len; ++pos, Yc += 36, yy += 36) dense_sub_mul(Yc, yy, acc, true);
    double* u = pp.us + 36ll * (static_cast<long long>(slot) * pp.u_stride + (cu - c0)) + 6 * c;
#pragma unroll
    for (int r = 0; r < 6; ++r) u[r] = acc[r];
  }
}

// Scalar column c of block v of x_S = Sigma_SS u_S of column k: the sum over the couplings of the column node's run, which are in
// ascending separator order; for a column node that is itself separator node number col_pos, column c of block (v, col_pos) of
// Sigma_SS.  Sg: the graph's Sigma_SS ([s, s] blocks, both triangles), s0 its first separator number.
__host__ __device__ inline void cons_separator_column(const Direct& dp, const Pairs& pp, const double* Sg, int s, int s0, int k, int slot,
                                                      int v, int c) {
  const int run = pp.col_run[k];
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (run < 0) {
    const double* Sb = Sg + 36ll * (static_cast<long long>(v) * s + (pp.col_pos[k] - s0));
#pragma unroll
    for (int r = 0; r < 6; ++r) x[r] = Sb[6 * r + c];
  } else {
    const int c0 = dp.cpl_off[run], c1 = dp.cpl_off[run + 1];
    for (int cu = c0; cu < c1; ++cu) {
      const double* u = pp.us + 36ll * (static_cast<long long>(slot) * pp.u_stride + (cu - c0)) + 6 * c;
      double t[6];
      block_mul(Sg + 36ll * (static_cast<long long>(v) * s + (dp.cpl_sep[cu] - s0)), u, false, t);
#pragma unroll
      for (int r = 0; r < 6; ++r) x[r] += t[r];
    }
  }
  double* o = pp.xs + 36ll * (static_cast<long long>(slot) * pp.x_stride + v) + 6 * c;
#pragma unroll
  for (int r = 0; r < 6; ++r) o[r] = x[r];
}

// Scalar column c of group `group` (column k in slot `slot`, row run `run`): x = L^-T (y [the column's own run] - Y x_S) backwards from
// the run's last position down to the lowest one asked for, as direct_run_back goes (a position's couplings that have begun in
// ascending separator order); column c of the block of every item on the way is written.  Row nodes in the separator (run -1) read x_S.
__host__ __device__ inline void cons_back_column(const Direct& dp, const DirectSystem& sy, const Pairs& pp, int s0, int group, int slot,
                                                 int c) {
  const int k = pp.grp_col[group], run = pp.grp_run[group];
  int it = pp.grp_off[group];
  const int ie = pp.grp_off[group + 1];
  const double* xs = pp.xs + 36ll * slot * pp.x_stride + 6 * c;
  if (run < 0) {
    for (; it < ie; ++it) {
      const double* x = xs + 36ll * (pp.item_pos[it] - s0);
      double* o = pp.cross + 36ll * pp.item_pair[it] + c;
#pragma unroll
      for (int r = 0; r < 6; ++r) o[6 * r] = x[r];
    }
    return;
  }
  const bool same = pp.col_run[k] == run;
  const int p = same ? pp.col_pos[k] : 0, len = dp.run_len[run], low = pp.item_pos[ie - 1];
  const long long first = dp.run_begin[run];
  const double* yf = pp.yf + 36ll * slot * pp.y_stride + 6 * c;
  const int c0 = dp.cpl_off[run], c1 = dp.cpl_off[run + 1];
  double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int pos = len - 1; pos >= low; --pos) {
    const long long node = first + pos;
    double t[6], q[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) t[r] = same && pos >= p ? yf[36ll * (pos - p) + r] : 0.0;
    for (int cu = c0; cu < c1; ++cu) {
      const int pc = dp.cpl_pos[cu];
      if (pos < pc) continue;
      dense_sub_mul(dp.Y + 36ll * (dp.cpl_y[cu] + (pos - pc)), xs + 36ll * (dp.cpl_sep[cu] - s0), t, false);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (pos + 1 < len) {
#pragma unroll
        for (int j = 0; j < 6; ++j) col[j] = sy.Wc[36 * (node + 1) + 6 * j + r];
      }
      q[r] = chain_row(t[r], col, y);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) y[r] = q[r];
    if (it < ie && pp.item_pos[it] == pos) {
      chain_gt_mul(sy.F + 21 * node, q, t);
      for (; it < ie && pp.item_pos[it] == pos; ++it) {
        double* o = pp.cross + 36ll * pp.item_pair[it] + c;
#pragma unroll
        for (int r = 0; r < 6; ++r) o[6 * r] = t[r];
      }
    }
  }
}

// Entry (r, c) of a node's covariance block whose lower triangle holds it (a staged block, or an exactly symmetric one).
__host__ __device__ __forceinline__ double sym_entry(const double* S, int r, int c) { return S[6 * (r > c ? r : c) + (r > c ? c : r)]; }

// One pair from (X_s, X_t, T, L or null) and the blocks Sigma_ss, Sigma_tt (their lower triangles are read) and Sigma_st (rows: s): the
// residual r (as edge_terms gives it), M = A Sigma_ss A^T + A Sigma_st B^T + B Sigma_ts A^T + B Sigma_tt B^T with edge_terms'
// Jacobians -- its lower triangle is computed and copied above the diagonal -- and d2 = r^T (M + L^-1)^-1 r by cholesky6 (L^-1 from
// chain_factor_node's G = F^-1 of L = F F^T; L symmetrised as the edges' are).  -> 0; 1: L or M + L^-1 is not positive definite (d2
// is NaN); -1: the residual is beyond the angle limit (nothing but r is written).
__host__ __device__ inline int pair_terms(const double* Xs, const double* Xt, const double* T, const double* L, const double* Sss,
                                          const double* Stt, const double* Sst, double* r_out, double* M_out, double* d2_out) {
  Residual res;
  const bool ok = edge_residual(Xs, Xt, T, res);
  double r[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r_out[i] = r[i] = res.w.v[i];
    r_out[3 + i] = r[3 + i] = res.v.v[i];
  }
  if (!ok) return -1;
  double A[36], B[36], m[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) A[k] = B[k] = m[k] = 0.0;
  {
    const EdgeJacobians J = edge_jacobians(res, T);
    put_block(A, 0, 0, J.Ja, 1.0);
    put_block(A, 1, 1, J.Ra, 1.0);
    put_block(B, 0, 0, J.B11, 1.0);
    put_block(B, 1, 0, J.B21, 1.0);
    put_block(B, 1, 1, J.B22, 1.0);
  }
  {  // U = A Sigma_ss + B Sigma_ts, then the lower triangle of U A^T
    double U[36];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          a += A[6 * i + k] * sym_entry(Sss, k, j);
          b += B[6 * i + k] * Sst[6 * j + k];
        }
        U[6 * i + j] = a + b;
      }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) a += U[6 * i + k] * A[6 * j + k];
        m[6 * i + j] = a;
      }
  }
  {  // V = A Sigma_st + B Sigma_tt, then the lower triangle of V B^T on top
    double V[36];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          a += A[6 * i + k] * Sst[6 * k + j];
          b += B[6 * i + k] * sym_entry(Stt, k, j);
        }
        V[6 * i + j] = a + b;
      }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) a += V[6 * i + k] * B[6 * j + k];
        m[6 * i + j] += a;
      }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) M_out[6 * i + j] = m[6 * (i > j ? i : j) + (i > j ? j : i)];
  bool pd = true;
  if (L != nullptr) {  // the lower triangle of L^-1 = G^T G on top of M's
    double d[36], g[21], x[36];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) d[6 * i + j] = 0.5 * (L[6 * i + j] + L[6 * j + i]);
    pd = chain_factor_node(d, nullptr, nullptr, g, x);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double a = 0.0;
#pragma unroll
        for (int k = i; k < 6; ++k) a += g[k * (k + 1) / 2 + i] * g[k * (k + 1) / 2 + j];
        m[6 * i + j] += a;
      }
  }
  if (!cholesky6(m)) pd = false;
  dense_lower_solve(m, r);
  double d2 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) d2 += r[i] * r[i];
  *d2_out = pd ? d2 : NAN;
  return pd ? 0 : 1;
}

// One thread per pair: its transform and information as pg_check_kernel holds an edge's, and the angle limit of its residual at the
// given poses.  The first refused pair and its cause go to *bad_pair (an integer minimum), and the call is refused through *failed.
__global__ __launch_bounds__(kBlock) void pg_cons_check_kernel(Pairs pp, int p_total, const double* __restrict__ X,
                                                               const double* __restrict__ T, const double* __restrict__ L,
                                                               const int* __restrict__ bad, int* __restrict__ failed) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= p_total || *bad != 0) return;
  int b = 0;
  const double* Ti = T + 16 * i;
  for (int k = 0; k < 16; ++k)
    if (!isfinite(Ti[k])) b = ST_NONFINITE;
  if (L != nullptr) {
    const double* M = L + 36 * i;
    double big = 0.0;
    for (int k = 0; k < 36; ++k) {
      if (!isfinite(M[k])) b = ST_NONFINITE;
      big = fmax(big, fabs(M[k]));
    }
    if (b == 0)
      for (int r = 0; r < 6; ++r)
        for (int c = r + 1; c < 6; ++c)
          if (fabs(M[6 * r + c] - M[6 * c + r]) > kSymTol * big) b = ST_ASYMMETRIC;
  }
  if (b == 0) {
    Residual r;
    if (!edge_residual(X + 16ll * pp.pair_s[i], X + 16ll * pp.pair_t[i], Ti, r)) b = ST_ANGLE;
  }
  if (b == 0) return;
  atomicMin(pp.bad_pair, 8ull * static_cast<unsigned long long>(i) + static_cast<unsigned long long>(b));
  *failed = b;  // (any writer's value names a cause that is present)
}

// The graph of column k takes no part: the input check refused the call, or the graph has no free node or a failed pivot.
__device__ __forceinline__ bool cons_skip(const Graphs& gr, const Direct& dp, const Pairs& pp, const GraphState* gs, const int* bad, int k,
                                          int* g_out) {
  if (*bad != 0) return true;
  const int g = gr.node_graph[pp.col_node[k]];
  *g_out = g;
  return gs[g].done || dp.fail[g] != 0;
}

// One thread per scalar column of the chunk's columns k0 .. k0 + cols - 1.
__global__ __launch_bounds__(kBlock) void pg_cons_forward_kernel(Graphs gr, Direct dp, DirectSystem sy, Pairs pp, int k0, int cols,
                                                                 const GraphState* __restrict__ gs, const int* __restrict__ bad) {
  const int t = blockIdx.x * kBlock + threadIdx.x, slot = t / 6;
  int g;
  if (slot >= cols || cons_skip(gr, dp, pp, gs, bad, k0 + slot, &g)) return;
  cons_forward_column(dp, sy, pp, k0 + slot, slot, t - 6 * slot);
}

// One thread per scalar column of every block of x_S of the chunk's columns (x_stride blocks each; a graph uses its first s).
__global__ __launch_bounds__(kBlock) void pg_cons_separator_kernel(Graphs gr, Direct dp, Pairs pp, int k0, int cols,
                                                                   const GraphState* __restrict__ gs, const int* __restrict__ bad) {
  const long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const int slot = static_cast<int>(t / (6ll * pp.x_stride));
  int g;
  if (slot >= cols || cons_skip(gr, dp, pp, gs, bad, k0 + slot, &g)) return;
  const int q = static_cast<int>(t - 6ll * pp.x_stride * slot), v = q / 6;
  const int s0 = dp.sep_off[g], s = dp.sep_off[g + 1] - s0;
  if (v >= s) return;
  cons_separator_column(dp, pp, dp.C + 36ll * dp.c_off[g], s, s0, k0 + slot, slot, v, q - 6 * v);
}

// One thread per scalar column of the chunk's groups r0 .. r0 + groups - 1.
__global__ __launch_bounds__(kBlock) void pg_cons_back_kernel(Graphs gr, Direct dp, DirectSystem sy, Pairs pp, int k0, int r0, int groups,
                                                              const GraphState* __restrict__ gs, const int* __restrict__ bad) {
  const int t = blockIdx.x * kBlock + threadIdx.x, q = t / 6;
  if (q >= groups) return;
  const int k = pp.grp_col[r0 + q];
  int g;
  if (cons_skip(gr, dp, pp, gs, bad, k, &g)) return;
  cons_back_column(dp, sy, pp, dp.sep_off[g], r0 + q, k - k0, t - 6 * q);
}

// One thread per pair, only when the call is not refused: the pair's outputs (each may be null) from the staged blocks through
// pair_terms; NaN for a graph whose factor failed; a pair with node 0 has a zero cross block.
__global__ __launch_bounds__(kWave) void pg_cons_pair_kernel(Graphs gr, Pairs pp, int p_total, const double* __restrict__ X,
                                                             const double* __restrict__ T, const double* __restrict__ L,
                                                             const int* __restrict__ fail, const int* __restrict__ failed,
                                                             const double* __restrict__ S, double* __restrict__ cross_out,
                                                             double* __restrict__ m_out, double* __restrict__ d2_out,
                                                             uint8_t* __restrict__ status_out) {
  const int i = blockIdx.x * kWave + threadIdx.x;
  if (i >= p_total || *failed != 0) return;
  const long long a = pp.pair_s[i], b = pp.pair_t[i];
  const int g = gr.node_graph[a];
  const long long node0 = gr.node_off[g];
  const double* zero = pp.cross + 36ll * p_total;
  const double* Sst = a == node0 || b == node0 ? zero : pp.cross + 36ll * i;
  double r[6], m[36], d2 = NAN;
  int status = 0;
  const bool dead = fail[g] != 0;
  if (!dead)
    status = pair_terms(X + 16 * a, X + 16 * b, T + 16ll * i, L != nullptr ? L + 36ll * i : nullptr, a == node0 ? zero : S + 36 * a,
                        b == node0 ? zero : S + 36 * b, Sst, r, m, &d2);
  if (cross_out != nullptr)
    for (int k = 0; k < 36; ++k) cross_out[36ll * i + k] = dead ? NAN : Sst[k];
  if (m_out != nullptr)
    for (int k = 0; k < 36; ++k) m_out[36ll * i + k] = dead ? NAN : m[k];
  if (d2_out != nullptr) d2_out[i] = dead ? NAN : d2;
  if (status_out != nullptr) status_out[i] = static_cast<uint8_t>(status > 0 ? status : 0);
}

// One thread per node: candidate pose Xc = X [Exp(dw) | dt]; node 0 of a graph keeps its pose.
__global__ __launch_bounds__(kBlock) void pg_update_kernel(Graphs gr, int n_total, const GraphState* __restrict__ gs,
                                                           const double* __restrict__ X, const double* __restrict__ xv,
                                                           double* __restrict__ Xc, const int* __restrict__ bad) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_total || *bad != 0) return;
  const int g = gr.node_graph[i];
  if (gs[g].done) return;
  if (i == gr.node_off[g]) {
    for (int k = 0; k < 16; ++k) Xc[16 * i + k] = X[16 * i + k];
    return;
  }
  retract(X + 16 * i, xv + 6 * i, Xc + 16 * i);
}

// One block; a thread per graph adds the graph's cost terms in edge order and decides.  mode 0: the initial cost.  Then thread 0
// counts the graphs that are not done into *remaining (in order; no atomics).
__global__ __launch_bounds__(kBlock) void pg_step_kernel(Graphs gr, int g_total, Params p, int mode, const double* __restrict__ term,
                                                         GraphState* __restrict__ gs, int* __restrict__ remaining,
                                                         const int* __restrict__ bad) {
  if (*bad != 0) {
    if (threadIdx.x == 0) *remaining = 0;
    return;
  }
  for (int g = threadIdx.x; g < g_total; g += kBlock) {
    GraphState s = gs[g];
    if (s.done) {  // (its last step was committed by the launch after the step that ended it)
      if (s.accepted) gs[g].accepted = 0;
      continue;
    }
    double f = 0.0;
    for (int e = gr.edge_off[g]; e < gr.edge_off[g + 1]; ++e) f += term[e];
    s.accepted = 0;
    if (mode == 0) {
      if (!isfinite(f)) {
        s.status = isnan(f) ? ST_NONFINITE : ST_ANGLE;
        s.done = 1;
      }
      s.cost = s.cost0 = f;
      if (p.max_iterations <= 0 && !s.done) {
        s.stop = STOP_MAX_ITERATIONS;
        s.done = 1;
      }
    } else {
      s.cand_cost = f;
      s.iterations += 1;
      if (f <= s.cost) {  // accept (false for +inf beyond the angle limit and for NaN)
        const double rel = s.cost > 0.0 ? (s.cost - f) / s.cost : 0.0;
        s.cost = f;
        s.accepted = 1;
        s.lambda = fmax(s.lambda * kLambdaDown, kLambdaMin);
        if (rel <= p.ctol) {
          s.stop = STOP_COST;
          s.done = 1;
        }
      } else {
        s.lambda *= kLambdaUp;
        if (s.lambda > kLambdaMax) {
          s.stop = STOP_COST;
          s.done = 1;
        }
      }
      if (!s.done && s.iterations >= p.max_iterations) {
        s.stop = STOP_MAX_ITERATIONS;
        s.done = 1;
      }
    }
    gs[g] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int left = 0;
    for (int g = 0; g < g_total; ++g) left += gs[g].done ? 0 : 1;
    *remaining = left;
  }
}

// One thread per node: an accepted candidate becomes the pose.  (A graph that stopped on this step still takes its last step.)
__global__ __launch_bounds__(kBlock) void pg_commit_kernel(Graphs gr, int n_total, const GraphState* __restrict__ gs,
                                                           double* __restrict__ X, const double* __restrict__ Xc,
                                                           const int* __restrict__ bad) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_total || *bad != 0) return;
  if (!gs[gr.node_graph[i]].accepted) return;
  for (int k = 0; k < 16; ++k) X[16 * i + k] = Xc[16 * i + k];
}

// Outputs, only when no graph of the call failed: poses, weights at the final poses, pruned flags.
__global__ __launch_bounds__(kBlock) void pg_finish_kernel(Graphs gr, int n_total, int e_total, Params p,
                                                           const GraphState* __restrict__ gs, const int* __restrict__ failed,
                                                           const double* __restrict__ X, const double* __restrict__ lw,
                                                           double* __restrict__ nodes_out, double* __restrict__ weights_out,
                                                           uint8_t* __restrict__ pruned_out) {
  if (*failed != 0) return;
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < 16ll * n_total) nodes_out[i] = X[i];
  if (i < e_total) {
    const bool empty = gs[gr.edge_graph[i]].stop == STOP_EMPTY;
    const double l = empty ? 1.0 : lw[i];
    if (weights_out) weights_out[i] = l;
    if (pruned_out) pruned_out[i] = (gr.uncertain != nullptr && gr.uncertain[i] != 0 && p.mu > 0.0 && l < p.prune) ? 1 : 0;
  }
}

// One thread: the report [G, kReport] and the call's failure word (the first failing graph's status, or the input check's).
__global__ void pg_report_kernel(int g_total, const GraphState* __restrict__ gs, const int* __restrict__ bad,
                                 double* __restrict__ report, int* __restrict__ failed) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int f = *bad;
  for (int g = 0; g < g_total; ++g) {
    const GraphState s = gs[g];
    if (f == 0 && s.status != ST_OK) f = s.status;
    double* r = report + static_cast<long long>(g) * kReport;
    r[0] = s.cost0;
    r[1] = s.cost;
    r[2] = s.iterations;
    r[3] = s.pcg_total;
    r[4] = s.stop;
    r[5] = s.status;
    r[6] = s.lambda;
    r[7] = s.grad_max;
  }
  *failed = f;
}

// ---- host ------------------------------------------------------------------------------------------------------------------

struct Work {
  int *node_off, *edge_off, *edge_graph, *node_graph, *es, *et, *inc_off, *inc;
  uint8_t* uncertain;
  int* flags;  // bad, remaining, failed
  GraphState* gs;
  double *X, *Xc, *lw, *term, *Haa, *Hab, *Hbb, *ga, *gb, *D, *F, *bv, *xv, *rv, *zv, *pv, *report;
  double* Wc;  // the chain preconditioner's [N, 36]; null without it
  size_t ints_bytes;  // the host-built integer tables are one upload: [node_off .. uncertain)
};

// The host-built tables; they lie first in the workspace, in one piece, so that the host fills a buffer of the same layout.
void carve_tables(Arena& ar, int64_t g, int64_t n, int64_t e, Work& w) {
  const size_t G = static_cast<size_t>(g > 0 ? g : 1), N = static_cast<size_t>(n > 0 ? n : 1), E = static_cast<size_t>(e > 0 ? e : 1);
  w.node_off = ar.take<int>(G + 1);
  w.edge_off = ar.take<int>(G + 1);
  w.edge_graph = ar.take<int>(E);
  w.node_graph = ar.take<int>(N);
  w.es = ar.take<int>(E);
  w.et = ar.take<int>(E);
  w.inc_off = ar.take<int>(N + 1);
  w.inc = ar.take<int>(2 * E);
  w.uncertain = ar.take<uint8_t>(E);
  w.ints_bytes = ar.off;
}

unsigned blocks_for(int64_t n) { return static_cast<unsigned>(((n > 0 ? n : 1) + kBlock - 1) / kBlock); }  // (n < 2^35: < 2^27 blocks)

// ---- the direct solve's plan (host) ------------------------------------------------------------------------------------------

// The separator of one graph: a vertex cover of the pairs of free nodes that an edge joins and that are not
// neighbours on the chain, chosen greedily -- the node with the most uncovered pairs, the lowest number among equals -- and returned
// in ascending order.  ends(e, s, t) gives edge e's ends inside the graph (already checked).
template <typename Ends>
void choose_separator(int64_t n, int64_t ne, Ends ends, std::vector<int>& S) {
  S.clear();
  std::vector<std::pair<int, int>> pairs;
  for (int64_t e = 0; e < ne; ++e) {
    int64_t s, t;
    ends(e, s, t);
    if (s == 0 || t == 0 || s - t == 1 || t - s == 1 || s == t) continue;
    pairs.emplace_back(static_cast<int>(std::min(s, t)), static_cast<int>(std::max(s, t)));
  }
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  if (pairs.empty()) return;
  const size_t P = pairs.size();
  std::vector<int> off(static_cast<size_t>(n) + 1, 0), count(static_cast<size_t>(n), 0);
  for (const auto& p : pairs) {
    off[p.first + 1] += 1;
    off[p.second + 1] += 1;
  }
  for (int64_t i = 0; i < n; ++i) {
    count[i] = off[i + 1];
    off[i + 1] += off[i];
  }
  std::vector<int> adj(2 * P), fill(off.begin(), off.end() - 1);
  for (size_t k = 0; k < P; ++k) {
    adj[fill[pairs[k].first]++] = static_cast<int>(k);
    adj[fill[pairs[k].second]++] = static_cast<int>(k);
  }
  std::set<std::pair<int, int>> order;  // (-uncovered pairs, node): the first is the next choice
  for (int64_t i = 0; i < n; ++i)
    if (count[i] > 0) order.emplace(-count[i], static_cast<int>(i));
  std::vector<char> covered(P, 0);
  while (!order.empty()) {
    const int node = order.begin()->second;
    order.erase(order.begin());
    S.push_back(node);
    for (int q = off[node]; q < off[node + 1]; ++q) {
      const int k = adj[q];
      if (covered[k]) continue;
      covered[k] = 1;
      const int other = pairs[k].first == node ? pairs[k].second : pairs[k].first;
      order.erase({-count[other], other});
      if (--count[other] > 0) order.emplace(-count[other], other);
    }
    count[node] = 0;
  }
  std::sort(S.begin(), S.end());
}

struct DirectPlan {  // Direct's tables on the host
  std::vector<int> sep_off, sep_node, run_off, run_begin, run_len, run_graph, cpl_off, cpl_sep, cpl_run, cpl_pos, cpl_y, ent_off, ent_pos,
      ent_code, sc_off, sc;
  std::vector<long long> c_off, item_off;
  long long y_blocks = 0;
};

// The ONE list of the tables (plan member, Direct member), in the order in which they lie in the workspace: the carve, the fill
// and the host's view of a plan all walk it, so a table is named here and in the two structs and nowhere else.
template <typename T>
struct DirectTable {
  std::vector<T> DirectPlan::*plan;
  const T* Direct::*table;
};
constexpr DirectTable<int> kDirectInts[] = {
    {&DirectPlan::sep_off, &Direct::sep_off},     {&DirectPlan::sep_node, &Direct::sep_node},   {&DirectPlan::run_off, &Direct::run_off},
    {&DirectPlan::run_begin, &Direct::run_begin}, {&DirectPlan::run_len, &Direct::run_len},     {&DirectPlan::run_graph, &Direct::run_graph},
    {&DirectPlan::cpl_off, &Direct::cpl_off},     {&DirectPlan::cpl_sep, &Direct::cpl_sep},     {&DirectPlan::cpl_run, &Direct::cpl_run},
    {&DirectPlan::cpl_pos, &Direct::cpl_pos},     {&DirectPlan::cpl_y, &Direct::cpl_y},         {&DirectPlan::ent_off, &Direct::ent_off},
    {&DirectPlan::ent_pos, &Direct::ent_pos},     {&DirectPlan::ent_code, &Direct::ent_code},   {&DirectPlan::sc_off, &Direct::sc_off},
    {&DirectPlan::sc, &Direct::sc}};
constexpr DirectTable<long long> kDirectLongs[] = {{&DirectPlan::c_off, &Direct::c_off}, {&DirectPlan::item_off, &Direct::item_off}};
template <typename Visit>
void for_each_direct_table(const DirectPlan& pl, Direct& d, Visit visit) {  // visit(the plan's vector, Direct's pointer to the table)
  for (const auto& t : kDirectInts) visit(pl.*t.plan, d.*t.table);
  for (const auto& t : kDirectLongs) visit(pl.*t.plan, d.*t.table);
}

// The plan of a call from its tables (global node numbers; inc in ascending edge order).  false, with the error set: a graph's
// separator is above the cap, or Y is too large to index.
bool build_direct_plan(int64_t G, const int* node_off, const int* edge_off, const int* es, const int* et, const int* inc_off,
                       const int* inc, DirectPlan& pl, const char* who, const char* hint = " (use the conjugate gradients)") {
  pl = DirectPlan();
  pl.sep_off.push_back(0);
  pl.run_off.push_back(0);
  pl.cpl_off.push_back(0);
  pl.sc_off.push_back(0);
  pl.c_off.push_back(0);
  pl.item_off.push_back(0);
  std::vector<int> S, node_sep, node_run;
  struct Entry {
    int run, sep, pos, code;
    bool operator<(const Entry& o) const {
      return run != o.run ? run < o.run : sep != o.sep ? sep < o.sep : pos != o.pos ? pos < o.pos : code < o.code;
    }
  };
  std::vector<Entry> entries;
  for (int64_t g = 0; g < G; ++g) {
    const int n0 = node_off[g], n = node_off[g + 1] - n0, e0 = edge_off[g], ne = edge_off[g + 1] - e0;
    choose_separator(n, ne, [&](int64_t e, int64_t& s, int64_t& t) { s = es[e0 + e] - n0; t = et[e0 + e] - n0; }, S);
    if (static_cast<int>(S.size()) > kMaxSeparator) {
      set_error("%s: graph %lld needs %zu separator nodes for the direct solve; the limit is %d%s", who, static_cast<long long>(g),
                S.size(), kMaxSeparator, hint);
      return false;
    }
    const int s = static_cast<int>(S.size()), sep0 = static_cast<int>(pl.sep_node.size()), run0 = static_cast<int>(pl.run_begin.size());
    node_sep.assign(static_cast<size_t>(n > 0 ? n : 1), -1);
    node_run.assign(static_cast<size_t>(n > 0 ? n : 1), -1);
    for (int u = 0; u < s; ++u) {
      node_sep[S[u]] = sep0 + u;
      pl.sep_node.push_back(n0 + S[u]);
    }
    for (int i = 1; i < n; ++i) {
      if (node_sep[i] >= 0) continue;
      if (i == 1 || node_sep[i - 1] >= 0) {
        pl.run_begin.push_back(n0 + i);
        pl.run_len.push_back(0);
        pl.run_graph.push_back(static_cast<int>(g));
      }
      node_run[i] = static_cast<int>(pl.run_begin.size()) - 1;
      pl.run_len.back() += 1;
    }
    // couplings: the edges of every separator node whose other end lies in a run
    entries.clear();
    for (int u = 0; u < s; ++u) {
      const int a = n0 + S[u];
      for (int q = inc_off[a]; q < inc_off[a + 1]; ++q) {
        const int code = inc[q], e = code >> 1, b = ((code & 1) ? es[e] : et[e]) - n0;
        if (b == 0 || node_run[b] < 0) continue;
        entries.push_back({node_run[b], sep0 + u, n0 + b - pl.run_begin[node_run[b]], code});
      }
    }
    std::sort(entries.begin(), entries.end());
    const int cpl0 = static_cast<int>(pl.cpl_sep.size());
    size_t k = 0;
    for (int run = run0; run < static_cast<int>(pl.run_begin.size()); ++run) {
      for (; k < entries.size() && entries[k].run == run; ++k) {
        const Entry& en = entries[k];
        if (k == 0 || entries[k - 1].run != en.run || entries[k - 1].sep != en.sep) {  // a new coupling; its first entry has its first position
          pl.ent_off.push_back(static_cast<int>(pl.ent_pos.size()));
          pl.cpl_sep.push_back(en.sep);
          pl.cpl_run.push_back(run);
          pl.cpl_pos.push_back(en.pos);
          pl.cpl_y.push_back(static_cast<int>(pl.y_blocks));
          pl.y_blocks += pl.run_len[run] - en.pos;
          if (pl.y_blocks > (1ll << 31) - 64) {
            set_error("%s: the border of the direct solve is too large to index (graph %lld)", who, static_cast<long long>(g));
            return false;
          }
        }
        pl.ent_pos.push_back(en.pos);
        pl.ent_code.push_back(en.code);
      }
      pl.cpl_off.push_back(static_cast<int>(pl.cpl_sep.size()));
    }
    // a separator node's couplings, ascending run (the couplings are numbered by run, then separator node)
    std::vector<int> cnt(static_cast<size_t>(s) + 1, 0);
    for (size_t c = cpl0; c < pl.cpl_sep.size(); ++c) cnt[pl.cpl_sep[c] - sep0 + 1] += 1;
    for (int u = 0; u < s; ++u) cnt[u + 1] += cnt[u];
    const int sc0 = static_cast<int>(pl.sc.size());
    pl.sc.resize(pl.sc.size() + (pl.cpl_sep.size() - cpl0));
    for (int u = 0; u < s; ++u) pl.sc_off.push_back(sc0 + cnt[u + 1]);
    for (size_t c = cpl0; c < pl.cpl_sep.size(); ++c) pl.sc[sc0 + cnt[pl.cpl_sep[c] - sep0]++] = static_cast<int>(c);
    pl.sep_off.push_back(static_cast<int>(pl.sep_node.size()));
    pl.run_off.push_back(static_cast<int>(pl.run_begin.size()));
    pl.c_off.push_back(pl.c_off.back() + static_cast<long long>(s) * s);
    pl.item_off.push_back(pl.item_off.back() + static_cast<long long>(s) * s + s);
  }
  pl.ent_off.push_back(static_cast<int>(pl.ent_pos.size()));  // (a coupling's entries end where the next one's begin)
  return true;
}

// Direct's tables in the workspace, behind the other host-built tables and uploaded with them.
void carve_direct_tables(Arena& ar, const DirectPlan& pl, Work& w, Direct& d) {
  for_each_direct_table(pl, d, [&](const auto& v, auto& table) {
    table = ar.take<typename std::decay_t<decltype(v)>::value_type>(v.size() > 0 ? v.size() : 1);
  });
  w.ints_bytes = ar.off;
}
void carve_direct_arrays(Arena& ar, const DirectPlan& pl, size_t G, Direct& d) {
  d.C = ar.take<double>(36 * static_cast<size_t>(pl.c_off.back() > 0 ? pl.c_off.back() : 1));
  d.Y = ar.take<double>(36 * static_cast<size_t>(pl.y_blocks > 0 ? pl.y_blocks : 1));
  d.fail = ar.take<int>(G);
}
// The plan's tables into a host buffer laid out as carve_direct_tables lays the workspace out (h: the same carve on that buffer).
void fill_direct_tables(const DirectPlan& pl, Direct h) {  // (h by value: the walk hands out its pointers, which are not changed)
  for_each_direct_table(pl, h, [](const auto& v, auto& table) {
    if (!v.empty()) memcpy(const_cast<void*>(static_cast<const void*>(table)), v.data(), v.size() * sizeof(v[0]));
  });
}

// plan: the direct solve's (null: conjugate gradients, and the layout is what it was)
bool carve(Arena& ar, int64_t g, int64_t n, int64_t e, int preconditioner, Work& w, const DirectPlan* plan = nullptr,
           Direct* direct = nullptr) {
  const size_t G = static_cast<size_t>(g > 0 ? g : 1), N = static_cast<size_t>(n > 0 ? n : 1), E = static_cast<size_t>(e > 0 ? e : 1);
  carve_tables(ar, g, n, e, w);
  if (plan) carve_direct_tables(ar, *plan, w, *direct);
  w.flags = ar.take<int>(4);
  w.gs = ar.take<GraphState>(G);
  w.X = ar.take<double>(16 * N);
  w.Xc = ar.take<double>(16 * N);
  w.lw = ar.take<double>(E);
  w.term = ar.take<double>(E);
  w.Haa = ar.take<double>(36 * E);
  w.Hab = ar.take<double>(36 * E);
  w.Hbb = ar.take<double>(36 * E);
  w.ga = ar.take<double>(6 * E);
  w.gb = ar.take<double>(6 * E);
  w.D = ar.take<double>(36 * N);
  w.F = ar.take<double>(21 * N);
  w.bv = ar.take<double>(6 * N);
  w.xv = ar.take<double>(6 * N);
  w.rv = ar.take<double>(6 * N);
  w.zv = ar.take<double>(6 * N);
  w.pv = ar.take<double>(6 * N);
  w.report = ar.take<double>(kReport * G);
  w.Wc = preconditioner == PRE_CHAIN || plan ? ar.take<double>(36 * N) : nullptr;  // (last: the other slots lie where they lay)
  if (plan) carve_direct_arrays(ar, *plan, G, *direct);
  return ar.ok;
}


// The offsets of a call's graphs.
int check_graphs(int64_t G, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host) {
  RDM_REQUIRE(graph_node_offsets_host[0] == 0 && graph_edge_offsets_host[0] == 0, "rdm_pose_graph_optimize: offsets must begin at 0");
  for (int64_t g = 0; g < G; ++g) {
    const int64_t n = graph_node_offsets_host[g + 1] - graph_node_offsets_host[g];
    const int64_t e = graph_edge_offsets_host[g + 1] - graph_edge_offsets_host[g];
    RDM_REQUIRE(n >= 0 && e >= 0, "rdm_pose_graph_optimize: offsets of graph %lld decrease", static_cast<long long>(g));
    RDM_REQUIRE(n <= kMaxNodes && e <= kMaxEdges,
                "rdm_pose_graph_optimize: graph %lld has %lld nodes and %lld edges; the limits are %lld and %lld per graph",
                static_cast<long long>(g), static_cast<long long>(n), static_cast<long long>(e), static_cast<long long>(kMaxNodes),
                static_cast<long long>(kMaxEdges));
  }
  const int64_t N = graph_node_offsets_host[G], E = graph_edge_offsets_host[G];
  RDM_REQUIRE(N < kMaxTotal && E < kMaxTotal / 2, "rdm_pose_graph_optimize: too many nodes or edges in one call");
  return RDM_OK;
}

// The integer tables (t: carve_tables on a zeroed host buffer): global node ids, graph of every node / edge, incidence lists by a
// counting sort.
int fill_tables(int64_t G, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host, const int64_t* edges_host,
                const uint8_t* uncertain_host, const Work& t) {
  const int64_t N = graph_node_offsets_host[G], E = graph_edge_offsets_host[G];
  int *node_off = t.node_off, *edge_off = t.edge_off, *edge_graph = t.edge_graph, *node_graph = t.node_graph, *es = t.es, *et = t.et;
  int *inc_off = t.inc_off, *inc = t.inc;
  uint8_t* unc = t.uncertain;
  for (int64_t g = 0; g <= G; ++g) {
    node_off[g] = static_cast<int>(graph_node_offsets_host[g]);
    edge_off[g] = static_cast<int>(graph_edge_offsets_host[g]);
  }
  for (int64_t i = 0; i <= N; ++i) inc_off[i] = 0;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t n = node_off[g + 1] - node_off[g];
    for (int64_t i = node_off[g]; i < node_off[g + 1]; ++i) node_graph[i] = static_cast<int>(g);
    for (int64_t e = edge_off[g]; e < edge_off[g + 1]; ++e) {
      const int64_t s = edges_host[2 * e], t = edges_host[2 * e + 1];
      RDM_REQUIRE(s >= 0 && s < n && t >= 0 && t < n, "rdm_pose_graph_optimize: edge %lld (%lld, %lld) is outside graph %lld of %lld nodes",
                  static_cast<long long>(e), static_cast<long long>(s), static_cast<long long>(t), static_cast<long long>(g),
                  static_cast<long long>(n));
      RDM_REQUIRE(s != t, "rdm_pose_graph_optimize: edge %lld joins node %lld to itself", static_cast<long long>(e),
                  static_cast<long long>(s));
      edge_graph[e] = static_cast<int>(g);
      es[e] = static_cast<int>(node_off[g] + s);
      et[e] = static_cast<int>(node_off[g] + t);
      inc_off[es[e] + 1] += 1;
      inc_off[et[e] + 1] += 1;
      unc[e] = uncertain_host ? (uncertain_host[e] != 0 ? 1 : 0) : 0;
    }
  }
  for (int64_t i = 0; i < N; ++i) inc_off[i + 1] += inc_off[i];
  std::vector<int> fill(inc_off, inc_off + N);
  for (int64_t e = 0; e < E; ++e) {  // ascending edge order per node
    inc[fill[es[e]]++] = static_cast<int>(2 * e);
    inc[fill[et[e]]++] = static_cast<int>(2 * e + 1);
  }
  return RDM_OK;
}

// `host` grown (with zeros; what it holds stays) to what layout(Arena&) carves, and carved: once on a null arena for the size, then
// on the buffer.
template <typename Layout>
void carve_host(std::vector<char>& host, Layout layout) {
  Arena sizes(nullptr, 0);
  layout(sizes);
  host.resize(sizes.off, 0);
  Arena ar(host.data(), host.size());
  layout(ar);
}

// The integer tables of a call, filled, in a host buffer laid out as the workspace's first part; t: their view on `host`.
int fill_host_tables(int64_t G, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                     const int64_t* edges_host, const uint8_t* uncertain_host, std::vector<char>& host, Work& t) {
  const int64_t N = graph_node_offsets_host[G], E = graph_edge_offsets_host[G];
  host.clear();
  carve_host(host, [&](Arena& ar) { carve_tables(ar, G, N, E, t); });
  return fill_tables(G, graph_node_offsets_host, graph_edge_offsets_host, edges_host, uncertain_host, t);
}

// The host-built tables of a call in one buffer laid out as the workspace's first part; with `plan`, the direct solve's behind them.
int build_host_tables(int64_t G, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                      const int64_t* edges_host, const uint8_t* uncertain_host, std::vector<char>& host, DirectPlan* plan,
                      const char* who = "rdm_pose_graph_optimize", const char* hint = " (use the conjugate gradients)") {
  Work t;
  const int rc = fill_host_tables(G, graph_node_offsets_host, graph_edge_offsets_host, edges_host, uncertain_host, host, t);
  if (rc != RDM_OK || plan == nullptr) return rc;
  if (!build_direct_plan(G, t.node_off, t.edge_off, t.es, t.et, t.inc_off, t.inc, *plan, who, hint)) return RDM_ERR_ARG;
  const int64_t N = graph_node_offsets_host[G], E = graph_edge_offsets_host[G];
  Direct d;
  carve_host(host, [&](Arena& ar) {  // (the filled tables lie first and stay)
    carve_tables(ar, G, N, E, t);
    carve_direct_tables(ar, *plan, t, d);
  });
  fill_direct_tables(*plan, d);
  return RDM_OK;
}

// What a graph's status says, for the calls' messages.
const char* status_text(int status) {
  static const char* const what[] = {"", "a pose, transform or information entry is not finite", "an information matrix is not symmetric",
                                     "a residual rotation of the given poses is beyond the supported angle (cos < -0.99)",
                                     "a node's block is not positive definite (a node that no edge reaches, or an indefinite information matrix)",
                                     "a weight is negative or not finite"};
  return what[status >= 1 && status <= 5 ? status : 0];
}

// The workspace of rdm_pose_graph_marginals: the tables and the direct solve's, the per-edge and per-node arrays that its kernels
// read and write (Work's other members stay null), then Z, Psi and the staged blocks.
bool carve_marginals(Arena& ar, int64_t g, int64_t n, int64_t e, Work& w, const DirectPlan& plan, Direct& d, Marginals& m) {
  const size_t G = static_cast<size_t>(g > 0 ? g : 1), N = static_cast<size_t>(n > 0 ? n : 1), E = static_cast<size_t>(e > 0 ? e : 1);
  w = Work();
  carve_tables(ar, g, n, e, w);
  carve_direct_tables(ar, plan, w, d);
  w.flags = ar.take<int>(4);
  w.gs = ar.take<GraphState>(G);
  w.Haa = ar.take<double>(36 * E);
  w.Hab = ar.take<double>(36 * E);
  w.Hbb = ar.take<double>(36 * E);
  w.ga = ar.take<double>(6 * E);
  w.gb = ar.take<double>(6 * E);
  w.D = ar.take<double>(36 * N);
  w.F = ar.take<double>(21 * N);
  w.bv = ar.take<double>(6 * N);
  w.xv = ar.take<double>(6 * N);
  w.rv = ar.take<double>(6 * N);
  w.zv = ar.take<double>(6 * N);
  w.report = ar.take<double>(kReport * G);
  w.Wc = ar.take<double>(36 * N);
  carve_direct_arrays(ar, plan, G, d);
  m.Z = ar.take<double>(36 * static_cast<size_t>(plan.c_off.back() > 0 ? plan.c_off.back() : 1));
  m.P = ar.take<double>(36 * (plan.cpl_sep.empty() ? 1 : plan.cpl_sep.size()));
  m.S = ar.take<double>(36 * N);
  return ar.ok;
}

// The direct solve of one system on the host up to the factors: the plan, the runs' factors (and y = L^-1 rhs), the border, the Schur
// complement and its dense factor, by the kernels' functions in their order.  RDM_ERR_ARG, with `who` in the message, for a failed
// pivot and for a separator above the limit.
struct HostDirect {
  std::vector<char> host;
  DirectPlan plan;
  Work t;
  std::vector<double> F, Wc, zv, xv, C, Y;
  int fail = 0, runs = 0, couplings = 0, s = 0;
  Direct dp = {};
  DirectSystem sy = {};
  double* block(int i, int j) { return C.data() + 36 * (static_cast<size_t>(i) * s + j); }
};
int host_direct_factor(HostDirect& h, int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, const double* diag, const double* off,
                       const double* rhs, const char* who, const char* hint) {
  const int64_t noff[2] = {0, n_nodes}, eoff[2] = {0, n_edges};
  Work& t = h.t;
  const int rc = fill_host_tables(1, noff, eoff, edges_host, nullptr, h.host, t);
  if (rc != RDM_OK) return rc;
  {  // edges that touch node 0 stay out of the incidence lists (they hold no block of the system)
    int kept = 0;
    std::vector<int> inc_off(static_cast<size_t>(n_nodes) + 1, 0);
    for (int64_t i = 0; i < n_nodes; ++i) {
      inc_off[i] = kept;
      for (int q = t.inc_off[i]; q < t.inc_off[i + 1]; ++q) {
        const int e = t.inc[q] >> 1;
        if (t.es[e] != 0 && t.et[e] != 0) t.inc[kept++] = t.inc[q];
      }
    }
    inc_off[n_nodes] = kept;
    for (int64_t i = 0; i <= n_nodes; ++i) t.inc_off[i] = inc_off[i];
  }
  DirectPlan& plan = h.plan;
  if (!build_direct_plan(1, t.node_off, t.edge_off, t.es, t.et, t.inc_off, t.inc, plan, who, hint)) return RDM_ERR_ARG;
  const size_t N = static_cast<size_t>(n_nodes);
  h.F.assign(21 * N, 0.0);
  h.Wc.assign(36 * N, 0.0);
  h.zv.assign(6 * N, 0.0);
  h.xv.assign(6 * N, 0.0);
  h.C.assign(36 * static_cast<size_t>(plan.c_off.back()) + 36, 0.0);
  h.Y.assign(36 * static_cast<size_t>(plan.y_blocks) + 36, 0.0);
  Direct& dp = h.dp;
  for_each_direct_table(plan, dp, [](const auto& v, auto& table) { table = v.empty() ? nullptr : v.data(); });
  dp.C = h.C.data();
  dp.Y = h.Y.data();
  dp.fail = &h.fail;
  h.sy = {t.es, t.et, t.inc_off, t.inc, diag, off, rhs, h.F.data(), h.Wc.data(), h.zv.data(), h.xv.data()};
  const DirectSystem& sy = h.sy;
  for (int64_t i = 2; i < n_nodes; ++i) chain_off_block(t.es, t.et, t.inc_off, t.inc, off, i, &h.Wc[36 * i]);
  h.runs = static_cast<int>(plan.run_begin.size());
  h.couplings = static_cast<int>(plan.cpl_sep.size());
  h.s = plan.sep_off[1];
  const int s = h.s;
  for (int run = 0; run < h.runs; ++run)
    if (!direct_run_factor(dp, sy, 1.0, run)) {
      set_error("%s: a pivot of the run that begins at node %d is not positive definite", who, plan.run_begin[run]);
      return RDM_ERR_ARG;
    }
  for (int c = 0; c < h.couplings; ++c)
    for (int col = 0; col < 6; ++col) direct_border_column(dp, sy, c, col);
  for (int u = 0; u < s; ++u)
    for (int v = 0; v <= u; ++v) direct_schur_block(dp, sy, 1.0, 0, s, u, v);
  for (int k = 0; k < s; ++k) {  // the dense factor, column after column
    if (!cholesky6(h.block(k, k))) {
      set_error("%s: the Schur complement's pivot of node %d is not positive definite", who, plan.sep_node[k]);
      return RDM_ERR_ARG;
    }
    for (int i = k + 1; i < s; ++i) dense_panel_block(h.block(k, k), h.block(i, k));
    for (int i = k + 1; i < s; ++i)
      for (int j = k + 1; j <= i; ++j) dense_trailing_block(h.block(i, k), h.block(j, k), h.block(i, j));
  }
  return RDM_OK;
}

// pg_marg_sweep_kernel's run on the host: the 64 lanes' partial sums one lane after the other, then wave_sum's butterfly.
void marg_sweep_run_host(const Direct& dp, const DirectSystem& sy, const Marginals& mg, int run) {
  const int s = dp.sep_off[1], len = dp.run_len[run], cols = 6 * (dp.cpl_off[run + 1] - dp.cpl_off[run]);
  const long long first = dp.run_begin[run];
  double om[36] = {};
  std::vector<double> a1(kWave * 36), a2(kWave * 36), b(kWave * 36);
  auto butterfly = [&](std::vector<double>& a) {
    for (int o = 32; o > 0; o >>= 1) {
      for (int l = 0; l < kWave; ++l)
        for (int k = 0; k < 36; ++k) b[36 * l + k] = a[36 * l + k] + a[36 * (l ^ o) + k];
      a.swap(b);
    }
  };
  for (int pos = len - 1; pos >= 0; --pos) {
    std::fill(a1.begin(), a1.end(), 0.0);
    std::fill(a2.begin(), a2.end(), 0.0);
    for (int lane = 0; lane < kWave; ++lane)
      for (int col = lane; col < cols; col += kWave) marg_sweep_column(dp, sy, mg, dp.C, s, 0, run, pos, col, &a1[36 * lane], &a2[36 * lane]);
    if (cols > 0) {
      butterfly(a1);
      butterfly(a2);
    }
    marg_sweep_node(sy, first + pos, pos + 1 == len, a1.data(), a2.data(), om, mg.S + 36 * (first + pos));
  }
}

// ---- the pairs' plan (host) ------------------------------------------------------------------------------------------------------

struct PairPlan {  // Pairs' tables on the host, and what the host alone needs: a chunk's first group, the strides
  std::vector<int> pair_s, pair_t, col_node, col_run, col_pos, grp_off, grp_col, grp_run, item_pos, item_pair;
  std::vector<int> chunk_grp;  // [chunks + 1] the first group of every chunk of kColumnsInFlight columns
  int y_stride = 1, u_stride = 1, x_stride = 1;
};
// The ONE list of Pairs' tables, as kDirectInts is the direct solve's.
struct PairTable {
  std::vector<int> PairPlan::*plan;
  const int* Pairs::*table;
};
constexpr PairTable kPairInts[] = {{&PairPlan::pair_s, &Pairs::pair_s},     {&PairPlan::pair_t, &Pairs::pair_t},
                                   {&PairPlan::col_node, &Pairs::col_node}, {&PairPlan::col_run, &Pairs::col_run},
                                   {&PairPlan::col_pos, &Pairs::col_pos},   {&PairPlan::grp_off, &Pairs::grp_off},
                                   {&PairPlan::grp_col, &Pairs::grp_col},   {&PairPlan::grp_run, &Pairs::grp_run},
                                   {&PairPlan::item_pos, &Pairs::item_pos}, {&PairPlan::item_pair, &Pairs::item_pair}};

// The plan of a call's pairs over the direct solve's plan: the pairs checked (inside their graph, s != t), grouped by column node t,
// then by the run of the row node s, positions descending -- so a column's forward pass runs once and a run's backward pass once,
// down to the lowest position asked for.  Pairs with node 0 hold no block and stay out of the groups.  false, with the error set.
bool build_pair_plan(int64_t G, const int* node_off, const DirectPlan& pl, const int64_t* pair_off, const int64_t* pairs_host,
                     PairPlan& pp, const char* who) {
  pp = PairPlan();
  const int64_t N = node_off[G], P = pair_off[G];
  std::vector<int> node_run(static_cast<size_t>(N > 0 ? N : 1), -1), node_at(static_cast<size_t>(N > 0 ? N : 1), -1);
  for (size_t r = 0; r < pl.run_begin.size(); ++r)
    for (int i = 0; i < pl.run_len[r]; ++i) {
      node_run[pl.run_begin[r] + i] = static_cast<int>(r);
      node_at[pl.run_begin[r] + i] = i;
    }
  for (size_t u = 0; u < pl.sep_node.size(); ++u) node_at[pl.sep_node[u]] = static_cast<int>(u);
  struct Item {
    int col, run, pos, pair;
    bool operator<(const Item& o) const {
      return col != o.col ? col < o.col : run != o.run ? run < o.run : pos != o.pos ? pos > o.pos : pair < o.pair;
    }
  };
  std::vector<Item> items;
  pp.pair_s.resize(static_cast<size_t>(P));
  pp.pair_t.resize(static_cast<size_t>(P));
  for (int64_t g = 0; g < G; ++g) {
    const int64_t n = node_off[g + 1] - node_off[g];
    for (int64_t k = pair_off[g]; k < pair_off[g + 1]; ++k) {
      const int64_t s = pairs_host[2 * k], t = pairs_host[2 * k + 1];
      if (s < 0 || s >= n || t < 0 || t >= n) {
        set_error("%s: pair %lld (%lld, %lld) is outside graph %lld of %lld nodes", who, static_cast<long long>(k), static_cast<long long>(s),
                  static_cast<long long>(t), static_cast<long long>(g), static_cast<long long>(n));
        return false;
      }
      if (s == t) {
        set_error("%s: pair %lld joins node %lld to itself", who, static_cast<long long>(k), static_cast<long long>(s));
        return false;
      }
      pp.pair_s[k] = static_cast<int>(node_off[g] + s);
      pp.pair_t[k] = static_cast<int>(node_off[g] + t);
      if (s == 0 || t == 0) continue;
      items.push_back({pp.pair_t[k], node_run[pp.pair_s[k]], node_at[pp.pair_s[k]], static_cast<int>(k)});  // (col: the node, for now)
    }
  }
  std::sort(items.begin(), items.end());
  std::vector<int> run_couplings(pl.run_begin.size(), 0);
  for (size_t r = 0; r < pl.run_begin.size(); ++r) run_couplings[r] = pl.cpl_off[r + 1] - pl.cpl_off[r];
  int graph = 0;
  for (size_t i = 0; i < items.size(); ++i) {
    const Item& it = items[i];
    const bool new_col = i == 0 || items[i - 1].col != it.col;
    if (new_col) {
      const int node = it.col, run = node_run[node];
      if (pp.col_node.size() % kColumnsInFlight == 0) pp.chunk_grp.push_back(static_cast<int>(pp.grp_col.size()));
      pp.col_node.push_back(node);
      pp.col_run.push_back(run);
      pp.col_pos.push_back(node_at[node]);
      while (node >= node_off[graph + 1]) ++graph;
      pp.x_stride = std::max(pp.x_stride, pl.sep_off[graph + 1] - pl.sep_off[graph]);
      if (run >= 0) {
        pp.y_stride = std::max(pp.y_stride, pl.run_len[run] - node_at[node]);
        pp.u_stride = std::max(pp.u_stride, run_couplings[run]);
      }
    }
    if (new_col || items[i - 1].run != it.run) {
      pp.grp_off.push_back(static_cast<int>(i));
      pp.grp_col.push_back(static_cast<int>(pp.col_node.size()) - 1);
      pp.grp_run.push_back(it.run);
    }
    pp.item_pos.push_back(it.pos);
    pp.item_pair.push_back(it.pair);
  }
  pp.grp_off.push_back(static_cast<int>(items.size()));
  pp.chunk_grp.push_back(static_cast<int>(pp.grp_col.size()));
  return true;
}

template <typename Visit>
void for_each_pair_table(const PairPlan& pl, Pairs& d, Visit visit) {
  for (const auto& t : kPairInts) visit(pl.*t.plan, d.*t.table);
}

// The pairs' part of the workspace, behind the marginals': the tables (one upload, from *tables_begin for *tables_bytes), the
// forward vectors, u_S and x_S of the columns in flight, the staged cross blocks and the refusal word.
bool carve_pairs(Arena& ar, const PairPlan& pl, Pairs& d, void** tables_begin, size_t* tables_bytes) {
  const size_t begin = ar.off;
  *tables_begin = ar.base != nullptr ? ar.base + begin : nullptr;
  for_each_pair_table(pl, d, [&](const std::vector<int>& v, const int*& table) { table = ar.take<int>(v.size() > 0 ? v.size() : 1); });
  *tables_bytes = ar.off - begin;
  const size_t cols = std::min<size_t>(pl.col_node.size() > 0 ? pl.col_node.size() : 1, kColumnsInFlight);
  d.y_stride = pl.y_stride;
  d.u_stride = pl.u_stride;
  d.x_stride = pl.x_stride;
  d.yf = ar.take<double>(36 * cols * static_cast<size_t>(pl.y_stride));
  d.us = ar.take<double>(36 * cols * static_cast<size_t>(pl.u_stride));
  d.xs = ar.take<double>(36 * cols * static_cast<size_t>(pl.x_stride));
  d.cross = ar.take<double>(36 * (pl.pair_s.size() + 1));
  d.bad_pair = ar.take<unsigned long long>(1);
  return ar.ok;
}

// The checks of a consistency call's host arguments, then the two plans; the marginals' refusals come first.
int build_consistency_plans(const char* who, int64_t G, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                            const int64_t* edges_host, const int64_t* graph_pair_offsets_host, const int64_t* pairs_host,
                            std::vector<char>& host, DirectPlan& plan, PairPlan& pairs) {
  RDM_REQUIRE(G >= 0 && G < kMaxTotal && graph_node_offsets_host && graph_edge_offsets_host && graph_pair_offsets_host,
              "%s: bad number of graphs or null offsets", who);
  int rc = check_graphs(G, graph_node_offsets_host, graph_edge_offsets_host);
  if (rc != RDM_OK) return rc;
  RDM_REQUIRE(graph_edge_offsets_host[G] == 0 || edges_host, "%s: null edges", who);
  RDM_REQUIRE(graph_pair_offsets_host[0] == 0, "%s: pair offsets must begin at 0", who);
  for (int64_t g = 0; g < G; ++g)
    RDM_REQUIRE(graph_pair_offsets_host[g + 1] >= graph_pair_offsets_host[g], "%s: pair offsets of graph %lld decrease", who,
                static_cast<long long>(g));
  RDM_REQUIRE(graph_pair_offsets_host[G] < kMaxTotal / 36, "%s: too many pairs in one call", who);
  RDM_REQUIRE(graph_pair_offsets_host[G] == 0 || pairs_host, "%s: null pairs", who);
  rc = build_host_tables(G, graph_node_offsets_host, graph_edge_offsets_host, edges_host, nullptr, host, &plan, who, "");
  if (rc != RDM_OK) return rc;
  Work t;
  Arena ar(host.data(), host.size());
  carve_tables(ar, G, graph_node_offsets_host[G], graph_edge_offsets_host[G], t);
  return build_pair_plan(G, t.node_off, plan, graph_pair_offsets_host, pairs_host, pairs, who) ? RDM_OK : RDM_ERR_ARG;
}

thread_local long long* t_marg_ticks = nullptr;  // rdm_dbg_pose_graph_marginals_ticks

// The marginals' kernels on the stream, from the state's initialisation to the run sweep and the report (which sets *failed): the
// staged blocks lie in mg.S, Sigma_SS in dp.C.  rdm_pose_graph_marginals and rdm_pose_graph_consistency both launch exactly this.
void enqueue_marginals(hipStream_t st, const Graphs& gr, const Work& w, const Direct& dp, const Marginals& mg, const DirectPlan& plan,
                       int64_t G, int64_t N, int64_t E, const double* nodes, const double* transforms, const double* informations,
                       const double* weights) {
  Params p = {};
  p.gtol = -1.0;  // (pg_direct_blocks_kernel's gradient test never ends a graph: the blocks are wanted at a minimum too)
  int *bad = w.flags, *failed = w.flags + 2;
  const int n = static_cast<int>(N), e = static_cast<int>(E), g = static_cast<int>(G);
  const DirectSystem sy = {w.es, w.et, w.inc_off, w.inc, w.D, w.Hab, w.rv, w.F, w.Wc, w.zv, w.xv};
  const int runs = static_cast<int>(plan.run_begin.size()), couplings = static_cast<int>(plan.cpl_sep.size());
  const long long items = plan.item_off.back();
  fill_words<int>(w.flags, 4, 0, st);
  fill_words<int>(dp.fail, G, 0, st);
  hipLaunchKernelGGL(pg_marg_init_kernel, dim3(blocks_for(G)), dim3(kBlock), 0, st, w.gs, g, w.node_off);
  hipLaunchKernelGGL(pg_check_kernel, dim3(blocks_for(std::max(N, E))), dim3(kBlock), 0, st, gr, nodes, n, transforms, informations, e,
                     w.gs, bad);
  hipLaunchKernelGGL(pg_marg_linearize_kernel, dim3(blocks_for(E)), dim3(kBlock), 0, st, gr, e, nodes, transforms, informations, weights,
                     w.gs, w.Haa, w.Hab, w.Hbb, w.ga, w.gb, bad);
  hipLaunchKernelGGL(pg_direct_blocks_kernel, dim3(static_cast<unsigned>(G)), dim3(kBlock), 0, st, gr, p, w.gs, w.Haa, w.Hab, w.Hbb, w.ga,
                     w.gb, w.D, w.bv, w.xv, w.rv, w.Wc, dp.fail, bad);
  if (runs > 0) hipLaunchKernelGGL(pg_direct_factor_kernel, dim3((runs + kWave - 1) / kWave), dim3(kWave), 0, st, dp, sy, runs, w.gs, bad);
  if (couplings > 0)
    hipLaunchKernelGGL(pg_direct_border_kernel, dim3(blocks_for(6ll * couplings)), dim3(kBlock), 0, st, dp, sy, couplings, w.gs, bad);
  if (items > 0) hipLaunchKernelGGL(pg_direct_schur_kernel, dim3(blocks_for(items)), dim3(kBlock), 0, st, dp, sy, g, items, w.gs, bad);
  hipLaunchKernelGGL(pg_marg_separator_kernel, dim3(static_cast<unsigned>(G)), dim3(kBlock), 0, st, dp, mg, w.gs, bad);
  if (runs > 0) {
    if (t_marg_ticks != nullptr)
      hipLaunchKernelGGL(pg_marg_sweep_kernel<true>, dim3(runs), dim3(kWave), 0, st, dp, sy, mg, w.gs, bad, t_marg_ticks);
    else
      hipLaunchKernelGGL(pg_marg_sweep_kernel<false>, dim3(runs), dim3(kWave), 0, st, dp, sy, mg, w.gs, bad, static_cast<long long*>(nullptr));
  }
  hipLaunchKernelGGL(pg_report_kernel, dim3(1), dim3(64), 0, st, g, w.gs, bad, w.report, failed);
}

// The end of both calls: the report and the runs' failure words read back; RDM_ERR_ARG for the first graph with a status, else
// `out` [G, 2] for report_host.
int read_marginals_report(const char* who, hipStream_t st, const Work& w, const Direct& dp, const DirectPlan& plan, int64_t G,
                          std::vector<double>& out) {
  std::vector<double> report(kReport * static_cast<size_t>(G));
  std::vector<int> fail(static_cast<size_t>(G));
  RDM_HIP_CHECK(hipMemcpyAsync(report.data(), w.report, sizeof(double) * kReport * G, hipMemcpyDeviceToHost, st));
  RDM_HIP_CHECK(hipMemcpyAsync(fail.data(), dp.fail, sizeof(int) * G, hipMemcpyDeviceToHost, st));
  RDM_HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t q = 0; q < G; ++q) {
    const int status = static_cast<int>(report[q * kReport + 5]);
    if (status == ST_OK) continue;
    set_error("%s: graph %lld: %s", who, static_cast<long long>(q), status_text(status));
    return RDM_ERR_ARG;
  }
  out.resize(2 * static_cast<size_t>(G));
  for (int64_t q = 0; q < G; ++q) {
    out[2 * q] = fail[q] != 0 ? ST_SINGULAR : ST_OK;
    out[2 * q + 1] = plan.sep_off[q + 1] - plan.sep_off[q];
  }
  return RDM_OK;
}

}  // namespace
}  // namespace rdm

extern "C" int rdm_pose_graph_edge_terms_host(const double* source_pose, const double* target_pose, const double* transform,
                                              const double* information, double line_process_weight, int uncertain, double* out) {
  using namespace rdm;
  RDM_REQUIRE(source_pose && target_pose && transform && information && out, "rdm_pose_graph_edge_terms_host: null argument");
  if (!edge_terms(source_pose, target_pose, transform, information, line_process_weight, uncertain != 0, out, out + 1, out + 8,
                  out + 44, out + 80, out + 116, out + 122, out + 2)) {
    set_error("rdm_pose_graph_edge_terms_host: the residual rotation is beyond the supported angle");
    return RDM_ERR_ARG;
  }
  return RDM_OK;
}

extern "C" int rdm_pose_graph_retract_host(const double* pose, const double* delta, double* out) {
  using namespace rdm;
  RDM_REQUIRE(pose && delta && out, "rdm_pose_graph_retract_host: null argument");
  retract(pose, delta, out);
  return RDM_OK;
}

extern "C" int rdm_pose_graph_chain_host(int64_t n, const double* diag, const double* off, const double* rhs, double* out) {
  using namespace rdm;
  RDM_REQUIRE(n >= 0 && n < kMaxTotal, "rdm_pose_graph_chain_host: bad number of nodes");
  if (n == 0) return RDM_OK;
  RDM_REQUIRE(diag && rhs && out && (off || n == 1), "rdm_pose_graph_chain_host: null argument");
  // the chain is one run of the direct solve without a separator: nodes 0 .. n - 1, no coupling
  const size_t N = static_cast<size_t>(n);
  std::vector<double> F(21 * N), Wc(36 * N, 0.0), zv(6 * N);
  for (size_t i = 1; i < N; ++i)  // M_{i,i-1} is the transpose of block (i - 1, i)
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) Wc[36 * i + 6 * r + c] = off[36 * (i - 1) + 6 * c + r];
  const int run_begin = 0, run_len = static_cast<int>(n), cpl_off[2] = {0, 0};
  Direct dp = {};
  dp.run_begin = &run_begin;
  dp.run_len = &run_len;
  dp.cpl_off = cpl_off;
  DirectSystem sy = {};
  sy.D = diag;
  sy.rv = rhs;
  sy.F = F.data();
  sy.Wc = Wc.data();
  sy.zv = zv.data();
  sy.xv = out;
  int failed = -1;
  if (!direct_run_factor(dp, sy, 1.0, 0, &failed)) {
    set_error("rdm_pose_graph_chain_host: the pivot of node %d is not positive definite", failed);
    return RDM_ERR_ARG;
  }
  direct_run_back(dp, sy, 0);
  return RDM_OK;
}

extern "C" int rdm_pose_graph_direct_max_separator(void) { return rdm::kMaxSeparator; }

extern "C" int64_t rdm_pose_graph_separator_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, int64_t* out_nodes,
                                                 int64_t capacity) {
  using namespace rdm;
  if (n_nodes < 0 || n_edges < 0 || (n_edges > 0 && edges_host == nullptr) || n_nodes > kMaxTotal) return -1;
  for (int64_t e = 0; e < n_edges; ++e) {
    const int64_t s = edges_host[2 * e], t = edges_host[2 * e + 1];
    if (s < 0 || s >= n_nodes || t < 0 || t >= n_nodes || s == t) return -1;
  }
  std::vector<int> S;
  choose_separator(n_nodes, n_edges, [&](int64_t e, int64_t& s, int64_t& t) { s = edges_host[2 * e]; t = edges_host[2 * e + 1]; }, S);
  for (size_t k = 0; k < S.size() && static_cast<int64_t>(k) < capacity && out_nodes != nullptr; ++k) out_nodes[k] = S[k];
  return static_cast<int64_t>(S.size());
}

extern "C" int rdm_pose_graph_direct_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, const double* diag,
                                          const double* off, const double* rhs, double* out) {
  using namespace rdm;
  RDM_REQUIRE(n_nodes >= 0 && n_nodes <= kMaxNodes && n_edges >= 0 && n_edges <= kMaxEdges, "rdm_pose_graph_direct_host: bad sizes");
  if (n_nodes == 0) return RDM_OK;
  RDM_REQUIRE(diag && rhs && out && ((edges_host && off) || n_edges == 0), "rdm_pose_graph_direct_host: null argument");
  HostDirect h;
  const int rc = host_direct_factor(h, n_nodes, n_edges, edges_host, diag, off, rhs, "rdm_pose_graph_direct_host", " (use the conjugate gradients)");
  if (rc != RDM_OK) return rc;
  const size_t N = static_cast<size_t>(n_nodes);
  const Direct& dp = h.dp;
  const DirectSystem& sy = h.sy;
  const DirectPlan& plan = h.plan;
  std::vector<double>& xv = h.xv;
  const int runs = h.runs, s = h.s;
  for (int u = 0; u < s; ++u) direct_schur_rhs(dp, sy, 0, u);
  std::vector<double> rs(6 * static_cast<size_t>(s) + 6);
  for (int u = 0; u < s; ++u)
    for (int k = 0; k < 6; ++k) rs[6 * u + k] = xv[6 * plan.sep_node[u] + k];
  auto block = [&](int i, int j) { return h.block(i, j); };
  for (int k = 0; k < s; ++k) {
    dense_lower_solve(block(k, k), &rs[6 * k]);
    for (int i = k + 1; i < s; ++i) dense_sub_mul(block(i, k), &rs[6 * k], &rs[6 * i], false);
  }
  for (int k = s - 1; k >= 0; --k) {
    dense_upper_solve(block(k, k), &rs[6 * k]);
    for (int j = 0; j < k; ++j) dense_sub_mul(block(k, j), &rs[6 * k], &rs[6 * j], true);
  }
  for (int u = 0; u < s; ++u)
    for (int k = 0; k < 6; ++k) xv[6 * plan.sep_node[u] + k] = rs[6 * u + k];
  for (int run = 0; run < runs; ++run) direct_run_back(dp, sy, run);
  for (int k = 0; k < 6; ++k) xv[k] = 0.0;
  memcpy(out, xv.data(), sizeof(double) * 6 * N);
  return RDM_OK;
}

extern "C" int rdm_pose_graph_marginals_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, const double* diag,
                                             const double* off, double* out) {
  using namespace rdm;
  RDM_REQUIRE(n_nodes >= 0 && n_nodes <= kMaxNodes && n_edges >= 0 && n_edges <= kMaxEdges, "rdm_pose_graph_marginals_host: bad sizes");
  if (n_nodes == 0) return RDM_OK;
  RDM_REQUIRE(diag && out && ((edges_host && off) || n_edges == 0), "rdm_pose_graph_marginals_host: null argument");
  const size_t N = static_cast<size_t>(n_nodes);
  const std::vector<double> rhs(6 * N, 0.0);  // (the runs' factor also sweeps a right-hand side)
  HostDirect h;
  const int rc = host_direct_factor(h, n_nodes, n_edges, edges_host, diag, off, rhs.data(), "rdm_pose_graph_marginals_host", "");
  if (rc != RDM_OK) return rc;
  const int s = h.s;
  std::vector<double> Z(h.C.size(), 0.0), P(36 * static_cast<size_t>(h.couplings) + 36, 0.0), S(36 * N, 0.0);
  const Marginals mg = {Z.data(), P.data(), S.data()};
  for (int t = 0; t < 6 * s; ++t) marg_inverse_column(h.C.data(), mg.Z, s, t / 6, t % 6);
  for (int u = 0; u < s; ++u)
    for (int v = 0; v <= u; ++v) marg_sigma_block(mg.Z, h.C.data(), s, u, v);
  for (int u = 0; u < s; ++u) memcpy(mg.S + 36 * static_cast<size_t>(h.plan.sep_node[u]), h.block(u, u), sizeof(double) * 36);
  for (int run = 0; run < h.runs; ++run) marg_sweep_run_host(h.dp, h.sy, mg, run);
  for (size_t i = 0; i < N; ++i) marg_write_block(mg.S + 36 * i, i == 0, false, out + 36 * i);
  return RDM_OK;
}

extern "C" size_t rdm_pose_graph_marginals_workspace_bytes(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                                           const int64_t* graph_edge_offsets_host, const int64_t* edges_host) {
  using namespace rdm;
  auto checked = [&]() -> int {
    RDM_REQUIRE(n_graphs >= 0 && n_graphs < kMaxTotal && graph_node_offsets_host && graph_edge_offsets_host,
                "rdm_pose_graph_marginals_workspace_bytes: bad number of graphs or null offsets");
    const int rc = check_graphs(n_graphs, graph_node_offsets_host, graph_edge_offsets_host);
    if (rc != RDM_OK) return rc;
    RDM_REQUIRE(graph_edge_offsets_host[n_graphs] == 0 || edges_host, "rdm_pose_graph_marginals_workspace_bytes: null edges");
    return RDM_OK;
  };
  if (checked() != RDM_OK) return 0;
  std::vector<char> host;
  DirectPlan plan;
  if (build_host_tables(n_graphs, graph_node_offsets_host, graph_edge_offsets_host, edges_host, nullptr, host, &plan,
                        "rdm_pose_graph_marginals", "") != RDM_OK)
    return 0;
  Arena ar(nullptr, 0);
  Work w;
  Direct dp;
  Marginals mg;
  carve_marginals(ar, n_graphs, graph_node_offsets_host[n_graphs], graph_edge_offsets_host[n_graphs], w, plan, dp, mg);
  return ar.off;
}

extern "C" int rdm_dbg_pose_graph_marginals_ticks(long long* device_ticks) {
  rdm::t_marg_ticks = device_ticks;
  return rdm::RDM_OK;
}

extern "C" int rdm_pose_graph_marginals(int64_t n_graphs, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                                        const double* nodes, const int64_t* edges_host, const double* transforms,
                                        const double* informations, const double* weights, double* covariances_out, double* report_host,
                                        void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  const int64_t G = n_graphs;
  RDM_REQUIRE(G >= 0 && G < kMaxTotal, "rdm_pose_graph_marginals: bad number of graphs");
  RDM_REQUIRE(G == 0 || (graph_node_offsets_host && graph_edge_offsets_host && report_host), "rdm_pose_graph_marginals: null argument");
  if (G == 0) return RDM_OK;
  int rc = check_graphs(G, graph_node_offsets_host, graph_edge_offsets_host);
  if (rc != RDM_OK) return rc;
  const int64_t N = graph_node_offsets_host[G], E = graph_edge_offsets_host[G];
  RDM_REQUIRE((nodes && covariances_out) || N == 0, "rdm_pose_graph_marginals: null nodes");
  RDM_REQUIRE((edges_host && transforms && informations) || E == 0, "rdm_pose_graph_marginals: null edges");
  std::vector<char> host;
  DirectPlan plan;
  rc = build_host_tables(G, graph_node_offsets_host, graph_edge_offsets_host, edges_host, nullptr, host, &plan, "rdm_pose_graph_marginals", "");
  if (rc != RDM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  Direct dp;
  Marginals mg;
  if (!carve_marginals(ar, G, N, E, w, plan, dp, mg)) {
    set_error("rdm_pose_graph_marginals: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  RDM_HIP_CHECK(hipMemcpyAsync(w.node_off, host.data(), host.size(), hipMemcpyHostToDevice, st));
  RDM_HIP_CHECK(hipStreamSynchronize(st));  // (`host` is pageable and leaves scope)
  const Graphs gr = {w.node_off, w.edge_off, w.edge_graph, w.node_graph, w.es, w.et, nullptr, w.inc_off, w.inc};
  enqueue_marginals(st, gr, w, dp, mg, plan, G, N, E, nodes, transforms, informations, weights);
  hipLaunchKernelGGL(pg_marg_finish_kernel, dim3(blocks_for(N)), dim3(kBlock), 0, st, gr, static_cast<int>(N), dp.fail, w.flags + 2, mg.S,
                     covariances_out);
  rc = launch_status("rdm_pose_graph_marginals");
  if (rc != RDM_OK) return rc;
  std::vector<double> report;
  rc = read_marginals_report("rdm_pose_graph_marginals", st, w, dp, plan, G, report);
  if (rc != RDM_OK) return rc;
  memcpy(report_host, report.data(), sizeof(double) * report.size());
  return RDM_OK;
}

extern "C" int rdm_pose_graph_pair_terms_host(const double* source_pose, const double* target_pose, const double* transform,
                                              const double* information, const double* cov_ss, const double* cov_tt, const double* cov_st,
                                              double* out) {
  using namespace rdm;
  RDM_REQUIRE(source_pose && target_pose && transform && cov_ss && cov_tt && cov_st && out, "rdm_pose_graph_pair_terms_host: null argument");
  double d2 = NAN;
  const int status = pair_terms(source_pose, target_pose, transform, information, cov_ss, cov_tt, cov_st, out, out + 6, &d2);
  if (status < 0) {
    set_error("rdm_pose_graph_pair_terms_host: the residual rotation is beyond the supported angle");
    return RDM_ERR_ARG;
  }
  out[42] = d2;
  out[43] = status;
  return RDM_OK;
}

extern "C" int rdm_pose_graph_pair_covariances_host(int64_t n_nodes, int64_t n_edges, const int64_t* edges_host, const double* diag,
                                                    const double* off, int64_t n_pairs, const int64_t* pairs_host, double* out) {
  using namespace rdm;
  const char* who = "rdm_pose_graph_pair_covariances_host";
  RDM_REQUIRE(n_nodes >= 0 && n_nodes <= kMaxNodes && n_edges >= 0 && n_edges <= kMaxEdges && n_pairs >= 0 && n_pairs < kMaxTotal / 36,
              "%s: bad sizes", who);
  if (n_pairs == 0) return RDM_OK;
  RDM_REQUIRE(diag && out && pairs_host && ((edges_host && off) || n_edges == 0), "%s: null argument", who);
  const size_t N = static_cast<size_t>(n_nodes), P = static_cast<size_t>(n_pairs);
  const std::vector<double> rhs(6 * (N > 0 ? N : 1), 0.0);
  HostDirect h;
  PairPlan pl;
  const int64_t poff[2] = {0, n_pairs};
  int rc = RDM_OK;
  if (n_nodes > 0) rc = host_direct_factor(h, n_nodes, n_edges, edges_host, diag, off, rhs.data(), who, "");
  if (rc != RDM_OK) return rc;
  const int noff[2] = {0, static_cast<int>(n_nodes)};
  if (n_nodes == 0) {
    h.plan = DirectPlan();
    h.plan.sep_off = {0, 0};
    h.plan.cpl_off = {0};
  }
  if (!build_pair_plan(1, noff, h.plan, poff, pairs_host, pl, who)) return RDM_ERR_ARG;
  const int s = h.s;
  std::vector<double> Z(h.C.size(), 0.0);
  for (int t = 0; t < 6 * s; ++t) marg_inverse_column(h.C.data(), Z.data(), s, t / 6, t % 6);
  for (int u = 0; u < s; ++u)
    for (int v = 0; v <= u; ++v) marg_sigma_block(Z.data(), h.C.data(), s, u, v);
  const size_t cols = std::min<size_t>(pl.col_node.size() > 0 ? pl.col_node.size() : 1, kColumnsInFlight);
  std::vector<double> yf(36 * cols * pl.y_stride), us(36 * cols * pl.u_stride), xs(36 * cols * pl.x_stride), cross(36 * (P + 1), 0.0);
  Pairs pp = {};
  for_each_pair_table(pl, pp, [](const std::vector<int>& v, const int*& table) { table = v.empty() ? nullptr : v.data(); });
  pp.y_stride = pl.y_stride;
  pp.u_stride = pl.u_stride;
  pp.x_stride = pl.x_stride;
  pp.yf = yf.data();
  pp.us = us.data();
  pp.xs = xs.data();
  pp.cross = cross.data();
  const int K = static_cast<int>(pl.col_node.size());
  for (int chunk = 0; chunk + 1 < static_cast<int>(pl.chunk_grp.size()); ++chunk) {  // a chunk's items in the kernels' order
    const int k0 = chunk * kColumnsInFlight, n = std::min(K - k0, kColumnsInFlight);
    for (int q = 0; q < n; ++q)
      for (int c = 0; c < 6; ++c) cons_forward_column(h.dp, h.sy, pp, k0 + q, q, c);
    for (int q = 0; q < n; ++q)
      for (int v = 0; v < s; ++v)
        for (int c = 0; c < 6; ++c) cons_separator_column(h.dp, pp, h.C.data(), s, 0, k0 + q, q, v, c);
    for (int r = pl.chunk_grp[chunk]; r < pl.chunk_grp[chunk + 1]; ++r)
      for (int c = 0; c < 6; ++c) cons_back_column(h.dp, h.sy, pp, 0, r, pl.grp_col[r] - k0, c);
  }
  for (size_t k = 0; k < P; ++k) {
    const bool zero = pl.pair_s[k] == 0 || pl.pair_t[k] == 0;
    for (int q = 0; q < 36; ++q) out[36 * k + q] = zero ? 0.0 : cross[36 * k + q];
  }
  return RDM_OK;
}

extern "C" size_t rdm_pose_graph_consistency_workspace_bytes(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                                             const int64_t* graph_edge_offsets_host, const int64_t* edges_host,
                                                             const int64_t* graph_pair_offsets_host, const int64_t* pairs_host) {
  using namespace rdm;
  std::vector<char> host;
  DirectPlan plan;
  PairPlan pairs;
  if (build_consistency_plans("rdm_pose_graph_consistency", n_graphs, graph_node_offsets_host, graph_edge_offsets_host, edges_host,
                              graph_pair_offsets_host, pairs_host, host, plan, pairs) != RDM_OK)
    return 0;
  Arena ar(nullptr, 0);
  Work w;
  Direct dp;
  Marginals mg;
  Pairs pp;
  void* tables;
  size_t tables_bytes;
  carve_marginals(ar, n_graphs, graph_node_offsets_host[n_graphs], graph_edge_offsets_host[n_graphs], w, plan, dp, mg);
  carve_pairs(ar, pairs, pp, &tables, &tables_bytes);
  return ar.off;
}

extern "C" int rdm_pose_graph_consistency(int64_t n_graphs, const int64_t* graph_node_offsets_host, const int64_t* graph_edge_offsets_host,
                                          const double* nodes, const int64_t* edges_host, const double* transforms,
                                          const double* informations, const double* weights, const int64_t* graph_pair_offsets_host,
                                          const int64_t* pairs_host, const double* pair_transforms, const double* pair_informations,
                                          double* covariances_out, double* cross_out, double* residual_cov_out, double* d2_out,
                                          uint8_t* pair_status_out, double* report_host, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  const char* who = "rdm_pose_graph_consistency";
  const int64_t G = n_graphs;
  RDM_REQUIRE(G >= 0 && G < kMaxTotal, "%s: bad number of graphs", who);
  if (G == 0) return RDM_OK;
  RDM_REQUIRE(report_host, "%s: null argument", who);
  std::vector<char> host;
  DirectPlan plan;
  PairPlan pairs;
  int rc = build_consistency_plans(who, G, graph_node_offsets_host, graph_edge_offsets_host, edges_host, graph_pair_offsets_host, pairs_host,
                                   host, plan, pairs);
  if (rc != RDM_OK) return rc;
  const int64_t N = graph_node_offsets_host[G], E = graph_edge_offsets_host[G], P = graph_pair_offsets_host[G];
  RDM_REQUIRE(nodes || N == 0, "%s: null nodes", who);
  RDM_REQUIRE((transforms && informations) || E == 0, "%s: null edges", who);
  RDM_REQUIRE(pair_transforms || P == 0, "%s: null pair transforms", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  Direct dp;
  Marginals mg;
  Pairs pp;
  void* tables = nullptr;
  size_t tables_bytes = 0;
  const bool fits = carve_marginals(ar, G, N, E, w, plan, dp, mg);
  if (!carve_pairs(ar, pairs, pp, &tables, &tables_bytes) || !fits) {
    set_error("%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  std::vector<char> pair_host(tables_bytes, 0);
  {  // the pairs' tables in a host buffer laid out as the workspace's part
    Arena hs(pair_host.data(), pair_host.size());
    Pairs hp;
    for_each_pair_table(pairs, hp, [&](const std::vector<int>& v, const int*& table) {
      int* dst = hs.take<int>(v.size() > 0 ? v.size() : 1);
      if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(int));
      table = dst;
    });
  }
  RDM_HIP_CHECK(hipMemcpyAsync(w.node_off, host.data(), host.size(), hipMemcpyHostToDevice, st));
  RDM_HIP_CHECK(hipMemcpyAsync(tables, pair_host.data(), pair_host.size(), hipMemcpyHostToDevice, st));
  RDM_HIP_CHECK(hipStreamSynchronize(st));  // (the host buffers are pageable and leave scope)
  const Graphs gr = {w.node_off, w.edge_off, w.edge_graph, w.node_graph, w.es, w.et, nullptr, w.inc_off, w.inc};
  const DirectSystem sy = {w.es, w.et, w.inc_off, w.inc, w.D, w.Hab, w.rv, w.F, w.Wc, w.zv, w.xv};
  int *bad = w.flags, *failed = w.flags + 2;
  const int p_total = static_cast<int>(P);
  enqueue_marginals(st, gr, w, dp, mg, plan, G, N, E, nodes, transforms, informations, weights);
  fill_words<unsigned long long>(pp.bad_pair, 1, ~0ull, st);
  fill_words<double>(pp.cross + 36 * P, 36, 0.0, st);
  if (P > 0)
    hipLaunchKernelGGL(pg_cons_check_kernel, dim3(blocks_for(P)), dim3(kBlock), 0, st, pp, p_total, nodes, pair_transforms, pair_informations,
                       bad, failed);
  if (covariances_out != nullptr)
    hipLaunchKernelGGL(pg_marg_finish_kernel, dim3(blocks_for(N)), dim3(kBlock), 0, st, gr, static_cast<int>(N), dp.fail, failed, mg.S,
                       covariances_out);
  const int K = static_cast<int>(pairs.col_node.size());
  for (int chunk = 0; chunk + 1 < static_cast<int>(pairs.chunk_grp.size()); ++chunk) {  // (on the stream: no read-back between chunks)
    const int k0 = chunk * kColumnsInFlight, cols = std::min(K - k0, kColumnsInFlight);
    const int r0 = pairs.chunk_grp[chunk], groups = pairs.chunk_grp[chunk + 1] - r0;
    hipLaunchKernelGGL(pg_cons_forward_kernel, dim3(blocks_for(6ll * cols)), dim3(kBlock), 0, st, gr, dp, sy, pp, k0, cols, w.gs, bad);
    hipLaunchKernelGGL(pg_cons_separator_kernel, dim3(blocks_for(6ll * cols * pp.x_stride)), dim3(kBlock), 0, st, gr, dp, pp, k0, cols, w.gs,
                       bad);
    hipLaunchKernelGGL(pg_cons_back_kernel, dim3(blocks_for(6ll * groups)), dim3(kBlock), 0, st, gr, dp, sy, pp, k0, r0, groups, w.gs, bad);
  }
  if (P > 0)
    hipLaunchKernelGGL(pg_cons_pair_kernel, dim3(static_cast<unsigned>((P + kWave - 1) / kWave)), dim3(kWave), 0, st, gr, pp, p_total, nodes,
                       pair_transforms, pair_informations, dp.fail, failed, mg.S, cross_out, residual_cov_out, d2_out, pair_status_out);
  rc = launch_status(who);
  if (rc != RDM_OK) return rc;
  unsigned long long bad_pair = ~0ull;
  RDM_HIP_CHECK(hipMemcpyAsync(&bad_pair, pp.bad_pair, sizeof(bad_pair), hipMemcpyDeviceToHost, st));
  std::vector<double> report;
  rc = read_marginals_report(who, st, w, dp, plan, G, report);
  if (rc != RDM_OK) return rc;
  if (bad_pair != ~0ull) {
    set_error("%s: pair %llu: %s", who, bad_pair >> 3, status_text(static_cast<int>(bad_pair & 7)));
    return RDM_ERR_ARG;
  }
  memcpy(report_host, report.data(), sizeof(double) * report.size());
  return RDM_OK;
}

extern "C" size_t rdm_pose_graph_workspace_bytes_ls(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                                    const int64_t* graph_edge_offsets_host, const int64_t* edges_host, int preconditioner,
                                                    int linear_solver) {
  using namespace rdm;
  auto checked = [&]() -> int {
    RDM_REQUIRE(linear_solver == SOLVER_PCG || linear_solver == SOLVER_DIRECT,
                "rdm_pose_graph_workspace_bytes_ls: linear_solver %d (0: conjugate gradients, 1: direct)", linear_solver);
    RDM_REQUIRE(n_graphs >= 0 && n_graphs < kMaxTotal && graph_node_offsets_host && graph_edge_offsets_host,
                "rdm_pose_graph_workspace_bytes_ls: bad number of graphs or null offsets");
    return check_graphs(n_graphs, graph_node_offsets_host, graph_edge_offsets_host);
  };
  if (checked() != RDM_OK) return 0;
  const int64_t N = graph_node_offsets_host[n_graphs], E = graph_edge_offsets_host[n_graphs];
  if (linear_solver == SOLVER_PCG) return rdm_pose_graph_workspace_bytes_pc(n_graphs, N, E, preconditioner);
  if (E > 0 && edges_host == nullptr) {
    set_error("rdm_pose_graph_workspace_bytes_ls: null edges");
    return 0;
  }
  std::vector<char> host;
  DirectPlan plan;
  if (build_host_tables(n_graphs, graph_node_offsets_host, graph_edge_offsets_host, edges_host, nullptr, host, &plan) != RDM_OK) return 0;
  Arena ar(nullptr, 0);
  Work w;
  Direct dp;
  carve(ar, n_graphs, N, E, PRE_BLOCK_JACOBI, w, &plan, &dp);
  return ar.off;
}

extern "C" size_t rdm_pose_graph_workspace_bytes_pc(int64_t n_graphs, int64_t n_nodes, int64_t n_edges, int preconditioner) {
  using namespace rdm;
  Arena ar(nullptr, 0);
  Work w;
  carve(ar, n_graphs, n_nodes, n_edges, preconditioner, w);
  return ar.off;
}

extern "C" size_t rdm_pose_graph_workspace_bytes(int64_t n_graphs, int64_t n_nodes, int64_t n_edges) {
  return rdm_pose_graph_workspace_bytes_pc(n_graphs, n_nodes, n_edges, 0);
}

extern "C" int rdm_pose_graph_optimize(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                       const int64_t* graph_edge_offsets_host, const double* nodes, const int64_t* edges_host,
                                       const double* transforms, const double* informations, const uint8_t* uncertain_host,
                                       double line_process_weight, double edge_prune_threshold, int max_iterations,
                                       double gradient_tolerance, double cost_tolerance, int pcg_max_iterations, double pcg_tolerance,
                                       double* nodes_out, double* weights_out, uint8_t* pruned_out, double* report_host, void* ws,
                                       size_t ws_bytes, void* stream) {
  return rdm_pose_graph_optimize_pc(n_graphs, graph_node_offsets_host, graph_edge_offsets_host, nodes, edges_host, transforms,
                                    informations, uncertain_host, line_process_weight, edge_prune_threshold, max_iterations,
                                    gradient_tolerance, cost_tolerance, pcg_max_iterations, pcg_tolerance, 0, nodes_out, weights_out,
                                    pruned_out, report_host, ws, ws_bytes, stream);
}

extern "C" int rdm_pose_graph_optimize_pc(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                          const int64_t* graph_edge_offsets_host, const double* nodes, const int64_t* edges_host,
                                          const double* transforms, const double* informations, const uint8_t* uncertain_host,
                                          double line_process_weight, double edge_prune_threshold, int max_iterations,
                                          double gradient_tolerance, double cost_tolerance, int pcg_max_iterations,
                                          double pcg_tolerance, int preconditioner, double* nodes_out, double* weights_out,
                                          uint8_t* pruned_out, double* report_host, void* ws, size_t ws_bytes, void* stream) {
  return rdm_pose_graph_optimize_ls(n_graphs, graph_node_offsets_host, graph_edge_offsets_host, nodes, edges_host, transforms,
                                    informations, uncertain_host, line_process_weight, edge_prune_threshold, max_iterations,
                                    gradient_tolerance, cost_tolerance, pcg_max_iterations, pcg_tolerance, preconditioner, 0, nodes_out,
                                    weights_out, pruned_out, report_host, ws, ws_bytes, stream);
}

extern "C" int rdm_pose_graph_optimize_ls(int64_t n_graphs, const int64_t* graph_node_offsets_host,
                                          const int64_t* graph_edge_offsets_host, const double* nodes, const int64_t* edges_host,
                                          const double* transforms, const double* informations, const uint8_t* uncertain_host,
                                          double line_process_weight, double edge_prune_threshold, int max_iterations,
                                          double gradient_tolerance, double cost_tolerance, int pcg_max_iterations,
                                          double pcg_tolerance, int preconditioner, int linear_solver, double* nodes_out,
                                          double* weights_out, uint8_t* pruned_out, double* report_host, void* ws, size_t ws_bytes,
                                          void* stream) {
  using namespace rdm;
  const int64_t G = n_graphs;
  RDM_REQUIRE(linear_solver == SOLVER_PCG || linear_solver == SOLVER_DIRECT,
              "rdm_pose_graph_optimize: linear_solver %d (0: conjugate gradients, 1: direct)", linear_solver);
  const bool direct = linear_solver == SOLVER_DIRECT;
  if (direct) preconditioner = PRE_BLOCK_JACOBI;  // (ignored)
  RDM_REQUIRE(preconditioner == PRE_BLOCK_JACOBI || preconditioner == PRE_CHAIN,
              "rdm_pose_graph_optimize: preconditioner %d (0: block-Jacobi, 1: the odometry chain)", preconditioner);
  RDM_REQUIRE(G >= 0 && G < kMaxTotal, "rdm_pose_graph_optimize: bad number of graphs");
  RDM_REQUIRE(G == 0 || (graph_node_offsets_host && graph_edge_offsets_host && report_host), "rdm_pose_graph_optimize: null argument");
  RDM_REQUIRE(max_iterations >= 0 && gradient_tolerance >= 0.0 && cost_tolerance >= 0.0 && pcg_max_iterations >= 0 &&
                  pcg_tolerance >= 0.0 && std::isfinite(pcg_tolerance) && !(line_process_weight != line_process_weight) &&
                  std::isfinite(edge_prune_threshold),
              "rdm_pose_graph_optimize: bad options");
  if (G == 0) return RDM_OK;
  int rc = check_graphs(G, graph_node_offsets_host, graph_edge_offsets_host);
  if (rc != RDM_OK) return rc;
  const int64_t N = graph_node_offsets_host[G], E = graph_edge_offsets_host[G];
  RDM_REQUIRE((nodes && nodes_out) || N == 0, "rdm_pose_graph_optimize: null nodes");
  RDM_REQUIRE((edges_host && transforms && informations) || E == 0, "rdm_pose_graph_optimize: null edges");
  // the integer tables, and with the direct solve its separators, runs and coupling lists behind them
  std::vector<char> host;
  DirectPlan plan;
  rc = build_host_tables(G, graph_node_offsets_host, graph_edge_offsets_host, edges_host, uncertain_host, host, direct ? &plan : nullptr);
  if (rc != RDM_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  Direct dp;
  if (!carve(ar, G, N, E, preconditioner, w, direct ? &plan : nullptr, &dp)) {
    set_error("rdm_pose_graph_optimize: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  RDM_HIP_CHECK(hipMemcpyAsync(w.node_off, host.data(), host.size(), hipMemcpyHostToDevice, st));
  RDM_HIP_CHECK(hipStreamSynchronize(st));  // (`host` is pageable and leaves scope)
  Graphs gr = {w.node_off, w.edge_off, w.edge_graph, w.node_graph, w.es, w.et, uncertain_host ? w.uncertain : nullptr, w.inc_off, w.inc};
  Params p;
  p.mu = line_process_weight;
  p.prune = edge_prune_threshold;
  p.gtol = gradient_tolerance;
  p.ctol = cost_tolerance;
  p.pcg_tol = pcg_tolerance;
  p.max_iterations = max_iterations;
  p.pcg_cap = pcg_max_iterations;
  int *bad = w.flags, *remaining = w.flags + 1, *failed = w.flags + 2;
  const int n = static_cast<int>(N), e = static_cast<int>(E), g = static_cast<int>(G);
  const int64_t widest = std::max<int64_t>(std::max<int64_t>(16 * N, E), G);
  const DirectSystem sy = {w.es, w.et, w.inc_off, w.inc, w.D, w.Hab, w.rv, w.F, w.Wc, w.zv, w.xv};
  const int runs = direct ? static_cast<int>(plan.run_begin.size()) : 0, couplings = direct ? static_cast<int>(plan.cpl_sep.size()) : 0;
  const long long items = direct ? plan.item_off.back() : 0;
  fill_words<int>(w.flags, 4, 0, st);
  hipLaunchKernelGGL(pg_init_kernel, dim3(blocks_for(widest)), dim3(kBlock), 0, st, nodes, n, w.X, w.Xc, w.gs, g, w.node_off, w.edge_off);
  hipLaunchKernelGGL(pg_check_kernel, dim3(blocks_for(std::max(N, E))), dim3(kBlock), 0, st, gr, nodes, n, transforms, informations, e,
                     w.gs, bad);
  hipLaunchKernelGGL(pg_cost_kernel, dim3(blocks_for(E)), dim3(kBlock), 0, st, gr, e, w.X, transforms, informations, p, w.gs, 0, w.term,
                     w.lw, bad);
  hipLaunchKernelGGL(pg_step_kernel, dim3(1), dim3(kBlock), 0, st, gr, g, p, 0, w.term, w.gs, remaining, bad);
  rc = launch_status("rdm_pose_graph_optimize (setup)");
  if (rc != RDM_OK) return rc;
  int left = 1;
  for (int k = 0; k < max_iterations && left > 0;) {
    const int end = std::min(max_iterations, k + kChunk);
    for (; k < end; ++k) {
      hipLaunchKernelGGL(pg_linearize_kernel, dim3(blocks_for(E)), dim3(kBlock), 0, st, gr, e, w.X, transforms, informations, p, w.gs,
                         w.lw, w.Haa, w.Hab, w.Hbb, w.ga, w.gb, bad);
      if (direct) {
        hipLaunchKernelGGL(pg_direct_blocks_kernel, dim3(static_cast<unsigned>(G)), dim3(kBlock), 0, st, gr, p, w.gs, w.Haa, w.Hab, w.Hbb,
                           w.ga, w.gb, w.D, w.bv, w.xv, w.rv, w.Wc, dp.fail, bad);
        if (runs > 0)
          hipLaunchKernelGGL(pg_direct_factor_kernel, dim3((runs + kWave - 1) / kWave), dim3(kWave), 0, st, dp, sy, runs, w.gs, bad);
        if (couplings > 0)
          hipLaunchKernelGGL(pg_direct_border_kernel, dim3(blocks_for(6ll * couplings)), dim3(kBlock), 0, st, dp, sy, couplings, w.gs, bad);
        if (items > 0)
          hipLaunchKernelGGL(pg_direct_schur_kernel, dim3(blocks_for(items)), dim3(kBlock), 0, st, dp, sy, g, items, w.gs, bad);
        hipLaunchKernelGGL(pg_direct_solve_kernel, dim3(static_cast<unsigned>(G)), dim3(kBlock), 0, st, dp, sy, w.gs, bad);
      } else {
        hipLaunchKernelGGL(preconditioner == PRE_CHAIN ? pg_solve_kernel<PRE_CHAIN> : pg_solve_kernel<PRE_BLOCK_JACOBI>,
                           dim3(static_cast<unsigned>(G)), dim3(kBlock), 0, st, gr, p, w.gs, w.Haa, w.Hab, w.Hbb, w.ga, w.gb, w.D, w.F,
                           w.bv, w.xv, w.rv, w.zv, w.pv, bad, w.Wc);
      }
      hipLaunchKernelGGL(pg_update_kernel, dim3(blocks_for(N)), dim3(kBlock), 0, st, gr, n, w.gs, w.X, w.xv, w.Xc, bad);
      hipLaunchKernelGGL(pg_cost_kernel, dim3(blocks_for(E)), dim3(kBlock), 0, st, gr, e, w.Xc, transforms, informations, p, w.gs, 0,
                         w.term, static_cast<double*>(nullptr), bad);
      hipLaunchKernelGGL(pg_step_kernel, dim3(1), dim3(kBlock), 0, st, gr, g, p, 1, w.term, w.gs, remaining, bad);
      hipLaunchKernelGGL(pg_commit_kernel, dim3(blocks_for(N)), dim3(kBlock), 0, st, gr, n, w.gs, w.X, w.Xc, bad);
    }
    rc = launch_status("rdm_pose_graph_optimize");
    if (rc != RDM_OK) return rc;
    RDM_HIP_CHECK(hipMemcpyAsync(&left, remaining, sizeof(int), hipMemcpyDeviceToHost, st));  // one word per chunk
    RDM_HIP_CHECK(hipStreamSynchronize(st));
  }
  // the weights at the final poses (the linearisation's are those before the last step)
  hipLaunchKernelGGL(pg_cost_kernel, dim3(blocks_for(E)), dim3(kBlock), 0, st, gr, e, w.X, transforms, informations, p, w.gs, 1, w.term,
                     w.lw, bad);
  hipLaunchKernelGGL(pg_report_kernel, dim3(1), dim3(64), 0, st, g, w.gs, bad, w.report, failed);
  hipLaunchKernelGGL(pg_finish_kernel, dim3(blocks_for(widest)), dim3(kBlock), 0, st, gr, n, e, p, w.gs, failed, w.X, w.lw, nodes_out,
                     weights_out, pruned_out);
  rc = launch_status("rdm_pose_graph_optimize (finish)");
  if (rc != RDM_OK) return rc;
  RDM_HIP_CHECK(hipMemcpyAsync(report_host, w.report, sizeof(double) * kReport * G, hipMemcpyDeviceToHost, st));
  RDM_HIP_CHECK(hipStreamSynchronize(st));
  for (int64_t q = 0; q < G; ++q) {
    const int status = static_cast<int>(report_host[q * kReport + 5]);
    if (status == ST_OK) continue;
    set_error("rdm_pose_graph_optimize: graph %lld: %s", static_cast<long long>(q), status_text(status));
    return RDM_ERR_ARG;
  }
  return RDM_OK;
}
