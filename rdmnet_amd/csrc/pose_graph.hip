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
// the default) or, on request, by the exactly factored block tridiagonal part along the odometry chain), pg_update_kernel
// (candidate poses), pg_cost_kernel (candidate cost terms), pg_step_kernel (accept / reject, damping, stopping tests) and
// pg_commit_kernel.  All decisions are taken on the device; the host reads one word every kChunk iterations.
#include "common.h"
#include "../../include/rdmnet_hip.h"

#include <cmath>
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
enum : int { ST_OK = 0, ST_NONFINITE = 1, ST_ASYMMETRIC = 2, ST_ANGLE = 3, ST_SINGULAR = 4 };

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

// Everything one edge contributes: l, its cost term, and (times l) Haa = A^T L A, Hab = A^T L B, Hbb = B^T L B, ga = A^T L r,
// gb = B^T L r (and r itself into r_out, also beyond the limit), where A = d r / d(source perturbation) = [[Jr^-1, 0], [0, R_E]] and B = d r / d(target perturbation) =
// [[-Jr^-1 Rst^T, 0], [R_T^T [u]x, -R_T^T]] (right perturbations X <- X [Exp(dw) | dt]).  Returns false beyond the angle limit.
__host__ __device__ inline bool edge_terms(const double* Xs, const double* Xt, const double* T, const double* L, double mu,
                                           bool uncertain, double* l_out, double* term, double* Haa, double* Hab, double* Hbb,
                                           double* ga, double* gb, double* r_out = nullptr) {
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
  const double l = line_weight(q, mu, uncertain);
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
  const M3 Ja = jr_inv(r.w, r.theta2), Ra = r.Re;
  const M3 RT = rot_of(T);
  const M3 B11 = neg(mul(Ja, transpose(r.Rst))), B21 = tmul(RT, skew(r.u)), B22 = neg(transpose(RT));
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
  if (*bad != 0 || gs[g].done) return;  // (uniform over the workgroup)
  const int n0 = gr.node_off[g], n = gr.node_off[g + 1] - n0;
  const double lambda = gs[g].lambda;
  if (threadIdx.x == 0) fail = 0;
  __syncthreads();
  // 1. blocks, gradient, factors
  double gmax = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) {
    const long long node = n0 + i;
    double d[36], b[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) d[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = 0.0;
    [[maybe_unused]] double off[36];  // kPre 1: M_{i,i-1}, the edges that join this node and the one before it, in edge order
    if constexpr (kPre == PRE_CHAIN) {
#pragma unroll
      for (int k = 0; k < 36; ++k) off[k] = 0.0;
    }
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
        if constexpr (kPre == PRE_CHAIN) {
          const long long other = (code & 1) ? gr.es[e] : gr.et[e];
          if (i > 1 && other == node - 1) {
            const double* C = Hab + 36 * e;  // rows: the edge's source
            if (code & 1) {
#pragma unroll
              for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) off[6 * r + c] += C[6 * c + r];
            } else {
#pragma unroll
              for (int k = 0; k < 36; ++k) off[k] += C[k];
            }
          }
        }
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
    if constexpr (kPre == PRE_CHAIN) {
#pragma unroll
      for (int k = 0; k < 36; ++k) Wc[36 * node + k] = off[k];
    } else if (i > 0) {
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
    if (threadIdx.x == 0) {
      gs[g].status = ST_SINGULAR;
      gs[g].done = 1;
    }
    return;
  }
  if (threadIdx.x == 0) gs[g].grad_max = gmax;
  if (gmax <= p.gtol) {
    if (threadIdx.x == 0) {
      gs[g].stop = STOP_GRADIENT;
      gs[g].done = 1;
    }
    return;
  }
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
      if (threadIdx.x == 0) {
        gs[g].status = ST_SINGULAR;
        gs[g].done = 1;
      }
      return;
    }
    for (int i = threadIdx.x; i < n; i += kBlock)
      if (i > 1) chain_w(F + 21ll * (n0 + i), Wc + 36ll * (n0 + i), Wc + 36ll * (n0 + i));
  }
  // 2. z = M^-1 r, pv = z, rz
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
        pv[6 * node + k] = z[k];
        if (i > 0) part += r[k] * z[k];
      }
    }
  }
  if constexpr (kPre == PRE_CHAIN) {
    part = chain_finish(F, Wc, rv, zv, n0, n);
    for (int i = threadIdx.x; i < n; i += kBlock)
#pragma unroll
      for (int k = 0; k < 6; ++k) pv[6ll * (n0 + i) + k] = zv[6ll * (n0 + i) + k];
  }
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
        double x[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = pv[6 * node + k];
        const double* d = D + 36 * node;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double a = 0.0;
#pragma unroll
          for (int c = 0; c < 6; ++c) a += d[6 * r + c] * x[c];
          y[r] = (1.0 + lambda) * a;
        }
        for (int q = gr.inc_off[node]; q < gr.inc_off[node + 1]; ++q) {
          const int code = gr.inc[q];
          const long long e = code >> 1;
          const double* H = Hab + 36 * e;
          if (code & 1) {  // this node is the target: Hab^T p_source
            const double* o = pv + 6ll * gr.es[e];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
              double a = 0.0;
#pragma unroll
              for (int c = 0; c < 6; ++c) a += H[6 * c + r] * o[c];
              y[r] += a;
            }
          } else {
            const double* o = pv + 6ll * gr.et[e];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
              double a = 0.0;
#pragma unroll
              for (int c = 0; c < 6; ++c) a += H[6 * r + c] * o[c];
              y[r] += a;
            }
          }
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
    part = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) {
      const long long node = n0 + i;
      double r[6], z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        xv[6 * node + k] += alpha * pv[6 * node + k];
        r[k] = rv[6 * node + k] - alpha * zv[6 * node + k];
        rv[6 * node + k] = r[k];
      }
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
    const double rz_new = block_sum(part, red);
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
void carve_tables(Arena& ar, size_t G, size_t N, size_t E, Work& w) {
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

bool carve(Arena& ar, int64_t g, int64_t n, int64_t e, int preconditioner, Work& w) {
  const size_t G = static_cast<size_t>(g > 0 ? g : 1), N = static_cast<size_t>(n > 0 ? n : 1), E = static_cast<size_t>(e > 0 ? e : 1);
  carve_tables(ar, G, N, E, w);
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
  w.Wc = preconditioner == PRE_CHAIN ? ar.take<double>(36 * N) : nullptr;  // (last: the other slots lie where they lay)
  return ar.ok;
}

unsigned blocks_for(int64_t n) { return static_cast<unsigned>(((n > 0 ? n : 1) + kBlock - 1) / kBlock); }  // (n < 2^35: < 2^27 blocks)

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
  const size_t N = static_cast<size_t>(n);
  std::vector<double> G(21 * N), W(36 * N), v(6 * N);
  for (size_t i = 0; i < N; ++i) {
    double m[36], x[36];
    if (i > 0)  // M_{i,i-1} is the transpose of block (i - 1, i)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) m[6 * r + c] = off[36 * (i - 1) + 6 * c + r];
    if (!chain_factor_node(diag + 36 * i, i > 0 ? m : nullptr, i > 0 ? &G[21 * (i - 1)] : nullptr, &G[21 * i], x)) {
      set_error("rdm_pose_graph_chain_host: the pivot of node %zu is not positive definite", i);
      return RDM_ERR_ARG;
    }
    chain_w(&G[21 * i], x, &W[36 * i]);
  }
  double y[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (size_t i = 0; i < N; ++i) {  // c = G r, then the forward sweep
    double c[6];
    chain_g_mul(&G[21 * i], rhs + 6 * i, c);
    for (int r = 0; r < 6; ++r) v[6 * i + r] = chain_row(c[r], &W[36 * i + 6 * r], y);
    for (int r = 0; r < 6; ++r) y[r] = v[6 * i + r];
  }
  for (int r = 0; r < 6; ++r) y[r] = 0.0;
  for (size_t i = N; i-- > 0;) {  // the backward sweep on q = L_ii^T z, then z = G^T q
    double q[6];
    for (int r = 0; r < 6; ++r) {
      double col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (i + 1 < N)
        for (int c = 0; c < 6; ++c) col[c] = W[36 * (i + 1) + 6 * c + r];
      q[r] = chain_row(v[6 * i + r], col, y);
    }
    for (int r = 0; r < 6; ++r) y[r] = q[r];
    chain_gt_mul(&G[21 * i], q, out + 6 * i);
  }
  return RDM_OK;
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
  using namespace rdm;
  const int64_t G = n_graphs;
  RDM_REQUIRE(preconditioner == PRE_BLOCK_JACOBI || preconditioner == PRE_CHAIN,
              "rdm_pose_graph_optimize: preconditioner %d (0: block-Jacobi, 1: the odometry chain)", preconditioner);
  RDM_REQUIRE(G >= 0 && G < kMaxTotal, "rdm_pose_graph_optimize: bad number of graphs");
  RDM_REQUIRE(G == 0 || (graph_node_offsets_host && graph_edge_offsets_host && report_host), "rdm_pose_graph_optimize: null argument");
  RDM_REQUIRE(max_iterations >= 0 && gradient_tolerance >= 0.0 && cost_tolerance >= 0.0 && pcg_max_iterations >= 0 &&
                  pcg_tolerance >= 0.0 && std::isfinite(pcg_tolerance) && !(line_process_weight != line_process_weight) &&
                  std::isfinite(edge_prune_threshold),
              "rdm_pose_graph_optimize: bad options");
  if (G == 0) return RDM_OK;
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
  RDM_REQUIRE((nodes && nodes_out) || N == 0, "rdm_pose_graph_optimize: null nodes");
  RDM_REQUIRE((edges_host && transforms && informations) || E == 0, "rdm_pose_graph_optimize: null edges");
  // the integer tables: global node ids, graph of every node / edge, incidence lists by a counting sort
  Arena sizes(nullptr, 0);
  Work t;
  carve_tables(sizes, G, N > 0 ? N : 1, E > 0 ? E : 1, t);
  std::vector<char> host(sizes.off, 0);
  Arena har(host.data(), host.size());
  carve_tables(har, G, N > 0 ? N : 1, E > 0 ? E : 1, t);
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
  {
    std::vector<int> fill(inc_off, inc_off + N);
    for (int64_t e = 0; e < E; ++e) {  // ascending edge order per node
      inc[fill[es[e]]++] = static_cast<int>(2 * e);
      inc[fill[et[e]]++] = static_cast<int>(2 * e + 1);
    }
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, G, N, E, preconditioner, w)) {
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
  fill_words<int>(w.flags, 4, 0, st);
  hipLaunchKernelGGL(pg_init_kernel, dim3(blocks_for(widest)), dim3(kBlock), 0, st, nodes, n, w.X, w.Xc, w.gs, g, w.node_off, w.edge_off);
  hipLaunchKernelGGL(pg_check_kernel, dim3(blocks_for(std::max(N, E))), dim3(kBlock), 0, st, gr, nodes, n, transforms, informations, e,
                     w.gs, bad);
  hipLaunchKernelGGL(pg_cost_kernel, dim3(blocks_for(E)), dim3(kBlock), 0, st, gr, e, w.X, transforms, informations, p, w.gs, 0, w.term,
                     w.lw, bad);
  hipLaunchKernelGGL(pg_step_kernel, dim3(1), dim3(kBlock), 0, st, gr, g, p, 0, w.term, w.gs, remaining, bad);
  int rc = launch_status("rdm_pose_graph_optimize (setup)");
  if (rc != RDM_OK) return rc;
  int left = 1;
  for (int k = 0; k < max_iterations && left > 0;) {
    const int end = std::min(max_iterations, k + kChunk);
    for (; k < end; ++k) {
      hipLaunchKernelGGL(pg_linearize_kernel, dim3(blocks_for(E)), dim3(kBlock), 0, st, gr, e, w.X, transforms, informations, p, w.gs,
                         w.lw, w.Haa, w.Hab, w.Hbb, w.ga, w.gb, bad);
      hipLaunchKernelGGL(preconditioner == PRE_CHAIN ? pg_solve_kernel<PRE_CHAIN> : pg_solve_kernel<PRE_BLOCK_JACOBI>,
                         dim3(static_cast<unsigned>(G)), dim3(kBlock), 0, st, gr, p, w.gs, w.Haa, w.Hab, w.Hbb, w.ga, w.gb, w.D, w.F, w.bv,
                         w.xv, w.rv, w.zv, w.pv, bad, w.Wc);
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
    static const char* const what[] = {"", "a pose, transform or information entry is not finite", "an information matrix is not symmetric",
                                       "a residual rotation of the given poses is beyond the supported angle (cos < -0.99)",
                                       "a node's block is not positive definite (a node that no edge reaches, or an indefinite information matrix)"};
    set_error("rdm_pose_graph_optimize: graph %lld: %s", static_cast<long long>(q), what[status >= 1 && status <= 4 ? status : 0]);
    return RDM_ERR_ARG;
  }
  return RDM_OK;
}
