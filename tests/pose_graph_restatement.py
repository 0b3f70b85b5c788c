"""Pose-graph optimisation, restated in numpy float64 ("pose-graph optimisation").  The definition the
GPU solver (rdmnet_amd/csrc/pose_graph.hip, ops.pose_graph_optimize) is held against; it shares no code with it: the normal
equations are assembled densely and solved with np.linalg.solve.

Nodes X_i: 4 x 4, the pose of scan i in the frame of node 0 (fixed).  Edge (s, t, T, L, uncertain): T maps source-scan to
target-scan coordinates, the model is X_s = X_t T, L is the 6 x 6 information matrix (rotation first).  Residual
r = (Log R_E, t_E) of E = T^-1 X_t^-1 X_s; cost F = sum l r^T L r + mu (sqrt(l) - 1)^2 with l = 1 for certain edges and without a
line process, l = (mu / (mu + r^T L r))^2 else; update X <- X [Exp(dw) | dt]."""
import math

import numpy as np

SMALL_SIN = 1e-3        # below it (cos > 0) the rotation vector uses the series of asin(s) / s
SMALL_ANGLE2 = 1e-2     # below it the inverse right Jacobian and Exp use their series
MAX_COS = -0.99         # residual rotations beyond it are refused
LAMBDA0, LAMBDA_DOWN, LAMBDA_UP, LAMBDA_MIN, LAMBDA_MAX = 1e-6, 0.1, 10.0, 1e-12, 1e12
STOP_GRADIENT, STOP_COST, STOP_MAX_ITERATIONS, STOP_EMPTY = 1, 2, 3, 4


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_log(R):
    """-> (rotation vector, cos of the angle)."""
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = math.sqrt(float(a @ a))
    c = 0.5 * (np.trace(R) - 1.0)
    if s < SMALL_SIN and c > 0.0:
        f = 1.0 + s * s * (1.0 / 6.0 + s * s * (3.0 / 40.0))
    else:
        f = math.atan2(s, c) / s if s > 0.0 else 0.0
    return a * f, c


def so3_exp(w):
    t2 = float(w @ w)
    if t2 < SMALL_ANGLE2:
        a = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0 - t2 / 362880.0)))
        b = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0 - t2 / 3628800.0)))
    else:
        t = math.sqrt(t2)
        a = math.sin(t) / t
        b = 2.0 * math.sin(0.5 * t) ** 2 / t2
    W = skew(w)
    return np.eye(3) + a * W + b * (W @ W)


def jr_inv(w):
    """Inverse right Jacobian of SO(3): Log(Exp(w) Exp(d)) = w + jr_inv(w) d + O(d^2)."""
    t2 = float(w @ w)
    if t2 < SMALL_ANGLE2:
        k = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 / 1209600.0))
    else:
        t = math.sqrt(t2)
        k = 1.0 / t2 - (1.0 + math.cos(t)) / (2.0 * t * math.sin(t))
    W = skew(w)
    return np.eye(3) + 0.5 * W + k * (W @ W)


def retract(X, d):
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3] @ so3_exp(d[:3])
    Y[:3, 3] = X[:3, 3] + X[:3, :3] @ d[3:]
    return Y


def residual(Xs, Xt, T):
    """-> r [6]; raises beyond the angle limit."""
    Rs, Rt, RT = Xs[:3, :3], Xt[:3, :3], T[:3, :3]
    u = Rt.T @ (Xs[:3, 3] - Xt[:3, 3])
    v = RT.T @ (u - T[:3, 3])
    w, c = so3_log(RT.T @ (Rt.T @ Rs))
    if not c >= MAX_COS:
        raise ValueError('residual rotation beyond the supported angle')
    return np.concatenate([w, v])


def jacobians(Xs, Xt, T):
    """-> (r, A = dr / d(source perturbation), B = dr / d(target perturbation)), exact."""
    r = residual(Xs, Xt, T)
    Rs, Rt, RT = Xs[:3, :3], Xt[:3, :3], T[:3, :3]
    Rst = Rt.T @ Rs
    u = Rt.T @ (Xs[:3, 3] - Xt[:3, 3])
    J = jr_inv(r[:3])
    A = np.zeros((6, 6))
    A[:3, :3] = J
    A[3:, 3:] = RT.T @ Rst
    B = np.zeros((6, 6))
    B[:3, :3] = -J @ Rst.T
    B[3:, :3] = RT.T @ skew(u)
    B[3:, 3:] = -RT.T
    return r, A, B


def sym(L):
    return 0.5 * (L + L.T)


def weight(q, mu, uncertain):
    if mu is None or not uncertain:
        return 1.0
    return (mu / (mu + q)) ** 2


def edge_cost(q, l, mu, uncertain):
    if mu is None or not uncertain:
        return q
    return l * q + mu * (math.sqrt(l) - 1.0) ** 2


def weights(nodes, edges, transforms, informations, uncertain=None, line_process_weight=None):
    out = np.ones(len(edges))
    for e, (s, t) in enumerate(edges):
        r = residual(nodes[s], nodes[t], transforms[e])
        out[e] = weight(float(r @ sym(informations[e]) @ r), line_process_weight, uncertain is not None and uncertain[e])
    return out


def cost(nodes, edges, transforms, informations, uncertain=None, line_process_weight=None):
    """F at `nodes` with every l at its optimum there (math.fsum over the edges)."""
    terms = []
    for e, (s, t) in enumerate(edges):
        r = residual(nodes[s], nodes[t], transforms[e])
        q = float(r @ sym(informations[e]) @ r)
        unc = uncertain is not None and uncertain[e]
        terms.append(edge_cost(q, weight(q, line_process_weight, unc), line_process_weight, unc))
    return math.fsum(terms)


def normal_equations(nodes, edges, transforms, informations, uncertain=None, line_process_weight=None):
    """-> (H [6N, 6N], b [6N]) with l at the current poses: H = sum l J^T L J, b = sum l J^T L r (rows of node 0 included)."""
    n = len(nodes)
    H = np.zeros((6 * n, 6 * n))
    b = np.zeros(6 * n)
    for e, (s, t) in enumerate(edges):
        r, A, B = jacobians(nodes[s], nodes[t], transforms[e])
        L = sym(informations[e])
        l = weight(float(r @ L @ r), line_process_weight, uncertain is not None and uncertain[e])
        ss, tt = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
        H[ss, ss] += l * (A.T @ L @ A)
        H[ss, tt] += l * (A.T @ L @ B)
        H[tt, ss] += l * (B.T @ L @ A)
        H[tt, tt] += l * (B.T @ L @ B)
        b[ss] += l * (A.T @ L @ r)
        b[tt] += l * (B.T @ L @ r)
    return H, b


def gradient(nodes, edges, transforms, informations, uncertain=None, line_process_weight=None):
    """The gradient of F with respect to the right perturbations of the free nodes (node 0 is fixed): 2 sum l J^T L r, [N - 1, 6].
    (With l at its optimum the derivative through l vanishes.)"""
    _, b = normal_equations(nodes, edges, transforms, informations, uncertain, line_process_weight)
    return 2.0 * b[6:].reshape(-1, 6)


def optimize(nodes, edges, transforms, informations, uncertain=None, line_process_weight=None, max_iterations=100,
             gradient_tolerance=1e-9, cost_tolerance=1e-12):
    """One graph.  -> dict(nodes, weights, cost0, cost, iterations, stop)."""
    X = np.array(nodes, dtype=np.float64)
    args = (edges, transforms, informations, uncertain, line_process_weight)
    n = len(X)
    if n == 0 or len(edges) == 0:
        return dict(nodes=X, weights=np.ones(len(edges)), cost0=0.0, cost=0.0, iterations=0, stop=STOP_EMPTY)
    F = F0 = cost(X, *args)
    lam, iterations, stop = LAMBDA0, 0, STOP_MAX_ITERATIONS
    while iterations < max_iterations:
        H, b = normal_equations(X, *args)
        if np.max(np.abs(2.0 * b[6:])) <= gradient_tolerance:
            stop = STOP_GRADIENT
            break
        Hf, bf = H[6:, 6:], b[6:]
        D = np.zeros_like(Hf)
        idx = np.arange(n - 1)
        D.reshape(n - 1, 6, n - 1, 6)[idx, :, idx, :] = Hf.reshape(n - 1, 6, n - 1, 6)[idx, :, idx, :]  # the 6 x 6 diagonal blocks
        d = np.linalg.solve(Hf + lam * D, -bf)
        Xc = X.copy()
        for i in range(1, n):
            Xc[i] = retract(X[i], d[6 * (i - 1):6 * i])
        try:
            Fc = cost(Xc, *args)
        except ValueError:
            Fc = math.inf
        iterations += 1
        if Fc <= F:
            rel = (F - Fc) / F if F > 0.0 else 0.0
            X, F = Xc, Fc
            lam = max(lam * LAMBDA_DOWN, LAMBDA_MIN)
            if rel <= cost_tolerance:
                stop = STOP_COST
                break
        else:
            lam *= LAMBDA_UP
            if lam > LAMBDA_MAX:
                stop = STOP_COST
                break
    return dict(nodes=X, weights=weights(X, *args), cost0=F0, cost=F, iterations=iterations, stop=stop)


def rotation_angle(R):
    return math.atan2(0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]), 0.5 * (np.trace(R) - 1.0))


def pose_errors(nodes, truth):
    """-> (largest rotation angle, largest translation distance) between corresponding poses."""
    ang = max(rotation_angle(a[:3, :3].T @ b[:3, :3]) for a, b in zip(nodes, truth))
    tra = max(float(np.linalg.norm(a[:3, 3] - b[:3, 3])) for a, b in zip(nodes, truth))
    return ang, tra
