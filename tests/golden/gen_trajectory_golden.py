"""Writes tests/golden/trajectory.npz: the reference's own umeyama_alignment and eval_absolute_error
(experiments/eval_pose_visualization_online.py:120-212) and its chaining rule (:279,386-388) on seeded synthetic trajectories.

    python tests/golden/gen_trajectory_golden.py

Runs only where the reference tree is present; the module is imported through ref_import's shims, with stubs for the
third-party modules it imports at the top and never uses in these two functions.  Only inputs and results are stored:
per case k: pair_k [n, 4, 4] (estimated pair transforms), gt_pair_k (ground-truth pair transforms), traj_k / gt_traj_k (chained),
umeyama_k [13] (r row-major, t, c), errors_k [4] (r_rmse, r_mean, rmse, mean -- the reference's dict in its order)."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_import  # noqa: E402
import pose_graph_restatement as R  # noqa: E402

# (poses, seed, noise scale); seed None: the trajectory equals its ground truth.  Case 4 is a longer drive with gentler turns (an
# extent of a few hundred metres) whose estimate drifts by several metres, the sizes a KITTI sequence shows.
CASES = [(3, 0, 1.0), (10, 1, 1.0), (57, 2, 1.0), (200, 3, 1.0), (200, 4, 3.0), (25, None, 1.0)]


def stub(name, **attrs):
    if name in sys.modules:
        return
    try:
        __import__(name)
    except Exception:
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m


def reference_module():
    ref_import.install()
    stub('tqdm', tqdm=lambda x, **k: x)
    # the module asks geotransformer.utils.open3d for names that the reference tree does not define (make_mesh_corr_lines, ...):
    # a module that answers every name, none of which the two functions use
    anything = types.ModuleType('geotransformer.utils.open3d')
    anything.__getattr__ = lambda name: None
    import geotransformer.utils  # noqa: F401
    sys.modules['geotransformer.utils.open3d'] = anything
    stub('tensorboard')
    stub('torch.utils.tensorboard', SummaryWriter=None)
    stub('matplotlib')
    stub('matplotlib.pyplot')
    stub('utils')
    stub('utils.utils_common', to_o3d_pcd=None)
    import eval_pose_visualization_online as m
    return m


def pairs(n, seed, scale):
    """Ground-truth pair transforms of a drive and estimates with a drift of a few metres and a few degrees over the run."""
    rng = np.random.default_rng(100 if seed is None else seed)
    gt, est = [], []
    for _ in range(n):
        turn = [0.0, 0.02, 0.08] if scale == 1.0 else [0.0, 0.002, 0.012]
        d = np.concatenate([turn + rng.normal(scale=0.03, size=3), [-2.0, 0.0, 0.0] + rng.normal(scale=0.2, size=3)])
        T = R.retract(np.eye(4), d)
        gt.append(T)
        noise = scale * np.concatenate([rng.normal(scale=0.004, size=3), rng.normal(scale=0.08, size=3)])
        est.append(T if seed is None else R.retract(T, noise))
    return np.asarray(est), np.asarray(gt)


def chain(transforms):  # the reference's loop (:279,386-388), run on its own arithmetic
    cur = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    out = []
    for T in transforms:
        cur = np.matmul(cur, np.linalg.inv(T))
        out.append(cur)
    return np.asarray(out)


def decided(value, decimals):
    """No unrounded value within 1e-6 of a rounding boundary."""
    scaled = abs(value) * 10 ** decimals
    assert abs(scaled - np.floor(scaled) - 0.5) > 1e-6 * 10 ** decimals, (value, decimals)


def main():
    m = reference_module()
    out = {'n_cases': np.int64(len(CASES))}
    for k, (n, seed, scale) in enumerate(CASES):
        est, gt = pairs(n, seed, scale)
        traj, gt_traj = chain(est), chain(gt)
        r, t, c = m.umeyama_alignment(traj[:, :3, 3].transpose((1, 0)), gt_traj[:, :3, 3].transpose((1, 0)))
        errors = m.eval_absolute_error(traj, gt_traj, np.linalg.inv(gt_traj))
        # the unrounded values, from the aligned trajectory, only to assert that the rounding is decided
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = r, t
        E = np.linalg.inv(gt_traj) @ (T @ traj)
        te = np.abs(E[:, :3, 3])
        deg = np.degrees(np.arccos(np.clip((np.trace(E[:, :3, :3], axis1=1, axis2=2) - 1) / 2, -1, 1)))
        rmse = np.sqrt(np.sum(te ** 2) / len(te))
        unrounded = np.array([np.mean(te), rmse, np.mean(deg), np.sqrt(np.sum(deg ** 2) / len(deg))])
        decided(unrounded[0], 3), decided(rmse, 3), decided(rmse, 2), decided(unrounded[2], 2), decided(unrounded[3], 2)
        out.update({f'pair_{k}': est, f'gt_pair_{k}': gt, f'traj_{k}': traj, f'gt_traj_{k}': gt_traj,
                    f'umeyama_{k}': np.concatenate([r.reshape(-1), t, [c]]),
                    f'errors_{k}': np.array([errors[key] for key in ('r_rmse', 'r_mean', 'rmse', 'mean')], np.float64),
                    f'unrounded_{k}': unrounded})
        print(k, n, errors, unrounded)
    np.savez_compressed(os.path.join(HERE, 'trajectory.npz'), **out)


if __name__ == '__main__':
    main()
