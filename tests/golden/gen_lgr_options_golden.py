"""Generates tests/golden/lgr_options.npz: the REFERENCE's LocalGlobalRegistration (geotransformer/modules/geotransformer/
local_global_registration.py, imported with the shims of ref_import.py, CPU) run with option sets other than the shipped one
on the LGR inputs four goldens already hold -- matching scores (expanded with tests/sampling.expand_scores), patch points and
masks, superpoint-pair scores.  Build container only; the fixture travels, the reference not.

Per (case, option set), under '<case>/<set>/':
  options           [topk, mutual, use_dustbin, confidence_threshold, use_global_score, correspondence_limit or -1]
  indices           (C, 3) int16: (patch, i, j) of the reference's correspondence matrix in nonzero order
  corr_scores       (C,) the reference's
  transform         the reference's estimated_transform
  inlier_counts, best, alt_hypotheses, alt_transforms
                    from tests/lgr_options_restatement.py (the reference restated with the lowest-index tie rule; un-forced, and
                    forced to every hypothesis within one inlier of the best, as gen_golden.py does with oracle.forward.lgr)
  undecided         (U, 3) int16: entries whose membership a relative perturbation of 3e-7 of S = exp(log scores) can flip
                    (lgr_options_restatement.decisions: k-th vs (k+1)-th of row and column, entry vs dustbin / threshold)
  limit_gap         relative gap between the L-th and (L+1)-th score (inf without a biting limit)
  exact             no undecided entry: the correspondence set must equal `indices` exactly; else the tie-aware comparison
Checked here: the restatement agrees with the reference on every decided entry (on all of them in exact cases), scores equal
bit for bit, the limit never sits on a tie, and a tie-aware entry has at most 1 % of C undecided (half the tests' cap).
synth0 is the tie-aware full-size case (its set 4 without the limit refines 5 471 correspondences, above the 4 608 the
refinement stages in LDS); its set 2 (mutual, k = 1) is left out: too many exact column ties to judge anything.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import ref_import  # noqa: E402

CASES = ('small', 'crop9', 'synth3', 'synth0')
SETS = {  # (topk, mutual, use_dustbin, confidence_threshold, use_global_score, correspondence_limit)
    'set1': (3, False, True, 0.0, False, None),
    'set2': (1, True, True, 0.0, False, None),
    'set3': (2, True, False, 0.05, False, None),
    'set4': (3, False, False, 0.05, True, 300),
    'set5': (2, False, True, 0.0, True, 200),
}
EXTRA = {'synth0': {'set4_nolimit': (3, False, False, 0.05, True, None)}}  # every correspondence refined: 5 471 > 4 608
LEFT_OUT = {('synth0', 'set2')}
TIE_AWARE_CASES = ('synth0',)


def main():
    ref_import.install()
    from geotransformer.modules.geotransformer.local_global_registration import LocalGlobalRegistration
    from rdmnet_amd import config as my_config
    from sampling import expand_scores
    import lgr_options_restatement as R

    torch.set_num_threads(8)
    fm = my_config.make_cfg().fine_matching
    fx = {}
    for case in CASES:
        g = np.load(os.path.join(HERE, f'forward_{case}.npz'))
        rm, sm = g['out/ref_node_corr_knn_masks'], g['out/src_node_corr_knn_masks']
        ms = torch.from_numpy(expand_scores(g['out/matching_scores'], rm, sm))
        rp, sp = torch.from_numpy(g['out/ref_node_corr_knn_points']), torch.from_numpy(g['out/src_node_corr_knn_points'])
        gs = torch.from_numpy(g['tap/node_corr_scores'])
        rmt, smt = torch.from_numpy(rm).bool(), torch.from_numpy(sm).bool()
        for name, tup in {**SETS, **EXTRA.get(case, {})}.items():
            if (case, name) in LEFT_OUT:
                continue
            opt = R.options(*tup)
            module = LocalGlobalRegistration(opt['topk'], fm.acceptance_radius, mutual=opt['mutual'],
                                             confidence_threshold=opt['confidence_threshold'], use_dustbin=opt['use_dustbin'],
                                             use_global_score=opt['use_global_score'],
                                             correspondence_threshold=fm.correspondence_threshold,
                                             correspondence_limit=opt['correspondence_limit'],
                                             num_refinement_steps=fm.num_refinement_steps)
            x = ms if opt['use_dustbin'] else ms[:, :-1, :-1]  # model_infer.py:319-320
            with torch.no_grad():
                ref_corr = module.compute_correspondence_matrix(torch.exp(x), rmt, smt)
                rc, sc, cs, T = module(rp, sp, rmt, smt, x, gs)
            idx = torch.nonzero(ref_corr)
            assert idx.shape[0] == cs.shape[0] and torch.equal(rc, rp[idx[:, 0], idx[:, 1]]) and torch.equal(sc, sp[idx[:, 0], idx[:, 2]])
            C = idx.shape[0]

            run, alts = R.alternatives(rp, sp, rmt, smt, ms, gs, fm, opt)
            corr, und = R.decisions(ms, rmt, smt, opt)
            n_und = int(und.sum())
            exact = n_und == 0 and case not in TIE_AWARE_CASES
            differ = (corr != ref_corr)
            assert not bool((differ & ~und).any()), (case, name, 'the restatement differs from the reference on a decided entry')
            if exact:
                assert torch.equal(run['indices'], idx) and torch.equal(run['corr_scores'], cs), (case, name)
            else:
                assert n_und <= 0.01 * C, (case, name, n_und, C, 'choose another full-size golden for this set')
                both = (corr & ref_corr)
                assert torch.equal(run['corr_scores'][both[corr]], cs[both[ref_corr]]), (case, name)
            gap = R.limit_gap(cs.numpy(), opt['correspondence_limit'])
            assert gap > 10 * R.UNDECIDED, (case, name, gap)
            p = f'{case}/{name}/'
            fx[p + 'options'] = np.asarray([tup[0], tup[1], tup[2], tup[3], tup[4], -1 if tup[5] is None else tup[5]], np.float64)
            fx[p + 'indices'] = idx.numpy().astype(np.int16)
            fx[p + 'corr_scores'] = cs.numpy()
            fx[p + 'transform'] = T.numpy()
            fx[p + 'undecided'] = torch.nonzero(und).numpy().astype(np.int16)
            fx[p + 'limit_gap'] = np.float64(gap)
            fx[p + 'exact'] = np.bool_(exact)
            if 'inlier_counts' in run:
                fx[p + 'inlier_counts'] = run['inlier_counts'].numpy().astype(np.int64)
                fx[p + 'best'] = np.int64(run['best'])
            fx[p + 'alt_hypotheses'] = np.asarray([i for i, _ in alts], np.int64)
            fx[p + 'alt_transforms'] = np.stack([A for _, A in alts]).astype(np.float32)
            from oracle import forward as ofw
            rre, rte = ofw.rre_rte(run['transform'].numpy(), T.numpy())
            print(f'{case:7s} {name:13s} C {C:5d} undecided {n_und:3d} ({100.0 * n_und / max(C, 1):.2f} %) exact {exact!s:5s} '
                  f'restatement vs reference: {int(differ.sum())} entries, limit gap {gap:.1e}, hypotheses {len(run["chunks"])}, '
                  f'near-tied {len(alts)}, pose rre {rre:.1e} deg rte {rte:.1e} m')
    path = os.path.join(HERE, 'lgr_options.npz')
    np.savez_compressed(path, **fx)
    print(f'{path}: {len(fx)} arrays, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
