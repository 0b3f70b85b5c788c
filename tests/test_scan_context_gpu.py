"""GPU: ops.scan_context, ops.scan_context_distance, ops.detect_loops and `python -m rdmnet_amd.prepare loops` against the float64
restatement tests/scan_context_restatement.py.

Descriptor.  A bin is the maximum of fp32 values, so it is compared bit for bit wherever the restatement says that no point of the
bin lies within 1e-5 rad / 1e-5 max(r, 1) m of a bin edge or 1e-5 max_range of the range limit (lo == hi), and must lie in [lo, hi]
elsewhere (tests/test_scan_context.py bounds how many such bins the bundled scans have).

Distance.  The inputs are the restatement's descriptors, so binning plays no part.  Bound |d - d64| <= 1e-5 absolute: a cosine is a
sum of 20 products of normalised fp32 columns and d a mean of at most 60 of them, a worst case of a few tens of 2^-24; measured on
one MI355X: 1.4e-7 on the scans and their rotated copies, 9.8e-8 on the random 37 x 53 fixture, at most 1.2e-7 on the other shapes
(printed by the tests).  Shifts are compared where the restatement's
best two shifts differ by >= 1e-4, best candidates where its best two candidates do.

End to end.  The issue quotes the distance of the rotated copy as 0.0442; the restatement gives 0.04417233, which is what the kernel
is held to within 1e-5 (the quoted figure is that value rounded to four places, asserted as such)."""
import os

import numpy as np
import pytest

import scan_context_restatement as SC

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def special_cloud():
    """A NaN row, a point at the origin, one beyond max_range, one exactly at max_range (48^2 + 64^2 = 80^2 exactly) and two
    ordinary points, one of them with a negative value."""
    return np.array([[np.nan, 1.0, 1.0], [0.0, 0.0, 5.0], [90.0, 5.0, 3.0], [48.0, 64.0, 1.0], [10.0, 3.0, -2.5], [1.0, np.inf, 2.0],
                     [-20.0, -7.0, 0.25]], np.float32)


def bin_centre_cloud(n_rings=20, n_sectors=60, max_range=80.0, seed=3):
    """Three points per bin at the bin centre with a jitter of at most 0.4 bin each way; a bin's heights lie within 0.3 m of a level
    between -3 and 3 m (values -1.3 ... 5.3, many bins all negative); one bin in ten stays empty."""
    rng = np.random.default_rng(seed)
    ring, sec = np.meshgrid(np.arange(n_rings), np.arange(n_sectors), indexing='ij')
    keep = rng.random(ring.shape) >= 0.1
    ring, sec = np.repeat(ring[keep], 3), np.repeat(sec[keep], 3)
    r = (ring + 0.5 + rng.uniform(-0.4, 0.4, ring.size)) * (max_range / n_rings)
    th = (sec + 0.5 + rng.uniform(-0.4, 0.4, sec.size)) * (2 * np.pi / n_sectors)
    z = np.repeat(rng.uniform(-3.0, 3.0, r.size // 3), 3) + rng.uniform(-0.3, 0.3, r.size)
    pts = np.stack([r * np.cos(th), r * np.sin(th), z], 1).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def batch_clouds(scans):
    return [scans['s000000'], scans['s000004'], np.zeros((0, 3), np.float32), scans['s000007'],
            np.array([[3.0, -4.0, -2.75]], np.float32), special_cloud()]


def check_interval(got, cloud, **kw):
    D, lo, hi = SC.descriptor_interval(cloud, **kw)
    assert got.shape == D.shape and got.dtype == np.float32
    tight = lo == hi
    assert ((lo <= got) & (got <= hi)).all()
    assert np.array_equal(got[tight].view(np.uint32), lo[tight].view(np.uint32))  # bit for bit
    return int((~tight).sum()), int((got != D).sum())


def test_descriptor_batch_against_the_restatement(ops, scans):
    clouds = batch_clouds(scans)
    got = ops.scan_context([dev(c) for c in clouds]).cpu().numpy()
    assert got.shape == (len(clouds), 20, 60)
    for i, c in enumerate(clouds):
        loose, differ = check_interval(got[i], c)
        print(f'cloud {i}: {len(c)} points, {loose} bins with lo != hi, {differ} bins differ from the restatement')
    assert not got[2].any()  # the empty cloud
    assert got[4, 1, 51] == np.float32(-0.75) and np.count_nonzero(got[4]) == 1  # one point: r = 5, theta = 2 pi - 0.927
    sp = got[5]
    assert sp[19, 8] == np.float32(3.0)  # r == max_range is kept, in the last ring
    assert sp[2, 2] == np.float32(-0.5) and sp[5, 33] == np.float32(2.25) and np.count_nonzero(sp) == 3
    assert got[0].min() < -0.7  # negative heights survive the integer maximum


def test_descriptor_is_deterministic_and_batch_independent(ops, scans):
    import torch
    clouds = [dev(c) for c in batch_clouds(scans)]
    a, an, av = ops.scan_context(clouds, return_normalised=True)
    b, bn, bv = ops.scan_context(clouds, return_normalised=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(an.view(torch.int32), bn.view(torch.int32))
    assert torch.equal(av, bv)
    for i, c in enumerate(clouds):
        one = ops.scan_context([c])  # (the empty cloud too: one scan of 0 rows)
        assert torch.equal(one[0].view(torch.int32), a[i].view(torch.int32)), f'cloud {i} alone differs from the batch'
    # another order of the points, and the packed form with ld = 4 (xyz + intensity)
    perm = torch.randperm(clouds[0].shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(ops.scan_context([clouds[0][perm]])[0].view(torch.int32), a[0].view(torch.int32))
    counts = [c.shape[0] for c in clouds]
    xyzi = torch.cat([torch.cat([c, torch.full((c.shape[0], 1), 7.0, device='cuda')], 1) for c in clouds])
    offsets = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
    packed = ops.scan_context(xyzi, offsets)
    assert xyzi.stride(0) == 4 and torch.equal(packed.view(torch.int32), a.view(torch.int32))
    # normalised form and masks: unit columns where valid, zero elsewhere and in the pad columns
    h, hn, hv = a.cpu().numpy(), an.cpu().numpy(), av.cpu().numpy()
    for i in range(len(clouds)):
        Dn, valid = SC.normalise(h[i])
        assert hn.shape[1:] == (20, 64) and not hn[i][:, 60:].any()
        assert np.abs(hn[i][:, :60] - Dn).max() <= 2.0 ** -23
        assert int(hv[i]) == sum(1 << j for j in np.nonzero(valid)[0])


def test_descriptor_bin_centres_are_bit_equal(ops):
    for kw in (dict(), dict(n_rings=7, n_sectors=64, max_range=55.0), dict(n_rings=64, n_sectors=1)):
        pts = bin_centre_cloud(kw.get('n_rings', 20), kw.get('n_sectors', 60), kw.get('max_range', 80.0))
        D, lo, hi = SC.descriptor_interval(pts, **kw)
        assert np.array_equal(lo, hi) and (D < 0).sum() >= 5 and (D == 0).any()
        got = ops.scan_context([dev(pts)], **kw)[0].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), D.view(np.uint32)), kw


def test_descriptor_other_shapes_and_heights(ops, scans):
    s0 = scans['s000000']
    for kw in (dict(n_rings=7, n_sectors=64), dict(n_rings=20, n_sectors=1), dict(n_rings=1, n_sectors=1),
               dict(n_rings=64, n_sectors=64, max_range=30.0, lidar_height=-1.5)):
        got = ops.scan_context([dev(s0)], **kw)[0].cpu().numpy()
        loose, differ = check_interval(got, s0, **kw)
        print(kw, loose, 'bins with lo != hi,', differ, 'differ')


def special_descriptors(scans):
    if 'special' not in _cache:
        s0 = scans['s000000']
        Ds = [SC.descriptor(scans[k]) for k in ('s000000', 's000004', 's000007')]
        Ds += [SC.descriptor(SC.rotate_z(s0, a)) for a in (91.0, 33.0, 200.0, -47.0)]
        Ds.append(np.zeros((20, 60), np.float32))
        one = np.zeros((20, 60), np.float32)
        one[:, 17] = Ds[0][:, 5]
        assert one.any()
        Ds.append(one)
        D = np.stack(Ds)
        _cache['special'] = (D, D) + SC.distance_matrix(D, D)
    return _cache['special']


def random_descriptors():
    if 'random' not in _cache:
        Q, C = SC.random_fixture()
        _cache['random'] = (Q, C) + SC.distance_matrix(Q, C)
    return _cache['random']


def check_matrix(ops, Q, C, d64, s64, m64, label):
    full = ops.scan_context_distance(dev(Q), dev(C), exclude_recent=-1, full=True)
    d, s = full.distances.cpu().numpy(), full.shifts.cpu().numpy()
    err = float(np.abs(d.astype(np.float64) - d64).max())
    clear = m64 >= 1e-4
    print(f'{label}: max |d - d64| = {err:.3e} over {d.size} pairs; shifts compared on {int(clear.sum())} of them')
    assert err <= 1e-5
    assert np.array_equal(s[clear], s64[clear])
    return full, d, s


def check_best(res, d, s, d64, **window):
    """res against the argmin of the kernel's own matrix (exactly) and against the restatement's candidate where that is clear."""
    idx, best, _ = SC.search(d, **window)
    gi, gd, gs = res.index.cpu().numpy(), res.distance.cpu().numpy(), res.shift.cpu().numpy()
    assert np.array_equal(gi, idx)
    assert np.array_equal(gd.view(np.uint32), best.astype(np.float32).view(np.uint32))
    has = idx >= 0
    assert np.array_equal(gs[has], s[np.nonzero(has)[0], idx[has]]) and (gs[~has] == -1).all() and np.isposinf(gd[~has]).all()
    idx64, _, gap64 = SC.search(d64, **window)
    clear = gap64 >= 1e-4
    assert np.array_equal(gi[clear], idx64[clear])
    return int(has.sum()), int(clear.sum())


def test_distance_matrix_special_descriptors(ops, scans):
    Q, C, d64, s64, m64 = special_descriptors(scans)
    full, d, s = check_matrix(ops, Q, C, d64, s64, m64, 'scans, rotated copies, zero and one-column descriptors')
    assert [int(s[3 + k, 0]) for k in range(4)] == [15, 5, 33, 52]  # the rotated copies against s000000
    assert (d[7] == 1.0).all() and (d[:, 7] == 1.0).all() and (s[7] == 0).all()  # the empty descriptor: no valid column pair
    assert np.abs(np.diag(d)[:7]).max() <= 1e-6 and (np.diag(s)[:7] == 0).all()
    check_best(full, d, s, d64, exclude_recent=-1)
    for ex in (0, 3):
        res = ops.scan_context_distance(dev(Q), dev(C), exclude_recent=ex, full=True)
        assert np.array_equal(res.distances.cpu().numpy().view(np.uint32), d.view(np.uint32))  # eligibility only affects the best
        check_best(res, d, s, d64, exclude_recent=ex)


def test_distance_matrix_random_descriptors(ops):
    Q, C, d64, s64, m64 = random_descriptors()
    full, d, s = check_matrix(ops, Q, C, d64, s64, m64, 'random 37 x 53')
    print('eligible / clear queries:', check_best(full, d, s, d64, exclude_recent=-1))


@pytest.mark.parametrize('window', [dict(exclude_recent=0), dict(exclude_recent=3), dict(exclude_recent=1000), dict(exclude_recent=-1),
                                    dict(exclude_recent=3, q_base=5), dict(exclude_recent=50, q_base=100, c_base=40)])
def test_best_only_mode_and_windows(ops, window):
    import torch
    Q, C, d64, s64, m64 = random_descriptors()
    full = ops.scan_context_distance(dev(Q), dev(C), full=True, **window)
    d, s = full.distances.cpu().numpy(), full.shifts.cpu().numpy()
    eligible, clear = check_best(full, d, s, d64, **window)
    want = SC.eligible(37, 53, window.get('q_base', 0), window.get('c_base', 0), window['exclude_recent']).any(1).sum()
    assert eligible == want
    only = ops.scan_context_distance(dev(Q), dev(C), **window)
    assert only.distances is None and only.shifts is None
    for a, b in ((only.distance.view(torch.int32), full.distance.view(torch.int32)), (only.index, full.index), (only.shift, full.shift)):
        assert torch.equal(a, b)
    if window['exclude_recent'] == 1000:
        assert (only.index == -1).all() and (only.shift == -1).all() and torch.isposinf(only.distance).all()
    if window == dict(exclude_recent=3):
        assert only.index[:3].tolist() == [-1, -1, -1] and (only.index[3:] >= 0).all()


def test_base_indices_split_a_search(ops):
    import torch
    Q, C, d64, s64, m64 = random_descriptors()
    one = ops.scan_context_distance(dev(Q), dev(C), exclude_recent=3, q_base=2)
    a = ops.scan_context_distance(dev(Q[:20]), dev(C), exclude_recent=3, q_base=2)
    b = ops.scan_context_distance(dev(Q[20:]), dev(C), exclude_recent=3, q_base=22)
    for name in ('distance', 'index', 'shift'):
        assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)]).view(torch.int32), getattr(one, name).view(torch.int32)), name
    # candidates in two calls: the better of the two per query, the first call winning ties, is the one call's answer
    lo = ops.scan_context_distance(dev(Q), dev(C[:30]), exclude_recent=3, q_base=2)
    hi = ops.scan_context_distance(dev(Q), dev(C[30:]), exclude_recent=3, q_base=2, c_base=30)
    take_hi = hi.distance < lo.distance
    index = torch.where(take_hi, torch.where(hi.index >= 0, hi.index + 30, hi.index), lo.index)
    assert torch.equal(index, one.index)
    assert torch.equal(torch.where(take_hi, hi.distance, lo.distance).view(torch.int32), one.distance.view(torch.int32))
    assert torch.equal(torch.where(take_hi, hi.shift, lo.shift), one.shift)
    # the sequence against itself (one normalised copy inside the call) equals the two-sided call
    self_a = ops.scan_context_distance(dev(C), dev(C), exclude_recent=5, full=True)
    same = dev(C)
    self_b = ops.scan_context_distance(same, same, exclude_recent=5, full=True)
    assert torch.equal(self_a.distances.view(torch.int32), self_b.distances.view(torch.int32)) and torch.equal(self_a.index, self_b.index)


def test_other_descriptor_shapes(ops):
    for n_rings, n_sectors, n_q, n_c in ((7, 64, 17, 9), (20, 1, 5, 4), (1, 1, 3, 3), (64, 33, 3, 19)):
        Q, C = SC.random_descriptors(n_q, 5, n_rings, n_sectors), SC.random_descriptors(n_c, 6, n_rings, n_sectors)
        d64, s64, m64 = SC.distance_matrix(Q, C)
        full, d, s = check_matrix(ops, Q, C, d64, s64, m64, f'{n_rings} x {n_sectors}')
        check_best(full, d, s, d64, exclude_recent=-1)
    with pytest.raises(ValueError):
        ops.scan_context_distance(dev(np.zeros((2, 20, 65))), dev(np.zeros((2, 20, 65))))
    empty = ops.scan_context_distance(dev(np.zeros((3, 20, 60))), dev(np.zeros((0, 20, 60))), exclude_recent=-1)
    assert empty.index.tolist() == [-1, -1, -1]


def loop_sequence(scans):
    return [scans['s000000'], scans['s000004'], scans['s000007'], SC.rotate_z(scans['s000000'], 91.0)]


def test_detect_loops_end_to_end(ops, scans):
    seq = loop_sequence(scans)
    ref = SC.distance(SC.descriptor(seq[3]), SC.descriptor(seq[0]))
    assert ref[1] == 15 and abs(ref[0] - 0.0442) < 5e-5
    assert abs(SC.distance(SC.descriptor(seq[2]), SC.descriptor(seq[0]))[0] - 0.309) < 1e-3  # 2 -> 0: rejected
    desc = ops.scan_context([dev(c) for c in seq])
    query, cand, dist, shift, yaw = ops.detect_loops(desc, threshold=0.13, exclude_recent=2)
    print('loops:', query, cand, dist, shift, yaw, 'restatement:', ref)
    assert query.tolist() == [3] and cand.tolist() == [0] and shift.tolist() == [15] and yaw.tolist() == [90.0]
    assert abs(float(dist[0]) - ref[0]) <= 1e-5
    assert len(ops.detect_loops(desc, threshold=0.13, exclude_recent=50)[0]) == 0
    assert ops.detect_loops(desc, threshold=0.4, exclude_recent=2)[0].tolist() == [2, 3]


def test_prepare_loops_writes_the_pair_list(ops, scans, tmp_path):
    from rdmnet_amd import dataset, prepare
    seq = loop_sequence(scans)
    folder = tmp_path / 'downsampled_xyzi' / '00'
    os.makedirs(folder)
    for f, c in enumerate(seq):
        np.save(folder / ('%06d.npy' % f), np.concatenate([c, np.zeros((len(c), 1), np.float32)], 1))
    assert prepare.main(['loops', '--dataset-root', str(tmp_path), '--sequences', '0', '--exclude-recent', '2', '--batch', '3']) == 0
    text = (tmp_path / 'loops' / '00').read_text()
    assert text == prepare.format_pair_line(3, 0, prepare.yaw_transform(15))
    score = (tmp_path / 'loops' / '00.scores').read_text().split('\n')
    assert len(score) == 2 and score[1] == ''
    q, c, d, s, yaw = score[0].split()
    ref = SC.distance(SC.descriptor(seq[3]), SC.descriptor(seq[0]))[0]
    assert (q, c, s, yaw) == ('3', '0', '15', '90.0') and abs(float(d) - ref) <= 1e-5 + 5e-7  # (six decimals in the file)
    meta = dataset.load_kitti_gt_txt(str(tmp_path / 'loops'), 0)
    assert len(meta) == 1 and (meta[0]['frame1'], meta[0]['frame0']) == (3, 0)
