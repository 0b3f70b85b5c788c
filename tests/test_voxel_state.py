"""CPU: the voxel map state (include/rdmnet_hip.h, "voxel map state") -- the header and the bindings, the merge law
on the NumPy restatement tests/voxel_state_restatement.py, the file format (ops.write_state / ops.read_state and every refusal of the
reader) and the command line's --map-save, --map-prior and --map-localize.  Everything is integers: np.array_equal throughout."""
import os
import re

import numpy as np
import pytest

import voxel_state_restatement as SR
from rdmnet_amd import _lib, trajectory
from test_voxel_map import write_pairs
from test_voxel_observations_gpu import fixture as six_scans

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'rdmnet_hip.h')
NEW = ('rdm_voxel_map_export', 'rdm_voxel_map_import')


def test_header_declares_the_entry_points_and_bindings_have_them():
    text = open(HEADER).read()
    for name in NEW:
        decl = re.search(r'^int ' + name + r'\(([^;]*)\);', text, re.M).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(',') if a.strip()]), name
    assert 'tests/voxel_state_restatement.py' in text and '§7 voxel map state' in text
    assert _lib.ABI_VERSION == 2 and re.search(r'#define RDM_ABI_VERSION 2\b', text)  # new entry points do not bump it
    assert re.search(r'#define RDM_VOXEL_MOMENTS_SHIFT %d\b' % _lib.VOXEL_MOMENTS_SHIFT, text)
    # both open with the map's head and the two optional blocks, as rdm_voxel_map_query does
    query = _lib.SIGNATURES['rdm_voxel_map_query'][1]
    for name in NEW:
        assert _lib.SIGNATURES[name][1][:8] == query[:8], name


# ---- the merge law ---------------------------------------------------------------------------------------------------------------

def build(clouds, poses, lo, hi, voxel=0.3, **kind):
    return SR.build(clouds[lo:hi], poses[lo:hi], voxel, 4, **kind)


@pytest.mark.parametrize('kind', [dict(), dict(moments=True), dict(observations=True), dict(moments=True, observations=True)],
                         ids=['plain', 'moments', 'observations', 'both'])
def test_the_restatements_merge_law(scans, kind):
    clouds, poses, _ = six_scans(scans)
    one = build(clouds, poses, 0, 6, **kind)
    assert len(one.keys) > 100 and one.counts.max() > 1 and one.integrated == sum(len(c) for c in clouds)
    for k in (1, 3, 5):
        merged = SR.merge(build(clouds, poses, 0, k, **kind), build(clouds, poses, k, 6, **kind))
        assert SR.same(merged, one) == [], (k, SR.same(merged, one))
    a, b, c = build(clouds, poses, 0, 2, **kind), build(clouds, poses, 2, 3, **kind), build(clouds, poses, 3, 6, **kind)
    left, right = SR.merge(SR.merge(a, b), c), SR.merge(a, SR.merge(b, c))
    assert SR.same(left, one) == [] and SR.same(right, one) == []
    if kind.get('observations'):
        assert one.num_scans == 6 and {1, 2, 3} <= set(one.seen[:, 0].tolist())
        # the other order needs the ids said: b's scans are 3 ... 5, a's stay 0 ... 2
        late, early = build(clouds, poses, 3, 6, **kind), build(clouds, poses, 0, 3, **kind)
        shifted = SR.State(0.3, 4, **kind)
        shifted = SR.merge(SR.merge(shifted, late, 3), early, 0)
        assert SR.same(shifted, one) == []


def test_the_record_rule_and_records_of_one_key():
    top = 2 ** 31 - 2
    keys = np.array([5, 1 << 63, (1 << 64) - 1, 5, 5, 5, 5, 5, 5, 7], np.uint64)
    counts = np.array([2, 1, 1, 0, 1, 1, 1, 1, 1, 1], np.uint32)
    seen = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [3, 4, 5], [1, -1, 0], [1, 3, 2], [1, top, top], [2, 0, top - 3]],
                    np.int32)
    assert SR.valid(keys, counts).tolist() == [True, False, False, False] + [True] * 6
    assert SR.valid(keys, counts, seen).tolist() == [True, False, False, False, False, False, False, False, True, True]
    assert SR.valid(keys, counts, seen, id_offset=3).tolist() == [True] + [False] * 8 + [True]
    assert SR.valid(keys, counts, seen, id_offset=4).tolist() == [True] + [False] * 9
    st = SR.State(1.0, 3, moments=True, observations=True)
    sums = np.arange(30, dtype=np.int64).reshape(10, 3) - 7
    moms = np.arange(90, dtype=np.int64).reshape(10, 9)
    assert SR.add_records(st, keys, counts, sums, moms, seen) == 7
    assert st.keys.tolist() == [5, 7] and st.counts.tolist() == [3, 1] and st.integrated == 4
    assert st.sums.tolist() == [(sums[0] + sums[8]).tolist(), sums[9].tolist()]
    assert st.moments.tolist() == [(moms[0] + moms[8]).tolist(), moms[9].tolist()]
    assert st.seen.tolist() == [[2, 0, top], [2, 0, top - 3]]
    wrap = SR.State(1.0, 3)
    SR.add_records(wrap, [9, 9], [0xffffffff, 2], np.zeros((2, 3), np.int64))
    assert wrap.counts.tolist() == [1] and wrap.integrated == 0x100000001  # a count wraps at 2^32, the counter does not


# ---- the file ----------------------------------------------------------------------------------------------------------------

def a_state(scans, **kind):
    clouds, poses, _ = six_scans(scans)
    st = SR.build(clouds, poses, 1.0, 4, **kind)
    rows = SR.export(st)
    return dict(keys=rows['keys'], counts=rows['counts'], sums=rows['sums'], moments=rows['moments'], observations=rows['observations'],
                voxel=1.0, channels=4, num_scans=st.num_scans, counters=st.stats())


def test_write_state_and_read_state_round_trip(scans, tmp_path):
    import torch
    from rdmnet_amd import ops
    for kind in (dict(), dict(moments=True), dict(moments=True, observations=True)):
        st = a_state(scans, **kind)
        path = str(tmp_path / 'a_state.npz')
        ops.write_state(path, st)
        assert os.listdir(tmp_path) == ['a_state.npz']
        back = ops.read_state(path)
        names = ['keys', 'counts', 'sums'] + [k for k in ('moments', 'observations') if st[k] is not None]
        assert sorted(k for k in back if isinstance(back[k], np.ndarray)) == sorted(names)
        for k in names:
            assert back[k].dtype == st[k].dtype and np.array_equal(back[k], st[k]), k
        assert back['voxel'] == 1.0 and back['channels'] == 4 and back['num_scans'] == st['num_scans']
        assert back['counters'] == st['counters'] and list(back['counters']) == list(_lib.VOXEL_MAP_STATS)
        # tensors are written as the arrays they hold
        ops.write_state(path, {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in st.items()})
        again = ops.read_state(path)
        assert all(np.array_equal(again[k], st[k]) for k in names)
        with np.load(path, allow_pickle=False) as z:
            assert str(z['format']) == 'rdmnet_amd.voxel_map' and int(z['version']) == 1 and int(z['frac_bits']) == 20
            assert int(z['moments_shift']) == 8 and z['voxel'].dtype == np.float64 and z['counters'].dtype == np.uint64


def test_read_state_refuses_by_name(scans, tmp_path):
    from rdmnet_amd import ops
    st = a_state(scans, moments=True, observations=True)
    path = str(tmp_path / 'good.npz')
    ops.write_state(path, st)
    with np.load(path, allow_pickle=False) as z:
        good = {k: z[k] for k in z.files}

    def refused(message, **change):
        data = dict(good)
        for k, v in change.items():
            if v is None:
                del data[k]
            else:
                data[k] = v
        bad = str(tmp_path / 'bad.npz')
        with open(bad, 'wb') as f:
            np.savez(f, **data)
        with pytest.raises(ValueError, match=message):
            ops.read_state(bad)

    def changed(name, row, col, value):
        a = good[name].copy()
        if a.ndim == 1:
            a[row] = value
        else:
            a[row, col] = value
        return a

    refused("not a voxel map state: format 'other'", format=np.array('other'))
    refused("not a voxel map state: no 'format'", format=None)
    refused('version 2, this library reads version 1', version=np.int64(2))
    refused('frac_bits 16, the library has 20', frac_bits=np.int64(16))
    refused('moments_shift 4, the library has 8', moments_shift=np.int64(4))
    refused(r'keys must be uint64 \[\d+\], got int64', keys=good['keys'].astype(np.int64))
    refused(r'counts must be uint32 \[\d+\], got int32', counts=good['counts'].astype(np.int32))
    refused(r'counts must be uint32 \[\d+\], got uint32 \[\d+\]', counts=good['counts'][:-1])
    refused(r'sums must be int64 \[\d+, 4\], got int64 \[\d+, 3\]', sums=good['sums'][:, :3])
    refused(r'moments must be int64 \[\d+, 9\], got float64', moments=good['moments'].astype(np.float64))
    refused(r'observations must be int32 \[\d+, 3\], got int32 \[\d+, 2\]', observations=good['observations'][:, :2])
    refused(r'counters must be uint64 \[6\]', counters=good['counters'][:5])
    refused('keys must ascend strictly with bit 63 clear', keys=changed('keys', 3, None, good['keys'][2]))
    refused('keys must ascend strictly with bit 63 clear', keys=good['keys'][::-1].copy())
    refused('keys must ascend strictly with bit 63 clear', keys=changed('keys', -1, None, np.uint64(1 << 63)))
    refused('counts must be >= 1', counts=changed('counts', 0, None, 0))
    refused('moments must be >= 0', moments=changed('moments', 2, 4, -1))
    for row in ([0, 0, 0], [3, 1, 2], [1, -1, 0], [1, 2, 1], [1, 2 ** 31 - 1, 2 ** 31 - 1]):
        obs = good['observations'].copy()
        obs[1] = row
        refused('observations must hold 1 <= scans <= last - first', observations=obs)
    obs = good['observations'].copy()
    obs[1] = [1, 2 ** 31 - 2, 2 ** 31 - 2]  # the last id there is
    data = dict(good, observations=obs)
    with open(path, 'wb') as f:
        np.savez(f, **data)
    assert np.array_equal(ops.read_state(path)['observations'], obs)
    pickled = str(tmp_path / 'pickled.npz')
    with open(pickled, 'wb') as f:
        np.savez(f, **dict(good, keys=np.array([{}], dtype=object)))
    with pytest.raises(ValueError):  # (allow_pickle=False)
        ops.read_state(pickled)


# ---- the command line ------------------------------------------------------------------------------------------------------------

def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_state_options_parse_and_need_their_flags(scans, tmp_path):
    from rdmnet_amd import ops
    a = parse(['--features-root', 'x'])
    assert a.map_save is False and a.map_prior is None and a.map_localize is False
    a = parse(['--features-root', 'x', '--map-save', '--map-prior', 'p.npz', '--map-localize'])
    assert a.map_save is True and a.map_prior == 'p.npz' and a.map_localize is True
    pairs, root = tmp_path / 'pairs', tmp_path / 'data'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10])
    folder = root / 'downsampled_xyzi' / '07'
    os.makedirs(folder)
    for f in (0, 10):
        np.save(folder / ('%06d.npy' % f), np.zeros((4, 4), np.float32))
    prior = {}
    for name, kind in (('full', dict(moments=True, observations=True)), ('bare', dict())):
        prior[name] = str(tmp_path / (name + '.npz'))
        ops.write_state(prior[name], a_state(scans, **kind))
    lines = []
    base = ['--features-root', str(pairs)]
    full = base + ['--map-scans', str(root), '--out', str(tmp_path / 'o')]

    def refused(argv, message):
        with pytest.raises(trajectory.TrajectoryError, match=message):
            trajectory.run(parse(argv), emit=lines.append)

    refused(base + ['--map-save'], '--map-save needs --map-scans and --out')
    refused(base + ['--map-save', '--out', str(tmp_path / 'o')], '--map-save needs --map-scans and --out')
    for argv in (base + ['--map-localize'], full + ['--map-localize'], base + ['--map-localize', '--map-prior', prior['full']],
                 base + ['--map-localize', '--map-prior', prior['full'], '--map-scans', str(root)]):
        refused(argv, '--map-localize needs --map-prior, --map-scans and --out')
    refused(full + ['--map-prior', prior['full']], '--map-prior needs --map-clean or --map-localize')
    missing = str(tmp_path / 'none.npz')
    refused(full + ['--map-localize', '--map-prior', missing], '--map-prior ' + re.escape(missing) + ': no such file')
    junk = str(tmp_path / 'junk.npz')
    open(junk, 'wb').write(b'not an archive')
    refused(full + ['--map-localize', '--map-prior', junk], '--map-prior ' + re.escape(junk) + ': cannot be read as a voxel map state')
    old = str(tmp_path / 'old.npz')
    with np.load(prior['full'], allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    with open(old, 'wb') as f:
        np.savez(f, **dict(data, version=np.int64(0)))
    refused(full + ['--map-localize', '--map-prior', old], 'cannot be read as a voxel map state .*version 0')
    refused(full + ['--map-localize', '--map-prior', prior['bare']], '--map-localize needs a prior with moments')
    refused(full + ['--map-clean', '--map-min-scans', '2', '--map-prior', prior['bare']],
            '--map-min-scans 2 with --map-clean counts the scans of the prior; --map-prior .* has no observations')
    refused(full + ['--map-clean', '--map-prior', prior['full']], '--map-clean needs a criterion')
    refused(full + ['--map-localize', '--map-prior', prior['full'], '--map-refine-sigma', '0'], '--map-refine-sigma must be > 0')
    refused(full + ['--map-localize', '--map-prior', prior['full'], '--map-refine-min-scans', '2'], '--map-refine-min-scans needs --map-refine')
    refused(full + ['--map-refine-neighbors', '7'], '--map-refine-neighbors needs --map-refine')
    assert lines == []  # found before anything is reported
    assert not os.path.exists(tmp_path / 'o')
    with pytest.raises(SystemExit, match='--map-save needs --map-scans and --out'):
        trajectory.main(base + ['--map-save'])


def test_the_two_line_formats():
    tallies = np.array([[1, 2, 3, 10, 20, 30, 100, 150], [0, 0, 1, 0, 5, 0, 50, 55]])
    prior = dict(name='5_chained_map_state.npz', voxels=1234, voxel=1.0, scans=8, moments=True)
    own = trajectory.clean_line(3, 'chained', tallies, 2, 25.0)
    assert trajectory.clean_line(3, 'chained', tallies, 2, 25.0, None) == own  # without a prior the line is what it was
    assert trajectory.clean_line(3, 'chained', tallies, 2, 25.0, prior) == (
        own + ', judged by the prior map 5_chained_map_state.npz (1234 voxels at 1 m, 8 scans)')
    assert trajectory.clean_line(3, 'chained', tallies, 1, 25.0, dict(prior, moments=False, voxel=0.3)).endswith(
        ', judged by the prior map 5_chained_map_state.npz (1234 voxels at 0.3 m, 8 scans, no moments: Sigma = sigma^2 I)')
    stats = dict(frames=4, iterations=np.array([3, 4, 5, 2]), correspondences=np.array([1000, 1100, 900, 0]), status=np.array([1, 1, 0, 2]),
                 degenerate=1)
    assert trajectory.localize_line(3, stats, prior) == (
        'seq 3 localized against the prior map 5_chained_map_state.npz (1234 voxels at 1 m, 8 scans): 4 frames, 3.50 iterations and 750 '
        'correspondences per frame, 1 degenerate frames')
