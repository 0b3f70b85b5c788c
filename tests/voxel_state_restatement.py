"""NumPy restatement of the voxel map state (include/rdmnet_hip.h, "voxel map state"), written from the definition
on top of voxel_map_restatement.Map, voxel_moments_restatement.Moments and voxel_observations_restatement.Observed and sharing no code
with the library.

The state of a voxel is what the integrates added to it, as integers: key, count, the C sums and, where kept, the nine moment sums and
{scans, first, last}.  `export` gives the rows with count >= min_points in ascending key order.  A RECORD is such a row; it is valid
unless its key has bit 63 set, its count is 0 or, where it carries observations, it is not 1 <= scans <= last - first + 1 with
0 <= first <= last <= 2^31 - 2 - id_offset.  `add_records` adds the valid records of a batch into a state, key by key: count (mod
2^32), the sums, the moment sums, scans, min of first + id_offset, max of last + id_offset; `integrated` grows by the counts and
`occupied` by the new keys.  `merge(a, b, id_offset)` is a plus the export of b plus b's four skip counters: the state of the map of
the scans of both, when they are other scans.  A `State` never fills up."""
import numpy as np

import voxel_map_restatement as VM
import voxel_moments_restatement as MO
import voxel_observations_restatement as OB

SKIPS = ('skipped_nonfinite', 'skipped_range', 'out_of_extent', 'dropped_full')
MAX_ID = 2 ** 31 - 1  # ids lie below this


class State:
    def __init__(self, voxel, channels=4, moments=False, observations=False):
        self.voxel, self.channels = float(voxel), int(channels)
        self.keys = np.zeros(0, np.uint64)
        self.counts = np.zeros(0, np.uint32)
        self.sums = np.zeros((0, self.channels), np.int64)
        self.moments = np.zeros((0, 9), np.int64) if moments else None
        self.seen = np.zeros((0, 3), np.int32) if observations else None  # {scans, first, last}
        self.integrated = 0
        self.skipped = dict.fromkeys(SKIPS, 0)
        self.num_scans = 0

    def copy(self):
        out = State(self.voxel, self.channels, self.moments is not None, self.seen is not None)
        out.keys, out.counts, out.sums = self.keys.copy(), self.counts.copy(), self.sums.copy()
        out.moments = None if self.moments is None else self.moments.copy()
        out.seen = None if self.seen is None else self.seen.copy()
        out.integrated, out.skipped, out.num_scans = self.integrated, dict(self.skipped), self.num_scans
        return out

    def stats(self):
        return dict(occupied=len(self.keys), integrated=self.integrated, **self.skipped)


def build(clouds, poses, voxel, channels=4, moments=False, observations=False, min_range=0.0, max_range=np.inf):
    """The state of the map of `clouds` under `poses`, through the three restatements it stands on; the scans get the ids 0, 1, ..."""
    out = State(voxel, channels, moments, observations)
    m = VM.build(clouds, poses, voxel, channels, min_range, max_range)
    out.keys, out.counts, out.sums = m.keys.copy(), m.counts.astype(np.uint32), m.sums.copy()
    out.integrated = int(m.counts.sum())
    out.skipped.update(m.skipped)
    if moments:
        mo = MO.build(clouds, poses, voxel, channels, min_range, max_range)
        assert np.array_equal(mo.keys, m.keys)
        out.moments = mo.sums.copy()
    if observations:
        ob = OB.build(clouds, poses, voxel, channels, min_range, max_range)
        assert np.array_equal(ob.map.keys, m.keys)
        out.seen = np.stack([ob.scans, ob.first, ob.last], 1).astype(np.int32)
        out.num_scans = ob.num_scans
    return out


def export(state, min_points=1):
    """-> dict(keys uint64 [M], counts uint32 [M], sums int64 [M, C], moments int64 [M, 9] or None, observations int32 [M, 3] or None):
    the rows with count >= min_points, ascending keys -- the rows of Map.extract(min_points)."""
    take = state.counts >= max(int(min_points), 1)
    return dict(keys=state.keys[take], counts=state.counts[take], sums=state.sums[take],
                moments=None if state.moments is None else state.moments[take],
                observations=None if state.seen is None else state.seen[take])


def valid(keys, counts, seen=None, id_offset=0):
    """The record validity rule -> bool [n]."""
    keys, counts = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32)
    ok = ((keys >> np.uint64(63)) == 0) & (counts != 0)
    if seen is not None:
        scans, first, last = (np.asarray(seen)[:, k].astype(np.int64) for k in range(3))
        ok &= (1 <= scans) & (scans <= last - first + 1) & (0 <= first) & (first <= last) & (last <= MAX_ID - 1 - int(id_offset))
    return ok


def add_records(state, keys, counts, sums, moments=None, seen=None, id_offset=0):
    """Adds a batch of records into `state` in place -> the number of rejected records.  moments / seen are read where the state keeps
    the block (and must then be given)."""
    keys, counts, sums = np.asarray(keys, np.uint64), np.asarray(counts, np.uint32), np.asarray(sums, np.int64).reshape(-1, state.channels)
    assert (state.moments is None or moments is not None) and (state.seen is None or seen is not None)
    seen = None if state.seen is None else np.asarray(seen, np.int32).reshape(-1, 3)
    ok = valid(keys, counts, seen, id_offset)
    k = np.concatenate([state.keys, keys[ok]])
    new, inverse = np.unique(k, return_inverse=True)
    inverse = inverse.reshape(-1)

    def total(old, add, width):
        out = np.zeros((len(new),) + width, np.int64)
        np.add.at(out, inverse, np.concatenate([old.astype(np.int64), add.astype(np.int64)]))
        return out

    n = total(state.counts, counts[ok], ())
    state.integrated += int(counts[ok].astype(np.int64).sum())
    state.counts = (n & 0xffffffff).astype(np.uint32)  # (a count wraps at 2^32)
    state.sums = total(state.sums, sums[ok], (state.channels,))
    if state.moments is not None:
        state.moments = total(state.moments, np.asarray(moments, np.int64).reshape(-1, 9)[ok], (9,))
    if state.seen is not None:
        add = seen[ok].astype(np.int64)
        old = state.seen.astype(np.int64)
        scans = total(old[:, 0], add[:, 0], ())
        first, last = np.full(len(new), MAX_ID, np.int64), np.full(len(new), -1, np.int64)
        np.minimum.at(first, inverse, np.concatenate([old[:, 1], add[:, 1] + int(id_offset)]))
        np.maximum.at(last, inverse, np.concatenate([old[:, 2], add[:, 2] + int(id_offset)]))
        state.seen = np.stack([scans, first, last], 1).astype(np.int32)
    state.keys = new
    return int((~ok).sum())


def merge(a, b, id_offset=None):
    """-> a new State: a, plus the records of b with its scans numbered on from id_offset (None: a.num_scans), plus b's skip counters.
    b must hold the blocks that a keeps."""
    id_offset = a.num_scans if id_offset is None else int(id_offset)
    assert a.voxel == b.voxel and a.channels == b.channels and id_offset >= 0 and id_offset + b.num_scans <= MAX_ID
    out = a.copy()
    rows = export(b)
    rejected = add_records(out, rows['keys'], rows['counts'], rows['sums'], rows['moments'], rows['observations'], id_offset)
    assert rejected == 0
    for k in SKIPS:
        out.skipped[k] += b.skipped[k]
    out.num_scans = max(a.num_scans, id_offset + b.num_scans)
    return out


def same(a, b):
    """Every array and counter of two states, for the tests: -> the list of names that differ."""
    diff = [k for k in ('keys', 'counts', 'sums', 'moments', 'seen')
            if not ((getattr(a, k) is None and getattr(b, k) is None) or
                    (getattr(a, k) is not None and getattr(b, k) is not None and getattr(a, k).dtype == getattr(b, k).dtype
                     and np.array_equal(getattr(a, k), getattr(b, k))))]
    return diff + [k for k in ('integrated', 'skipped', 'num_scans') if getattr(a, k) != getattr(b, k)]
