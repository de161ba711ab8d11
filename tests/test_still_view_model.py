"""The still view's state machine and chain plan (csrc/rt_still.h) without a GPU, through the host library's rth_still_replay: sequences of chunks, chains and edits with
made-up keys, their counters and the launch table of every chain.

The sequences are the ones whose outcomes tests/test_gpu_first_{hit,shadow,shade}_cache.py assert on the device, and the expected counters are theirs (in chains: two
parts, so twice the figures those files give per sub-frame); the launch tables are written out from what those files' docstrings and csrc/rt_still.h's rules say a chain
enqueues.  Counters read (used, filled, ineligible, key_misses); a table row reads (position, traversal launch, window, it writes the hit block, m0, x0, wf_advance,
kill_x), position -1 being the opening launch."""
import numpy as np
import pytest

from raytracinggpu_amd import hostlib

HIT, SHADOW, SHADE = 0, 1, 2
OFF, FILL, USE = 0, 1, 2
NONE, Y, X = 0, 1, 2
BEGIN, RESUME, PLAIN, STORE = 0, 1, 2, 3
MESH, ROWS, HAS_Y = 1, 2, 4
ALL = MESH | ROWS | HAS_Y


def chunk(level=3, ray=1, scene=1, rest=1, parts=2, chains=1, segs=3, flags=ALL):
    """one frame of one chunk: begin, then the chains of every sample chunk for all parts"""
    return [(0, level, ray, scene, rest)] + [(1, j, segs, flags) for _ in range(chains) for j in range(parts)]


MESH_EDIT, SHADING_EDIT = [(2,)], [(3,)]


def moved(level):
    return [(4, level)]


def deltas(*steps):
    """how far the counters of the three levels moved over each step (a list of events), as a list of 3 x 4 arrays"""
    out, ev, before = [], [], np.zeros((3, 4), np.int64)
    for s in steps:
        ev = ev + list(s)
        after, _ = hostlib.still_replay(ev)
        out.append(after - before)
        before = after
    return out


def tables(*steps):
    """(modes, rows without the event number and the modes) of every chain of the LAST step"""
    ev = [e for s in steps for e in s]
    _, rows = hostlib.still_replay(ev)
    first = len(ev) - len(steps[-1])
    out = {}
    for r in rows:
        if r[0] >= first:
            out.setdefault(int(r[0]), (tuple(int(v) for v in r[9:12]), []))[1].append(tuple(int(v) for v in r[1:9]))
    return [out[k] for k in sorted(out)]


def want(level_rows):
    return np.array(level_rows, np.int64)


def test_a_still_view_of_five_frames():
    d = deltas(*[chunk()] * 5)
    np.testing.assert_array_equal(d[0], want([[0, 2, 0, 0], [0, 2, 0, 0], [0, 0, 0, 0]]))       # fills the two older levels; an eligible chain that neither stores nor resumes counts nowhere
    np.testing.assert_array_equal(d[1], want([[2, 0, 0, 0], [2, 0, 0, 0], [0, 2, 0, 0]]))       # reads them and stores the records
    for k in (2, 3, 4):
        np.testing.assert_array_equal(d[k], want([[2, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0]]))   # resumes: skipped in the two older counters as well


def test_a_light_edit():
    still = [chunk()] * 3
    d = deltas(*still, chunk(scene=2), chunk(scene=2), chunk(scene=2))
    np.testing.assert_array_equal(d[3], want([[2, 0, 0, 0], [0, 2, 0, 1], [0, 0, 0, 1]]))       # a shadow miss and refill only: the camera rays' hits are kept
    np.testing.assert_array_equal(d[4], want([[2, 0, 0, 0], [2, 0, 0, 0], [0, 2, 0, 0]]))
    np.testing.assert_array_equal(d[5], want([[2, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0]]))       # two frames later the chains resume
    d = deltas(*still, chunk(rest=2), SHADING_EDIT + chunk(rest=2))                             # eps or an elision rule; normals, UVs or texels behind a pointer
    for k in (3, 4):
        np.testing.assert_array_equal(d[k], want([[2, 0, 0, 0], [0, 2, 0, 1], [0, 0, 0, k == 3]]))


@pytest.mark.parametrize("frames_before", [1, 2, 3])
def test_a_mesh_edit(frames_before):
    d = deltas(*[chunk()] * frames_before, MESH_EDIT + chunk(), chunk(), chunk())
    stored = frames_before >= 2                        # the shade counter's fourth value moves only if records were stored
    np.testing.assert_array_equal(d[frames_before], want([[0, 2, 0, 1], [0, 2, 0, 1], [0, 0, 0, int(stored)]]))
    np.testing.assert_array_equal(d[frames_before + 1], want([[2, 0, 0, 0], [2, 0, 0, 0], [0, 2, 0, 0]]))
    np.testing.assert_array_equal(d[frames_before + 2], want([[2, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0]]))


def test_a_new_ray_key_replaces_everything():
    """a moved camera, another row share, other streams: the ray key.  Two shares alternating are a miss every time"""
    d = deltas(*[chunk()] * 3, *[chunk(ray=2 + k % 2) for k in range(6)], chunk(ray=3), chunk(ray=3))
    np.testing.assert_array_equal(d[3], want([[0, 2, 0, 1], [0, 2, 0, 1], [0, 0, 0, 1]]))
    for k in range(4, 9):
        np.testing.assert_array_equal(d[k], want([[0, 2, 0, 1], [0, 2, 0, 1], [0, 0, 0, 0]]))
    np.testing.assert_array_equal(d[9], want([[2, 0, 0, 0], [2, 0, 0, 0], [0, 2, 0, 0]]))
    np.testing.assert_array_equal(d[10], want([[2, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0]]))


def test_an_edit_before_every_one_of_six_frames():
    """the key never holds for two chains: no chain pays for a fill, and only the first edit found records to drop"""
    d = deltas(*[chunk()] * 3, [e for k in range(6) for e in chunk(scene=10 + k)], chunk(scene=15), chunk(scene=15))
    np.testing.assert_array_equal(d[3], want([[12, 0, 0, 0], [0, 12, 0, 6], [0, 0, 0, 1]]))
    np.testing.assert_array_equal(d[4][SHADE], [0, 2, 0, 0])
    np.testing.assert_array_equal(d[5][SHADE], [2, 0, 0, 0])


def test_five_samples_as_five_chains_per_part():
    d = deltas(*[chunk(chains=5, segs=13)] * 3)
    np.testing.assert_array_equal(d[0], want([[8, 2, 0, 0], [8, 2, 0, 0], [0, 0, 0, 0]]))       # (the records' buffer is not allocated yet: nothing to store into)
    np.testing.assert_array_equal(d[1], want([[10, 0, 0, 0], [10, 0, 0, 0], [8, 2, 0, 0]]))     # the frame's first chain stores, its other four resume
    np.testing.assert_array_equal(d[2], want([[10, 0, 0, 0], [10, 0, 0, 0], [10, 0, 0, 0]]))


def test_a_new_allocation_empties_its_own_level():
    still = [chunk()] * 3
    d = deltas(*still, moved(SHADE) + chunk(), chunk())
    np.testing.assert_array_equal(d[3], want([[2, 0, 0, 0], [2, 0, 0, 0], [0, 2, 0, 1]]))
    np.testing.assert_array_equal(d[4], want([[2, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0]]))
    d = deltas(*still, moved(SHADOW) + chunk())
    np.testing.assert_array_equal(d[3], want([[2, 0, 0, 0], [0, 2, 0, 1], [0, 0, 0, 1]]))
    d = deltas(*still, moved(HIT) + chunk())
    np.testing.assert_array_equal(d[3], want([[0, 2, 0, 1], [0, 2, 0, 1], [0, 0, 0, 1]]))


def test_level_0_counts_as_ineligible_and_touches_nothing():
    """a batch, a counting run, a frame under rt_stats_enable, sigma != 0 (the list chains of rt_render_counts* do not even count)"""
    d = deltas(*[chunk()] * 3, chunk(level=0, ray=9, scene=9, chains=3), chunk())
    np.testing.assert_array_equal(d[3], want([[0, 0, 6, 0]] * 3))
    np.testing.assert_array_equal(d[4], want([[2, 0, 0, 0]] * 3))
    for segs in (0, 1, 3, 16):
        for modes, rows in tables(*[chunk()] * 3, chunk(level=0, segs=segs)):
            assert modes == (OFF, OFF, OFF)
            plain = [(-1, 0, NONE, 0, 0, 0, BEGIN, 0)] + [(it, 1, Y if it == 0 else X if it == segs else NONE, 0, 0, 0, PLAIN, 0) for it in range(segs + 1 if segs else 0)]
            assert rows == plain


def test_shaded_records_off():
    """a textured scene: level 2.  The shade counter counts ineligible, the others are as before"""
    d = deltas(*[chunk(level=2)] * 3)
    np.testing.assert_array_equal(d[0], want([[0, 2, 0, 0], [0, 2, 0, 0], [0, 0, 2, 0]]))
    for k in (1, 2):
        np.testing.assert_array_equal(d[k], want([[2, 0, 0, 0], [2, 0, 0, 0], [0, 0, 2, 0]]))
    d = deltas(*[chunk(level=1)] * 2)                  # RT_FIRST_SHADOW_CACHE=0
    np.testing.assert_array_equal(d[1], want([[2, 0, 0, 0], [0, 0, 2, 0], [0, 0, 2, 0]]))
    d = deltas(*[chunk()] * 3, chunk(level=2), chunk())   # the texture set and dropped again is a shading edit besides: here the levels alone
    np.testing.assert_array_equal(d[3], want([[2, 0, 0, 0], [2, 0, 0, 0], [0, 0, 2, 0]]))
    np.testing.assert_array_equal(d[4], want([[2, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0]]))


def _one(t):
    assert t[0] == t[1]                                # both parts' chains are alike
    return t[0]


def test_the_launch_tables_of_one_segment():
    """num_bounce 0"""
    f = chunk(segs=1)
    assert _one(tables(f)) == ((FILL, FILL, OFF), [(-1, 0, NONE, 0, 1, 0, BEGIN, 0), (0, 1, Y, 1, 1, 1, PLAIN, 0), (1, 1, X, 0, 0, 1, PLAIN, 0)])
    # a reading chain of one segment enqueues neither traversal launch
    assert _one(tables(f, f)) == ((USE, USE, FILL), [(-1, 0, NONE, 0, 1, 0, BEGIN, 0), (0, 0, NONE, 0, 1, 2, STORE, 0), (1, 0, NONE, 0, 0, 2, PLAIN, 0)])
    # a resumed one: the resume kernel only folds, the table starts at position 1
    assert _one(tables(f, f, f)) == ((USE, USE, USE), [(-1, 0, NONE, 0, 0, 0, RESUME, 0), (1, 0, NONE, 0, 0, 0, PLAIN, 0)])
    g = chunk(level=2, segs=1)
    assert _one(tables(g, g)) == ((USE, USE, OFF), [(-1, 0, NONE, 0, 1, 0, BEGIN, 0), (0, 0, NONE, 0, 1, 2, PLAIN, 0), (1, 0, NONE, 0, 0, 2, PLAIN, 0)])
    h = chunk(level=1, segs=1)
    assert _one(tables(h, h)) == ((USE, OFF, OFF), [(-1, 0, NONE, 0, 1, 0, BEGIN, 0), (0, 0, NONE, 0, 1, 0, PLAIN, 0), (1, 1, X, 0, 0, 0, PLAIN, 0)])


@pytest.mark.parametrize("flags", [ALL, MESH | ROWS, MESH | HAS_Y, MESH])
def test_the_launch_tables_of_two_and_more_segments(flags):
    """num_bounce 1 and 2, with and without RT_TRAVQ_ROWS, with and without a Y window that is not every row"""
    rows, has_y = bool(flags & ROWS), bool(flags & HAS_Y)
    wy, wx = (Y if rows and has_y else NONE), (X if rows else NONE)
    for segs in (2, 3):
        f = chunk(segs=segs, flags=flags)
        mid = [(it, 1, NONE, 0, 0, 0, PLAIN, 0) for it in range(2, segs)]
        last = [(segs, 1, wx, 0, 0, 0, PLAIN, 0)]
        assert _one(tables(f)) == ((FILL, FILL, OFF), [(-1, 0, NONE, 0, 1, 0, BEGIN, 0), (0, 1, wy, 1, 1, 1, PLAIN, 0), (1, 1, NONE, 0, 0, 1, PLAIN, 0)] + mid + last)
        assert _one(tables(f, f)) == ((USE, USE, FILL), [(-1, 0, NONE, 0, 1, 0, BEGIN, 0), (0, 0, NONE, 0, 1, 2, STORE, 0), (1, 1, NONE, 0, 0, 2, PLAIN, 0)] + mid + last)
        # a resumed chain starts at position 1 and takes the Y window there; where there is none it sets kill_x
        assert _one(tables(f, f, f)) == ((USE, USE, USE), [(-1, 0, NONE, 0, 0, 0, RESUME, 0 if wy else 1), (1, 1, wy, 0, 0, 0, PLAIN, 0)] + mid + last)


def test_a_scene_without_a_mesh_has_no_traversal_launch():
    for modes, rows in tables(chunk(level=0, segs=2, flags=ROWS | HAS_Y)):
        assert rows == [(-1, 0, NONE, 0, 0, 0, BEGIN, 0)] + [(it, 0, NONE, 0, 0, 0, PLAIN, 0) for it in range(3)]
