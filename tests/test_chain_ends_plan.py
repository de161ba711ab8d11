"""The closing kernel in the chain plan (csrc/rt_still.h still_plan, kAdvClose) without a GPU, through rth_still_replay: flag 8 of a chain event says the chain is a plain
one under RT_CHAIN_ENDS.  Only the wf_advance of the chain's last position changes, in every state of the still view and for every depth; without the flag the table is
the one tests/test_still_view_model.py pins."""
import pytest

from raytracinggpu_amd import hostlib

MESH, ROWS, HAS_Y, ENDS = 1, 2, 4, 8
PLAIN, STORE, CLOSE = 2, 3, 4


def _tables(segs, flags, frames=4, level=3):
    """per frame of a still view, the rows (position, ..., wf_advance, kill_x) of part 0's chain"""
    ev, first = [], []
    for _ in range(frames):
        first.append(len(ev) + 1)
        ev += [(0, level, 1, 1, 1), (1, 0, segs, flags)]
    _, rows = hostlib.still_replay(ev)
    return [[tuple(int(v) for v in r[1:9]) for r in rows if r[0] == e] for e in first]


@pytest.mark.parametrize("flags", [MESH | ROWS | HAS_Y, MESH, 0])
@pytest.mark.parametrize("segs", [1, 2, 3, 4, 16])
def test_only_the_last_position_changes(segs, flags):
    for level in (0, 1, 2, 3):
        off, on = _tables(segs, flags, level=level), _tables(segs, flags | ENDS, level=level)
        for a, b in zip(off, on):                          # fill, read and store, resume, resume
            assert len(a) == len(b) and a[-1][0] == b[-1][0] == segs
            assert a[:-1] == b[:-1]
            assert a[-1][6] == PLAIN and b[-1][6] == CLOSE and a[-1][:6] + a[-1][7:] == b[-1][:6] + b[-1][7:]
            assert sum(r[6] == CLOSE for r in b) == 1
        if level == 3:
            assert on[1][1][6] == STORE                    # the launch that stores the records stays at position 0, also in a chain of one segment


def test_a_chain_of_no_segments_has_no_position():
    assert _tables(0, MESH | ENDS, frames=1) == _tables(0, MESH, frames=1)
