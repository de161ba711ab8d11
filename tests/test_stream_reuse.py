"""tools/stream_reuse.py without a GPU: the headline's totals follow from the layout constants of csrc/rt_wavefront.hip.h (a queue record of two float4 per ray slot, an
8-byte traversal word per ray, 4 + 1 bytes per shaded segment, a 32-byte first-shade record per pixel slot, a float4 per pixel), the chain is the one csrc/rt_still.h
plans for a resumed still view, and the streams the table puts out of reach are the once-per-frame ones and segment 0's LS / SID."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stream_reuse as sr  # noqa: E402

PATHS = 2 * 240 * 68 * 64                                             # two sub-frames of 540 rows: 240 x 68 tiles of 64 pixel slots each


@pytest.fixture(scope="module")
def headline():
    return sr.table(1920, 1080, 3, 2, 2)


def test_headline_totals(headline):
    assert headline["paths"] == PATHS == 2088960
    g = sr.group_totals(headline)
    assert g == dict(QR=2 * 32 * PATHS, M=2 * 8 * PATHS, LS=4 * 4 * PATHS, SID=4 * PATHS, DCH=PATHS, S0=32 * PATHS, frame=16 * 1920 * 1080)
    assert sum(g.values()) == headline["frame_footprint"] == 133 * PATHS + 16 * 1920 * 1080 == 311009280  # every stream of a resumed frame is touched: 311 MB through 268
    assert headline["frame_footprint"] > sr.CACHE > g["QR"] + g["M"] + g["DCH"]


def test_headline_chain(headline):
    names = [n for n, _ in headline["launches"]]
    assert names == ["wf_advance<resume>", "wf_travq@1", "wf_advance@1", "wf_travq@2", "wf_advance@2", "wf_travq@3", "wf_advance@3", "wf_travq@4", "wf_advance<close>@4"]
    first = [n for n, _ in sr.table(1920, 1080, 3, 2, 0)["launches"]]
    assert first[:3] == ["wf_advance<first>", "wf_travq@0", "wf_advance@0"] and first[-1] == "wf_advance<close>@4" and len(first) == 11


def test_reach(headline):
    reach = {r["stream"]: r["reach"] for r in headline["rows"]}
    for s in ("QR.y", "QR.x", "M.y", "M.x", "DCH"):
        assert reach[s], s                                            # the path state one launch hands the next
    for s in ("S0", "frame"):
        assert not reach[s], s                                        # a frame away
    segs = headline["segs"]
    far = [s for s in range(segs) if not reach[f"LS[{s}]"]]
    assert far == [s for s in range(segs) if not reach[f"SID[{s}]"]] == [0]    # the resume launch, which writes them, also streams the records through


def test_everything_fits_a_small_frame():
    t = sr.table(512, 512, 3, 2, 2)
    assert all(r["reach"] for r in t["rows"]) and t["frame_footprint"] < sr.CACHE
