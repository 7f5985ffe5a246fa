"""Which chain of launches each option combination produces, held to a recording (tests/golden/frame_forms.json, made by
tests/golden/make_frame_forms.py with the library as it was before the frame dispatch moved to crt_frames.cpp).  The other suites hold
the frames to their numpy references; this one pins the frame's FORM: the sum's bits, crt_debug_launch_info's four words, the number of
timed launches and the ray counts, for one axis at a time off the defaults on a small tree, a tree of 64+ nodes and an instanced scene."""
import json
import os

import pytest

import frame_forms as ff

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_forms.json")) as _f:
    RECORDED = json.load(_f)

CONFIGS = ff.configurations()


@pytest.fixture(scope="module")
def scenes(cr, cornell, cornell_data, tess8, tess40):
    return ff.Scenes(cr, cornell, cornell_data, [("tess8",) + tuple(tess8), ("tess40",) + tuple(tess40)])


def test_the_recording_covers_every_configuration():
    assert sorted(RECORDED["records"]) == sorted(cid for cid, _ in CONFIGS)
    assert RECORDED["frame"] == [ff.W, ff.H] and ff.H % 16 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [cid for cid, _ in CONFIGS])
def test_frame_form_is_the_recorded_one(scenes, cid):
    cfg = dict(CONFIGS)[cid]
    want = RECORDED["records"][cid]
    got = ff.observe(scenes, cfg)
    if cfg["scene"] == "big":
        assert scenes.big_name == RECORDED["big"]
    print(cid, got)
    if "sha256" not in want:                 # a configuration whose sums differed between two recordings of the same library
        got.pop("sha256", None)
    assert got == want
