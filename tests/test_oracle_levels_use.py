"""The use case of include/slideo_amd.h "Frame levels" on the CPU restatement (oracle/): a dim, low-contrast recording loses every
frame at the similarity test; the per-channel stretch learnt from the darkened frames' own histogram (tests/levels_ref.py) brings
every verdict back.  This pins the restatement the GPU test (tests/test_gpu_levels.py) compares the library with; it needs no
library call of the feature."""
import numpy as np
import pytest

import levels_ref as R
from conftest import small_cfg

TRUTH = [-1, 2, 3, 0, -1, 2, 3, 0]


@pytest.fixture(scope="module")
def db(oracle, cfg0_data):
    pages, _, _, _ = cfg0_data
    d = oracle.PageDB(small_cfg(oracle))
    d.add_pages(pages)
    d.finalize()
    return d


def test_the_synthetic_truth_is_what_the_issue_states(cfg0_data, db):
    _, frames, truth, _ = cfg0_data
    assert [int(t) for t in truth] == TRUTH
    assert db.match_frames(frames)["page_idx"].tolist() == TRUTH


def test_a_dim_recording_loses_every_frame_and_learnt_levels_bring_them_back(cfg0_data, db):
    _, frames, _, _ = cfg0_data
    dark = R.darken(frames)
    assert db.match_frames(dark)["page_idx"].tolist() == [-1] * 8
    lo, hi = R.points(R.histogram(dark), 10000, 10000)
    assert (lo, hi) == ([34] * 3, [106] * 3)
    lut = R.stretch_lut(lo, hi)
    got = db.match_frames(R.apply(dark, lut))
    assert got["page_idx"].tolist() == TRUTH
