"""gate_recall_kernel on its own (include/slideo_amd.h "Gate memory"): slideo_gate_recall_walk against the restatement's integer walk
(tests/gate_memory_ref.py), exact equality of every output — flags, ssd_a per frame, refs, the slot occupants behind the unit, head,
count, anchor slot and d.

The cases are tests/gate_memory_cases.py's: frames and memory entries as integer vectors of 8 components, as
tests/test_gpu_gate_settle_kernels.py builds its own tables, so dot products and norms are exact integers.  n = 1, 2, 63, 64, 65,
130, 300 around the 64-lane window; M = 1, 2, 3, 64; from the state "none", from a carried memory that is partly full and from a
full one whose head is not 0; no settle, and a settle with caps 0, 4 and 2**30; and tables that force exact SSD ties between two
entries (the ordinal decides), a best entry at T_c - 1 and at T_c, a unit with more than M matches followed by returns to an evicted
and to a surviving in-unit entry, a recall of a carried entry followed by frames compared against that carried anchor, all frames
away and deferred, and no frame away.  tests/test_gate_memory_abi.py asserts on the restatement that every branch occurs."""
import numpy as np
import pytest

import gate_memory_cases as cases
import gate_memory_ref as mref
from conftest import small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain(capi):
    m = capi.Matcher(small_cfg(capi))                            # the tap needs no pages
    yield m
    m.close()


def _run(m, c):
    return m.gate_recall_walk(c["dot"], c["norm"], c["mdot"], c["mnorm"], c["ordinals"], c["count"], c["head"], c["anchor"], c["prev_ssd0"], c["thr_c"],
                              c["thr_s"], c["max_defer"], c["d_in"], c["none"], c["t0"])


def _check(m, c):
    fl, ssd, refs, kind, occ, head, count, anc, d = c["want"]
    got = _run(m, c)
    what = c["what"]
    assert np.array_equal(got[0], fl), (what, "flags", np.nonzero(got[0] != fl)[0][:8])
    assert np.array_equal(got[1].astype(np.int64), ssd), (what, "SSDs", np.nonzero(got[1].astype(np.int64) != ssd)[0][:8])
    assert np.array_equal(got[2], refs), (what, "refs", np.nonzero(got[2] != refs)[0][:8])
    assert np.array_equal(got[3], occ), (what, "occupants", got[3][:c["M"]], occ[:c["M"]])
    assert got[4:] == (head, count, anc, d), (what, got[4:], (head, count, anc, d))


@pytest.mark.parametrize("n", cases.NS)
def test_walk(plain, n):
    ran = 0
    for c in cases.all_stream_cases():
        if c["n"] == n:
            _check(plain, c)
            ran += 1
    assert ran == len(cases.MS) * len(cases.STATES) * len(cases.SETTLES)


def test_forced_tables(plain):
    for c in cases.forced_cases():
        _check(plain, c)


def test_m_1_is_the_shipped_walk(plain):
    """With one slot the walk is gate_settle_kernel's: the same flags, SSDs and count from the same tables, the carried column in
    place of the carried anchor's SSDs."""
    ran = 0
    for c in cases.all_stream_cases():
        if c["M"] != 1 or c["n"] > 130:
            continue
        carried = np.concatenate([c["mtable"][:, 0], [c["prev_ssd0"]]]).astype(np.uint64)
        want = plain.gate_settle_walk(c["dot"], c["norm"], carried, c["thr_c"], c["thr_s"], c["max_defer"], c["d_in"], c["none"])
        got = _run(plain, c)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[7] == want[3], c["what"]
        assert not (c["want"][3] == mref.RECALLED).any()
        ran += 1
    assert ran >= 60


def test_walk_refusals(capi, plain):
    c = dict(cases.forced_cases()[0])
    for key, bad in (("count", 0), ("count", 4), ("head", 3), ("anchor", 3), ("d_in", 1), ("max_defer", -1)):
        with pytest.raises(capi.SlideoError) as e:
            _run(plain, dict(c, **{key: bad}))
        assert e.value.code == 1, key
    with pytest.raises(capi.SlideoError) as e:
        plain.gate_recall_walk(c["dot"], c["norm"], np.zeros((c["n"], 65)), np.zeros(65), np.zeros(65, np.int64), 1, 1, 0, 0, 0, 0, 0)
    assert e.value.code == 1, "65 slots"
