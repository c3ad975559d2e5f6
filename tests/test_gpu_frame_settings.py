"""The six frame settings (working size, frame region, frame mask, frame mask scope, direct similarity, direct scope) as ordered
pairs of set calls, on a Matcher and on a Group over the same device twice, observed through the public getters and calls only.

For every ordered pair of the twelve calls (each setting with a value that is in force and a value that is off): the return code
of each call, the settings the getters report afterwards, whether the kept frames of a mask call and the gate state survived the
second call, and that a gated call afterwards returns what a fresh matcher under the same final settings returns.  PAIRS is the
literal table of tools/frame_settings_hostcheck.cpp, written from include/slideo_amd.h: with these values no pair is refused, and
what a call ends depends on its setting alone — working size K(ept frames) G(ate state) M(ap generation, not observable here),
region K G, mask and mask scope K M, the direct settings nothing.

small_area is 2000 so that the 320x180 frames, their 160x90 reduction and the 128x72 region output all have a small image.  Under
some final settings frame calls are refused (a 320x180 mask beside frames analysed at 160x90 or 128x72): the handle and the fresh
matcher must then be refused with the same code.
"""
import numpy as np
import pytest

from conftest import small_cfg
from slideo_amd import _capi

pytestmark = pytest.mark.gpu

W, H = 320, 180
WS = (160, 90)
OUT = (128, 72)
QUAD = [(32, 18), (287, 18), (287, 161), (32, 161)]      # axis-aligned
MASK = np.full((H, W), 255, np.uint8)
MASK[100:150, 200:300] = 0                              # one rectangular hole

CALLS = ["ws_on", "ws_off", "region_on", "region_off", "mask_on", "mask_off", "scope_on", "scope_off", "t_on", "t_off", "dscope_on", "dscope_off"]
ROW = ["0:KGM", "0:KGM", "0:KG-", "0:KG-", "0:K-M", "0:K-M", "0:K-M", "0:K-M", "0:---", "0:---", "0:---", "0:---"]
PAIRS = {a: dict(zip(CALLS, ROW)) for a in CALLS}       # first call down, second call across: "<code>:<ends>"
DEFAULTS = dict(ws=(0, 0), region=None, mask=None, scope=_capi.MASK_DETECT, t=np.float32(0.0), dscope=_capi.DIRECT_WHOLE)


def _do(h, call):
    {"ws_on": lambda: h.set_working_size(*WS), "ws_off": lambda: h.set_working_size(0, 0),
     "region_on": lambda: h.set_frame_region(W, H, QUAD, *OUT), "region_off": h.clear_frame_region,
     "mask_on": lambda: h.set_frame_mask(MASK), "mask_off": lambda: h.set_frame_mask(None),
     "scope_on": lambda: h.set_frame_mask_scope(_capi.MASK_DETECT | _capi.MASK_GATE), "scope_off": lambda: h.set_frame_mask_scope(_capi.MASK_DETECT),
     "t_on": lambda: h.set_direct_similarity(0.9), "t_off": lambda: h.set_direct_similarity(0.0),
     "dscope_on": lambda: h.set_direct_scope(_capi.DIRECT_VALID), "dscope_off": lambda: h.set_direct_scope(_capi.DIRECT_WHOLE)}[call]()


def _expected(settings, call):
    s = dict(settings)
    key, val = {"ws_on": ("ws", WS), "ws_off": ("ws", (0, 0)), "region_on": ("region", (W, H) + OUT), "region_off": ("region", None),
                "mask_on": ("mask", (W, H)), "mask_off": ("mask", None), "scope_on": ("scope", 3), "scope_off": ("scope", 1),
                "t_on": ("t", np.float32(0.9)), "t_off": ("t", np.float32(0.0)), "dscope_on": ("dscope", 1), "dscope_off": ("dscope", 0)}[call]
    s[key] = val
    return s


def _code(fn):
    try:
        return 0, fn()
    except _capi.SlideoError as e:
        return e.code, None


def _reported(h):
    """What the getters report; a group: what every member reports, the members agreeing."""
    if isinstance(h, _capi.Group):
        got = [_reported(h.member(i)) for i in range(len(h.devices))]
        assert all(g == got[0] for g in got), got
        return got[0]
    reg = h.frame_region
    return dict(ws=tuple(h.working_size), region=None if reg is None else (reg[0], reg[1], reg[3], reg[4]), mask=h.frame_mask_info,
                scope=h.frame_mask_scope, t=np.float32(h.direct_similarity), dscope=h.direct_scope)


def _gated(h, frames):
    """A gated call from the state "none": (code, flags, similarities, verdicts) as comparable bytes."""
    h.gate_reset()
    code, out = _code(lambda: h.match_changed_frames(frames))
    return (code,) if code else (0, out[0].tobytes(), out[1].tobytes(), out[2].tobytes())


@pytest.fixture(scope="module")
def data(synth):
    pages = synth.pages(3, 400, 225)
    frames, _, _ = synth.frames(pages, 4, W, H)
    frames[1] = frames[0]                                # an unchanged frame among the four
    return pages, np.ascontiguousarray(frames)


def _make(kind, pages):
    cfg = small_cfg(_capi, nfeatures=300, small_area=2000)
    h = _capi.Matcher(cfg, device=0) if kind == "matcher" else _capi.Group(cfg, devices=[0, 0])
    h.add_pages(list(pages))
    h.finalize()
    return h


@pytest.fixture(scope="module")
def fresh(data):
    """What a fresh matcher under the given final settings returns for the gated call, once per distinct settings."""
    pages, frames = data
    cache = {}

    def get(calls):
        key = tuple(sorted(c for c in calls if c.endswith("_on")))
        if key not in cache:
            m = _make("matcher", pages)
            for c in key:
                _do(m, c)
            cache[key] = _gated(m, frames)
            m.close()
        return cache[key]
    return get


@pytest.mark.parametrize("kind", ["matcher", "group"])
def test_every_ordered_pair_of_set_calls(kind, data, fresh):
    pages, frames = data
    h = _make(kind, pages)
    for a in CALLS:
        for b in CALLS:
            for c in CALLS[1::2]:                        # every setting off: the defaults
                _do(h, c)
            assert _reported(h) == DEFAULTS, (a, b)
            assert _code(lambda: _do(h, a))[0] == 0, (a, b)
            want = _expected(DEFAULTS, a)
            assert _reported(h) == want, (a, b)
            # a gate state and, behind it, the kept frames of a mask call (a gated call may reuse the mask call's buffer)
            h.gate_reset()
            h.match_changed_frames(frames)
            h.changed_mask(frames)
            code, ends = PAIRS[a][b].split(":")
            assert _code(lambda: _do(h, b))[0] == int(code), (a, b)
            if int(code) == 0:
                want = _expected(want, b)
            assert _reported(h) == want, (a, b)
            kept = _code(lambda: h.match_kept_frames([0]))[0]
            gate = _code(h.gate_last_small)[0]
            assert (kept == 4) == (ends[0] == "K") and kept in (0, 4), (a, b, kept)
            assert (gate == 4) == (ends[1] == "G") and gate in (0, 4), (a, b, gate)
            final = {a.rsplit("_", 1)[0]: a}
            final[b.rsplit("_", 1)[0]] = b                   # (the second call of a setting replaces the first)
            assert _gated(h, frames) == fresh(final.values()), (a, b)
    h.close()


# The refused combinations of tools/frame_settings_hostcheck.cpp (COMBOS) on real handles: the calls before, the call under test,
# its code.  A refused call leaves every getter — on a group, every member's — as it was.
COMBOS = [
    (["mask_on", "scope_on"], "t_on", 5), (["t_on", "scope_on"], "mask_on", 5), (["t_on", "mask_on"], "scope_on", 5),
    (["dscope_on", "mask_on", "scope_on"], "t_on", 0), (["dscope_on", "mask_on", "scope_on", "t_on"], "dscope_off", 5),
    (["dscope_on", "mask_on", "scope_on", "t_on"], "mask_off", 0),
    (["region_on"], "ws_small", 5), (["ws_small"], "region_on", 5), (["ws_on"], "region_on", 0),
    ([], "ws_bad", 1), ([], "scope_bad", 1), ([], "t_bad", 1), ([], "dscope_bad", 1), ([], "region_bad", 1),
]
EXTRA = {"ws_small": lambda h: h.set_working_size(100, 60), "ws_bad": lambda h: h.set_working_size(0, 90),
         "scope_bad": lambda h: h.set_frame_mask_scope(4), "t_bad": lambda h: h.set_direct_similarity(1.5),
         "dscope_bad": lambda h: h.set_direct_scope(2), "region_bad": lambda h: h.set_frame_region(W, H, [1, 0, 0, 0, 1, 0, 1, 0, -10], *OUT)}


@pytest.mark.parametrize("kind", ["matcher", "group"])
def test_refused_combinations(kind, data):
    pages, _ = data
    h = _make(kind, pages)

    def do(call):
        return EXTRA[call](h) if call in EXTRA else _do(h, call)
    for before, call, code in COMBOS:
        for c in CALLS[1::2]:
            _do(h, c)
        for c in before:
            do(c)
        was = _reported(h)
        assert _code(lambda: do(call))[0] == code, (before, call)
        if code != 0:
            assert _reported(h) == was, (before, call)
    h.close()
