"""Which call spends which one-shot flag (tf_chain_next, tf_hold_next, tf_frames_next): the table that stands at spend() in
csrc/teeflow_engine.hip.h, pinned as a table.  One row per call family; for each call of a row all three flags are armed on a DualTVL1
handle with useInitialFlow set and four frames held, the call is made, and three probes say which flags are still armed.

The probes do no device work, each is refused on the host, and they run in the order chain, frames, hold, because each spends what the
ones before it have already read:
  chain   a pairs call with H = 0 is refused with "tf_chain_next arms a sequence call" if the flag is armed, with "bad sizes" if not
          (check_call tests the chain before the sizes); a pairs call spends the chain flag alone.
  frames  a NULL-pointer tf_echo_frames of 1 x 1 x 1 is refused by take_frames, with a message that names the call, if the flag is armed
          (its range never is one frame of 1 x 1), and with no message -- the last error stays the sentinel left just before -- if not;
          a frames-taking call spends the frames flag alone.
  hold    tf_calc_seq_rgb with N = 1, the frames flag being spent by now, is refused with "only a float16 study call can leave its
          payload held" if the flag is armed, with "a sequence needs at least 2 frames" if not.

Most calls of a row are refused before any GPU work (a row spends its flags refused or not); each row also makes one successful call at
the size of the chain case "one" (tests/tvl1_chain_cases.py: four frames of 72 x 88, one pyramid level).  Nothing here provokes a
fault: every call is well-formed or refused on the host."""
import ctypes as C

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tests import tvl1_chain_cases as CC

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = _lib.TF_OK, _lib.TF_ERR_INVALID_ARG, _lib.TF_ERR_UNSUPPORTED
ALL = frozenset({"chain", "hold", "frames"})
# family -> the flags a call of it spends, refused or not; every other armed flag stays armed
SPENDS = {
    "pairs-seq": frozenset({"chain"}),
    "study": ALL,
    "lock-step": ALL,
    "frames-tail": frozenset({"frames"}),
    "other": frozenset(),
}
SENTINEL = b"armed_matrix_probe"


class Rig:
    """the handle, the arrays the calls point at, and the probes"""

    def __init__(self):
        import tee_optical_flow_amd as T
        self.gray = CC.frames("one")
        self.rgb = np.ascontiguousarray(CC.rgb_of(self.gray))
        self.N, self.H, self.W = self.gray.shape
        self.eng = T.DenseFlow(**CC.overrides("one"))
        self.eng.setUseInitialFlow(True)
        self.L, self.h = self.eng._L, self.eng._h
        self.flow = np.zeros((self.N, self.H, self.W, 2), np.float32)      # any call's flow destination (float32 or float16)
        self.out = np.zeros((self.N, self.H, self.W, 4), np.float32)       # any tail call's destination
        self.st = _lib.TfStats()
        assert self.L.tf_hold_frames(self.h, self.rgb.ctypes.data, _lib.FRAMES_FORMS["RGB"], 0, self.N, self.H, self.W) == OK

    def close(self):
        self.eng.close()

    def err(self):
        return self.L.tf_last_error(self.h).decode()

    def arm(self, flags=ALL):
        if "chain" in flags:
            assert self.L.tf_chain_next(self.h, 1) == OK, self.err()
        if "hold" in flags:
            assert self.L.tf_hold_next(self.h, 1) == OK
        if "frames" in flags:
            assert self.L.tf_frames_next(self.h, 0, self.N) == OK

    def armed(self):
        """-> the set of flags still armed; leaves none armed"""
        L, h, p = self.L, self.h, self.flow.ctypes.data
        on = set()
        rc = L.tf_calc_pairs(h, p, p, 1, 0, 0, p, None)
        assert rc == INVALID, (rc, self.err())
        if "tf_chain_next arms a sequence call" in self.err():
            on.add("chain")
        else:
            assert "bad sizes" in self.err(), self.err()
        assert L.tf_set_tuning(h, SENTINEL, 0) == INVALID and SENTINEL.decode() in self.err()
        rc = L.tf_echo_frames(h, None, 1, 1, 1, p)
        assert rc == INVALID, (rc, self.err())
        if self.err().startswith("tf_echo_frames: "):
            on.add("frames")
        else:
            assert SENTINEL.decode() in self.err(), self.err()
        rc = L.tf_calc_seq_rgb(h, p, 1, 8, 8, 1.0, p, None)
        if rc == UNSUPPORTED and "only a float16 study call can leave its payload held" in self.err():
            on.add("hold")
        else:
            assert rc == INVALID and "a sequence needs at least 2 frames" in self.err(), (rc, self.err())
        return on


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def _ptrs(*arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


# ---- the calls: name -> (family, the code it returns, call(rig) -> (code, what its message must hold or None)) ----------------------
def _refused_tail(name, args):
    """a frames-taking tail call refused for H = 0, after it has spent the frames flag"""
    def call(r):
        return getattr(r.L, name)(r.h, None, r.N, 0, r.W, *args(r)), None
    return call


def _seq_solved(r):
    rc = r.L.tf_calc_seq(r.h, r.gray.ctypes.data, r.N, r.H, r.W, 1.0, r.flow.ctypes.data, C.byref(r.st))
    return rc, None


def _study_solved(r):
    """the held frames, chained, left held: every flag honoured"""
    steps, reads = r.eng.counter("chain_steps"), r.eng.counter("frames_held_reads")
    echo = np.zeros((r.N, r.H, r.W), np.uint16)
    rc = r.L.tf_calc_seq_rgb_f16(r.h, None, r.N, r.H, r.W, 1.0, r.flow.ctypes.data, echo.ctypes.data, C.byref(r.st))
    shape = (C.c_longlong * _lib.HELD_SHAPE_LEN)()
    assert r.L.tf_held_shape(r.h, C.byref(shape)) == OK
    assert list(shape[:4]) == [r.N, r.H, r.W, r.N], "tf_hold_next was not honoured"
    assert r.eng.counter("chain_steps") - steps == r.N - 1, "tf_chain_next was not honoured"
    assert r.eng.counter("frames_held_reads") - reads == 1, "tf_frames_next was not honoured"
    return rc, None


def _chains(r, name="tf_calc_chains"):
    n = (C.c_int * 1)(r.N)
    if name == "tf_calc_chains_rgb":
        return r.L.tf_calc_chains_rgb(r.h, _ptrs(r.rgb), n, 1, r.H, r.W, 1.0, 0, _ptrs(r.flow), None, C.byref(r.st))
    return getattr(r.L, name)(r.h, _ptrs(r.gray), n, 1, r.H, r.W, 1.0, _ptrs(r.flow), C.byref(r.st))


def _other_solved(r):
    """the calls that hold and release: a study of two frames, a mask, the frames again"""
    flow16 = np.zeros((2, 8, 8, 2), np.uint16)
    mask = np.ones((2, 8, 8, 1), np.uint8)
    cent, area = np.zeros((2, 2)), np.zeros(2, np.int64)
    shape, fshape, warps = (C.c_longlong * _lib.HELD_SHAPE_LEN)(), (C.c_longlong * 4)(), C.c_double(1.0)
    for rc in (r.L.tf_hold_study(r.h, flow16.ctypes.data, 2, 8, 8, None, 0),
               r.L.tf_hold_mask(r.h, 0, mask.ctypes.data, 2, 1),
               r.L.tf_held_av_centroids(r.h, 0, 2, cent.ctypes.data, area.ctypes.data),
               r.L.tf_held_shape(r.h, C.byref(shape)),
               r.L.tf_release_study(r.h),
               r.L.tf_hold_frames(r.h, r.rgb.ctypes.data, _lib.FRAMES_FORMS["RGB"], 0, r.N, r.H, r.W),
               r.L.tf_held_frames_shape(r.h, C.byref(fshape)),
               r.L.tf_download_frames(r.h, r.out.ctypes.data),
               r.L.tf_set_tuning(r.h, b"queue_unit", 0),
               r.L.tf_get_param(r.h, _lib.PARAM_KEYS["warps"], C.byref(warps)),
               r.L.tf_set_param(r.h, _lib.PARAM_KEYS["warps"], warps.value)):
        assert rc == OK, r.err()
    return OK, None


def _other_refused(r):
    p = r.out.ctypes.data
    for rc in (r.L.tf_hold_study(r.h, None, 2, 8, 8, None, 0),
               r.L.tf_hold_mask(r.h, 99, p, 2, 1),
               r.L.tf_held_av_centroids(r.h, 99, 2, p, p),
               r.L.tf_hold_frames(r.h, None, 0, 0, r.N, r.H, r.W),
               r.L.tf_download_frames(r.h, None),
               r.L.tf_set_tuning(r.h, b"no_such_knob", 0),
               r.L.tf_set_param(r.h, 999, 0.0),
               r.L.tf_inflate(r.h, None, None, None, None, -1, 0, None, None),
               r.L.tf_deflate(r.h, None, -1, 0, None, 0, None, None, None)):
        assert rc == INVALID, (rc, r.err())
    return INVALID, None


CALLS = {
    # pairs and sequence calls through calc_entry / submit_entry
    "tf_calc_seq, one frame": ("pairs-seq", INVALID, lambda r: (r.L.tf_calc_seq(r.h, r.gray.ctypes.data, 1, r.H, r.W, 1.0, r.flow.ctypes.data, None), "at least 2 frames")),
    "tf_calc_pairs, armed": ("pairs-seq", INVALID, lambda r: (r.L.tf_calc_pairs(r.h, r.gray.ctypes.data, r.gray.ctypes.data, 1, r.H, r.W, r.flow.ctypes.data, None),
                                                       "tf_chain_next arms a sequence call")),
    "tf_submit_seq, no ticket": ("pairs-seq", INVALID, lambda r: (r.L.tf_submit_seq(r.h, r.gray.ctypes.data, r.N, r.H, r.W, 1.0, r.flow.ctypes.data, None), None)),
    "tf_calc_seq, solved": ("pairs-seq", OK, _seq_solved),
    # study calls
    "tf_calc_seq_rgb, one frame": ("study", INVALID, lambda r: (r.L.tf_calc_seq_rgb(r.h, None, 1, r.H, r.W, 1.0, r.flow.ctypes.data, None), "the call's frames are 1 x")),
    "tf_calc_seq_rgb_held, a pointer too": ("study", INVALID, lambda r: (r.L.tf_calc_seq_rgb_held(r.h, r.rgb.ctypes.data, r.N, r.H, r.W, 1.0, 0, None), "null frame pointer")),
    "tf_calc_seq_rgb_f16, solved": ("study", OK, _study_solved),
    # lock-step calls
    "tf_calc_chains": ("lock-step", UNSUPPORTED, lambda r: (_chains(r), "tf_frames_next was armed")),
    "tf_calc_chains_device": ("lock-step", UNSUPPORTED, lambda r: (_chains(r, "tf_calc_chains_device"), "tf_frames_next was armed")),
    "tf_calc_chains_rgb": ("lock-step", UNSUPPORTED, lambda r: (_chains(r, "tf_calc_chains_rgb"), "tf_frames_next was armed")),
    # frames-taking tail calls
    "tf_condition_frames, H = 0": ("frames-tail", INVALID, _refused_tail("tf_condition_frames", lambda r: (r.out.ctypes.data,))),
    "tf_echo_frames, H = 0": ("frames-tail", INVALID, _refused_tail("tf_echo_frames", lambda r: (r.out.ctypes.data,))),
    "tf_saliency_frames, H = 0": ("frames-tail", INVALID, _refused_tail("tf_saliency_frames", lambda r: (3, r.out.ctypes.data))),
    "tf_saliency_frames_f32, H = 0": ("frames-tail", INVALID, _refused_tail("tf_saliency_frames_f32", lambda r: (3, r.out.ctypes.data))),
    "tf_otsu_masks, H = 0": ("frames-tail", INVALID, _refused_tail("tf_otsu_masks", lambda r: (20, r.out.ctypes.data, None))),
    "tf_segmentor_input, H = 0": ("frames-tail", INVALID, _refused_tail("tf_segmentor_input", lambda r: (8, 8, r.out.ctypes.data, r.out.ctypes.data, None))),
    "tf_echo_frames, solved": ("frames-tail", OK, lambda r: (r.L.tf_echo_frames(r.h, None, r.N, r.H, r.W, r.out.ctypes.data), None)),
    # everything else
    "holds and settings, refused": ("other", INVALID, _other_refused),
    "holds and settings, done": ("other", OK, _other_solved),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_a_call_spends_its_family_s_flags_and_no_other(rig, name):
    family, code, call = CALLS[name]
    assert rig.armed() == set()
    rig.arm()
    rc, text = call(rig)
    msg = rig.err()
    left = rig.armed()
    print(f"{name}: code {rc}, still armed {sorted(left)}, message {msg!r}")
    assert rc == code, (rc, msg)
    assert text is None or text in msg, msg
    assert left == ALL - SPENDS[family], (family, sorted(left))
    assert rig.armed() == set()                               # the probes leave nothing armed


def test_the_probes_tell_each_flag_alone(rig):
    """each probe answers for its own flag whatever the other two are"""
    for flags in ([], ["chain"], ["hold"], ["frames"], ["chain", "hold"], ["chain", "frames"], ["hold", "frames"]):
        rig.arm(flags)
        assert rig.armed() == set(flags), flags


def test_lock_step_refuses_frames_first_then_hold_and_solves_armed_with_chain(rig):
    for flags, text in ((ALL, "tf_frames_next was armed: chains in lock-step take their frames from the caller's pointers (the flag is spent)"),
                        ({"chain", "hold"}, "tf_hold_next was armed: chains in lock-step hold nothing (the flag is spent; a study call holds a study)")):
        for name in ("tf_calc_chains", "tf_calc_chains_device", "tf_calc_chains_rgb"):
            rig.arm(flags)
            assert _chains(rig, name) == UNSUPPORTED and rig.err() == text, (name, rig.err())
            assert rig.armed() == set(), name
    # a lock-step call is chained anyway: an armed tf_chain_next changes nothing, and is spent by the call that is solved
    want = np.zeros_like(rig.flow)
    assert rig.L.tf_calc_chains(rig.h, _ptrs(rig.gray), (C.c_int * 1)(rig.N), 1, rig.H, rig.W, 1.0, _ptrs(want), C.byref(rig.st)) == OK, rig.err()
    for name in ("tf_calc_chains", "tf_calc_chains_rgb"):
        rig.flow[:] = 0
        rig.arm({"chain"})
        assert _chains(rig, name) == OK, (name, rig.err())
        assert rig.armed() == set(), name
        if name == "tf_calc_chains":
            assert np.array_equal(rig.flow, want) and want.any()
    rig.arm({"chain"})
    assert _seq_solved(rig)[0] == OK and np.array_equal(rig.flow, want), "one chain in lock-step is not the chained sequence call"


def test_a_refused_tf_chain_next_leaves_the_chain_disarmed(rig):
    key = _lib.PARAM_KEYS["use_initial_flow"]
    rig.arm()
    try:
        assert rig.L.tf_set_param(rig.h, key, 0.0) == OK                 # (spends nothing)
        assert rig.L.tf_chain_next(rig.h, 1) == UNSUPPORTED and "useInitialFlow is clear" in rig.err()
        assert rig.armed() == {"hold", "frames"}
    finally:
        assert rig.L.tf_set_param(rig.h, key, 1.0) == OK
    rig.arm()
    assert rig.L.tf_chain_next(rig.h, 0) == rig.L.tf_hold_next(rig.h, 0) == OK   # disarmed by hand; tf_frames_next has no such form
    assert rig.armed() == {"frames"}
