"""Held frames (tf_hold_frames, DenseFlow.hold_frames, frames.ingest_host): the inputs the CPU and the GPU tests share, and a numpy
stand-in for the engine's frame protocol.  A helper module of tests/test_frames_cpu.py, tests/test_gpu_held_frames.py and the walk's
frame tests: nothing here is collected."""
import numpy as np

from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.dense_flow import HeldFrames
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

FORMS = ("RGB", "GRAY", "YBR_FULL")
# (N, H, W) and what each exercises in k_ingest (a lane takes 4 pixels of the flat N * H * W)
SHAPES = [
    (1, 1, 1),       # the smallest frame: one short run, bytes only
    (2, 1, 3),       # a few pixels, more than one frame: one full run and a tail of 2
    (3, 2, 5),       # a width that is no multiple of 4: runs cross row ends
    (2, 3, 7),       # rows whose 3 * W byte offset is not dword-aligned
    (5, 7, 13),      # frame offsets that are odd
    (3, 37, 53),     # a flip of an odd width, more than one block
    (2, 40, 64),     # the aligned fast path
]


def cube():
    """All 2^24 (Y, Cb, Cr) triples as a study, uint8 [64, 512, 512, 3]"""
    v = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(64, 512, 512, 3))


def source(form, N, H, W, seed=0):
    """Frames as a file stores them in `form`: uniform random bytes (every clamp and rounding case of the YBR conversion turns up in a
    few thousand pixels; the cube has them all)"""
    rng = np.random.default_rng(1000 * seed + 100 * N + 10 * H + W + FORMS.index(form))
    return rng.integers(0, 256, (N, H, W) if form == "GRAY" else (N, H, W, 3), dtype=np.uint8)


def speckle_source(form, N, H, W, seed=0):
    """A moving speckle study (something the solvers can follow) stored in `form`: the grey frames themselves, or as RGB / YBR triples
    whose conversion is not grey (so that the three channels differ)"""
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(seed + N * 1000 + H + W, N, H, W)
    if form == "GRAY":
        return np.ascontiguousarray(g)
    rng = np.random.default_rng(seed + 7)
    tint = rng.integers(96, 160, (1, H, W, 2), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([g[..., None], np.broadcast_to(tint, (N, H, W, 2))], axis=3))


class NumpyFrames:
    """The engine's held-frames protocol in numpy: hold_frames / download_frames / release_frames with DenseFlow's token rules, and
    `resolve`, which gives a frames argument's RGB array the way the library's armed call reads it.  `uploads` counts the frame bytes
    that would cross the bus."""

    def __init__(self):
        self.rgb, self.generation, self.uploads, self.held_reads = None, 0, 0, 0

    def _shape(self):
        return (0, 0, 0, self.generation) if self.rgb is None else self.rgb.shape[:3] + (self.generation,)

    def hold_frames(self, arr, form="RGB", flip=False):
        if form not in FORMS:
            raise OpticalFlowCalculationError(f"form must be one of {FORMS}, got {form!r}")
        self.rgb = F.ingest_host(arr, form, flip)
        self.uploads += np.asarray(arr).nbytes
        self.generation += 1
        N, H, W = self.rgb.shape[:3]
        return HeldFrames(self, N, H, W, self.generation)

    def download_frames(self):
        if self.rgb is None:
            raise OpticalFlowCalculationError("no frames are held (hold_frames)")
        return self.rgb.copy()

    def release_frames(self):
        if self.rgb is not None:
            self.generation += 1
        self.rgb = None

    def resolve(self, frames, min_frames=1):
        """an array as it is (counted as an upload), or the held frames a token names"""
        if not isinstance(frames, HeldFrames):
            frames = np.asarray(frames)
            self.uploads += frames.nbytes
            return frames
        t = frames.checked(self, self._shape(), min_frames)
        self.held_reads += 1
        return self.rgb[t.first:t.first + t.count]


# ---- the GPU cases that need torch in the process (tests/test_gpu_held_frames.py runs `python -m tests.frames_cases` once): torch is
# imported before the first engine is made, so that both share one HIP runtime -----------------------------------------------------------
TORCH_CASES = ["segmentor_input_chunks", "caller_stream"]


def _case_segmentor_input_chunks(T, torch):
    """predict_movie's device glue in chunks through token[a:b], a last short chunk included: bit-equal to the same chunks of the
    twin's host RGB, nothing uploaded; new frames held right behind a call wait for its kernel"""
    e = T.DenseFlow(device_id=0, max_batch=3)
    try:
        src = speckle_source("YBR_FULL", 7, 37, 53)
        rgb = F.ingest_host(src, "YBR_FULL", True)
        tok = e.hold_frames(src, "YBR_FULL", True)
        up = e.counter("frames_upload_bytes")
        for a in range(0, 7, 3):
            got = e.segmentor_input(tok[a:a + 3], out_size=(64, 80))
            assert e.counter("frames_upload_bytes") == up
            want = e.segmentor_input(rgb[a:a + 3], out_size=(64, 80))
            up = e.counter("frames_upload_bytes")
            assert got.shape == want.shape == (min(3, 7 - a), 3, 64, 80) and torch.equal(got, want), a
        got = e.segmentor_input(tok, out_size=(33, 47))                  # (the element-store form of the kernel)
        e.hold_frames(np.zeros_like(rgb), "RGB")                         # replaces the frames the queued kernel reads: waits for it
        assert torch.equal(got, e.segmentor_input(rgb, out_size=(33, 47)))
        try:
            e.segmentor_input(tok[0:2])
            raise AssertionError("a stale token was accepted")
        except OpticalFlowCalculationError as err:
            assert "stale" in str(err)
    finally:
        e.close()


def _case_caller_stream(T, torch):
    """the held buffers follow the handle's stream, a caller's included (tf_set_stream)"""
    e = T.DenseFlow(device_id=0, max_batch=3)
    try:
        src = speckle_source("YBR_FULL", 6, 37, 53)
        rgb = F.ingest_host(src, "YBR_FULL", True)
        want = e.calc_study_payload(rgb, 2.0), e.otsu_masks(rgb, 20), e.echo_frames(rgb)
        side = torch.cuda.Stream(0)
        e.set_stream(int(side.cuda_stream), external=True)
        tok = e.hold_frames(src, "YBR_FULL", True)
        assert np.array_equal(e.download_frames(), rgb)
        got = e.calc_study_payload(tok, 2.0), e.otsu_masks(tok, 20), e.echo_frames(tok[0:6])
        e.set_stream(0, external=False)
        back = e.calc_study_payload(tok, 2.0), e.otsu_masks(tok, 20), e.echo_frames(tok)     # held on the caller's stream, read on the handle's own
        for g in (got, back):
            assert np.array_equal(g[0][0], want[0][0]) and np.array_equal(g[0][1], want[0][1])
            assert np.array_equal(g[1], want[1]) and np.array_equal(g[2], want[2])
        e.release_frames()
    finally:
        e.close()


if __name__ == "__main__":
    import json
    import time
    import torch                                                         # before the library: one HIP runtime for both
    import tee_optical_flow_amd as T
    results = {}
    for name in TORCH_CASES:
        t0 = time.time()
        try:
            globals()["_case_" + name](T, torch)
            outcome = "ok"
        except Exception as err:                                         # the parent test shows it
            import traceback
            outcome = traceback.format_exc()[-1500:] or repr(err)
        results[name] = (round(time.time() - t0, 2), outcome)
    print(json.dumps(results))
