"""Shared by tests/test_single_overlay_cpu.py and tests/test_gpu_single_overlay.py: the magnitude overlay's cases.  Every case is a few
small frames: (name, FlowStudy with an 'rv' mask, param, keywords of analysis.magnitude_overlay, chunk KiB or 0).  The frame rate's type
chooses the gradient's rule under numpy >= 2 (np.float64: float64 division; a Python float: float32), norm_f64 the norm's.  A helper
module: nothing here is collected."""
import os

import numpy as np

from tee_optical_flow_amd import analysis as A

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_single_overlay.npz")
# (case in the fixture): <study>/<param>
FIXTURE_CASES = ["main/velocity", "main/acceleration", "main/PWR", "u8/velocity", "emptymask/velocity", "zeroecho/velocity", "full/velocity",
                 "c1/velocity"]


def load_fixture():
    with np.load(FIX) as f:
        return {k: f[k] for k in f.files}


def fixture_study(z, name):
    # float(frame_rate): the fixture's numpy divided the gradient in float32 (see the generator's docstring)
    return A.FlowStudy(z[f"{name}/flow"], {"rv": z[f"{name}/rv"]}, float(z["frame_rate"]), nframes=int(z["nframes"]), echo=z[f"{name}/echo"],
                       filename=str(z[f"{name}/filename"]))


def hot():
    return A.magnitude_colormap_lut("hot")


def _study(seed, N, n, H, W, C=2, flow_dtype=np.float16, echo_dtype=np.float16, full=False, frame_rate=30.0):
    """speckle flow, an rv mask of drifting discs (or full), an echo of non-round grey levels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    amp = rng.uniform(0.5, 6, N)[:, None, None, None]
    flow = (rng.normal(0, 1, (N, H, W, 2)) * amp).astype(flow_dtype)
    rv = np.ones((N, H, W), bool)
    if not full:
        for f in range(N):
            rv[f] = ((yy - H / 2 - f / 4) / (0.35 * H + 1)) ** 2 + ((xx - W / 2 + f / 4) / (0.4 * W + 1)) ** 2 < 1
    else:
        flow[np.abs(flow.astype(np.float32)).sum(-1) < 0.5] = 0.75      # no zero vector: vmin > 0
    echo = rng.integers(0, 251, (N, H, W))
    echo = (echo * rng.choice([1.0, 0.37, 200.0])).astype(np.float16) if echo_dtype == np.float16 else echo.astype(np.uint8)
    rv = np.stack([rv] * C, -1)
    return A.FlowStudy(flow, {"rv": rv}, frame_rate, nframes=n, echo=echo)


def every_index_field():
    """one 8 x 33 velocity frame (float16 flow, full mask) whose magnitudes are (k + 0.5) / 4 for k = 0..255, 64 (the maximum: t == 1)
    and 0 (the minimum): t * 256 = k + 0.5 exactly, so every row 0..255 is used, and t == 1 lands on row 255"""
    x = np.concatenate([(np.arange(256) + 0.5) / 4, [64.0], np.zeros(7)])
    flow = np.zeros((1, 8, 33, 2), np.float16)
    flow[0, ..., 0] = x.reshape(8, 33)
    assert np.array_equal(flow[0, ..., 0].astype(np.float64).ravel(), x)
    return flow, x.reshape(8, 33).astype(np.float32)


def tie_case():
    """(study, table, ties): every_index_field under a table whose entries put v = (0.5 * (entry / 1)) * 255 exactly on float16
    midpoints, with an all-zero echo (its term is 0): channel 0 just below an integer (the tie goes up to the integer, which is the
    even neighbour: the byte shows it), channel 1 just above an integer (the tie goes down to it), channel 2 the same in the next
    binade down.  Row 255 is white, so the colour maximum is 1.  `ties` counts the entries of rows 0..254 whose v is the midpoint
    exactly, in the twin's own arithmetic."""
    flow, _ = every_index_field()
    lut = np.ones((256, 3), np.float64)
    mid = np.empty((255, 3), np.float64)
    j = np.arange(255)
    mid[:, 0] = 65 + j % 60 - 2.0 ** -5                                # [64, 128): float16 values are 2^-4 apart
    mid[:, 1] = 65 + j % 60 + 2.0 ** -5
    mid[:, 2] = 33 + j % 30 - 2.0 ** -6                                # [32, 64): 2^-5 apart
    lut[:255] = 2 * (mid / 255)
    v = (0.5 * (lut[:255] / 1.0)) * 255
    ties = int((v == mid).sum())
    st = A.FlowStudy(flow, {"rv": np.ones((1, 8, 33, 1), bool)}, 30.0, nframes=1, echo=np.zeros((1, 8, 33), np.float16))
    return st, lut, ties, mid, v


def cases():
    out = []
    z = load_fixture()
    for c in FIXTURE_CASES:
        name, param = c.split("/")
        out.append((f"fixture-{name}-{param}", fixture_study(z, name), param, dict(norm_f64=False), 0))
    for param in A.PARAMS:
        out.append((f"37x53-{param}", _study(1, 5, 3, 37, 53), param, {}, 0))
        out.append((f"1x5-{param}", _study(2, 3, 2, 1, 5), param, {}, 0))     # H * W * 3 is no multiple of 4
    out.append(("n1", _study(3, 3, 1, 19, 23), "acceleration", {}, 0))
    out.append(("N-equals-n", _study(4, 4, 4, 19, 23), "PWR", {}, 0))
    out.append(("N1", _study(5, 1, 1, 9, 7), "velocity", {}, 0))
    out.append(("chunk-of-one-frame", _study(6, 5, 4, 37, 53), "velocity", {}, 1))
    out.append(("chunk-of-one-frame-u8", _study(6, 5, 4, 37, 53, echo_dtype=np.uint8), "PWR", {}, 1))
    out.append(("chunks-of-two", _study(6, 7, 5, 37, 53), "acceleration", {}, 20))      # 5 B a pixel: 9.6 KiB a frame
    out.append(("C1", _study(7, 4, 2, 21, 30, C=1), "velocity", {}, 0))
    out.append(("C2", _study(7, 4, 2, 21, 30, C=2), "velocity", {}, 0))
    out.append(("f32-flow", _study(8, 4, 3, 21, 30, flow_dtype=np.float32), "PWR", {}, 0))
    out.append(("f32-flow-u8", _study(8, 4, 3, 21, 30, flow_dtype=np.float32, echo_dtype=np.uint8), "acceleration", {}, 0))
    out.append(("u8-echo", _study(9, 4, 3, 21, 30, echo_dtype=np.uint8), "velocity", {}, 0))
    for g64 in (False, True):
        for n64 in (False, True):
            st = _study(10, 5, 3, 29, 41, full=True, frame_rate=np.float64(29.97) if g64 else 29.97)
            out.append((f"full-grad{'64' if g64 else '32'}-norm{'64' if n64 else '32'}", st, "acceleration", dict(norm_f64=n64), 0))
            out.append((f"full-velocity-grad{'64' if g64 else '32'}-norm{'64' if n64 else '32'}", st, "velocity", dict(norm_f64=n64), 0))
    const = _study(11, 3, 2, 13, 17, full=True)
    const.flow[:] = np.array([1.5, 2.0], np.float16)
    out.append(("constant-magnitude", const, "velocity", {}, 0))
    flow, _ = every_index_field()
    rng = np.random.default_rng(12)
    out.append(("every-index", A.FlowStudy(flow, {"rv": np.ones((1, 8, 33, 2), bool)}, 30.0, nframes=1,
                                           echo=rng.integers(0, 251, (1, 8, 33)).astype(np.float16)), "velocity", {}, 0))
    st, lut, _, _, _ = tie_case()
    out.append(("ties", st, "velocity", dict(colormap=lut), 0))
    black = _study(13, 4, 3, 21, 30)
    black.masks["rv"][1] = False                                       # frame 1 uses row 0 alone, and row 0 is black: its colour maximum is 0
    lut = rng.uniform(0, 1, (256, 3))
    lut[0] = 0
    out.append(("black-row", black, "velocity", dict(colormap=lut), 0))
    sub = _study(14, 4, 3, 21, 30)
    sub.echo = rng.choice(np.array([0, 6e-8, 1.2e-7, 3e-5], np.float16), (4, 21, 30))   # frame 0: subnormals alone
    sub.echo[1, 3, 4] = 65504
    sub.echo[2] = 65504
    sub.echo[2, :5] = rng.choice(np.array([0, 6e-8, 1, 40000], np.float16), (5, 30))
    out.append(("echo-subnormal-and-65504", sub, "PWR", {}, 0))
    return out


class Recorder:
    """writer_factory and writer in one: records the path, fps, the frames and the order of the calls"""

    def __init__(self):
        self.path, self.fps, self.frames, self.events, self.closed = None, None, [], [], False

    def __call__(self, path, fps=None):
        self.path, self.fps = path, fps
        return self

    def append_data(self, frame):
        assert not self.closed
        self.frames.append(np.array(frame))
        self.events.append("append")

    def close(self):
        self.closed = True
        self.events.append("close")
