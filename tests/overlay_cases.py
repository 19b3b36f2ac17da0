"""Shared by tests/test_overlay_cpu.py and tests/test_gpu_overlay.py: the fixture's cases, a recording video writer, and the seeded
generator of random overlay studies."""
import os

import numpy as np

from tee_optical_flow_amd import analysis as A

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_overlay.npz")
# (case in the fixture, keywords of radlong_overlay): "vm" is the main study through VisualizationManager's colormaps
CASES = [("main/velocity", {}), ("main/acceleration", {}), ("main/PWR", {}), ("u8/velocity", {}), ("empty0/velocity", {}),
         ("vm/velocity", dict(colormap_rad="BrBG", colormap_long="PiYG"))]
COLORMAPS = ("bwr", "BrBG", "PiYG", "viridis")                 # the committed tables


def fixture_study(z, name):
    src = "main" if name == "vm" else name
    # float(frame_rate): the fixture's numpy divided the gradient in float32 (see the generator's docstring)
    return A.FlowStudy(z[f"{src}/flow"], {"rv": z[f"{src}/rv"], "av": z[f"{src}/av"]}, float(z["frame_rate"]), nframes=int(z["nframes"]),
                       echo=z[f"{src}/echo"], filename=str(z[f"{src}/filename"]))


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


def random_case(seed, max_hw=(200, 300)):
    """(FlowStudy, param, colormap keywords, centroids) for one seeded case: sizes from 1 x 1 to max_hw, 1 to 6 frames used, an rv mask
    of a density between empty and full, a flow family (speckle, quantised, a quiet first frame under loud later ones, huge values, an
    all-zero first frame, constant), a float16 or uint8 echo and a pair of the committed colormaps."""
    rng = np.random.default_rng(seed)
    H = int(rng.integers(1, max_hw[0] + 1))
    W = int(rng.integers(1, max_hw[1] + 1))
    if seed % 10 == 0:
        H, W = 1, 1
    if seed % 10 == 1:
        H, W = max_hw
    n = int(rng.integers(1, 7))
    N = n + int(rng.integers(1, 3))                                # the gradient needs a frame after the last one used, or not
    family = int(rng.integers(0, 6))
    flow = rng.normal(0, 3, (N, H, W, 2))
    if family == 1:
        flow = np.round(flow * 2) / 2
    elif family == 2:
        flow *= np.concatenate([[0.05], rng.uniform(1, 8, N - 1)])[:, None, None, None]
    elif family == 3:
        flow *= 2000                                               # near the float16 range: PWR reaches 1e10
    elif family == 4:
        flow[0] = 0
    elif family == 5:
        flow[:] = 1.5
    flow = flow.astype(np.float16 if rng.random() < 0.7 else np.float32)
    density = [0.0, 0.05, 0.5, 0.95, 1.0][int(rng.integers(0, 5))]
    rv = rng.random((N, H, W)) < density
    if density == 0.0:
        rv[n - 1, H // 2, W // 2] = True                           # one pixel, in the last frame only
    rv = np.stack([rv, rv], -1) if rng.random() < 0.5 else rv[..., None]
    if rng.random() < 0.5:
        echo = rng.integers(0, 256, (N, H, W)).astype(np.uint8)
        echo[0, 0, 0] = max(echo[0, 0, 0], 1)
    else:
        kind = int(rng.integers(0, 3))
        if kind == 0:
            echo = rng.integers(0, 256, (N, H, W)).astype(np.float16)
            echo[0, 0, 0] = 255
        elif kind == 1:
            echo = rng.uniform(0, 1, (N, H, W)).astype(np.float16)
            echo[0, 0, 0] = 1
        else:
            echo = rng.integers(0, 2, (N, H, W)).astype(np.float16)   # quotients and their halves are float16 subnormals
            echo[0, 0, 0] = 60000
    cent = [(float(rng.uniform(-2, H + 2)), float(rng.uniform(-2, W + 2))) for _ in range(n)]
    if rng.random() < 0.3:
        cent[0] = (float(H // 2), float(W // 2))                   # a centroid on a pixel: the 0/0 of the unit vector
    a, b = rng.integers(0, 4, 2)
    st = A.FlowStudy(flow, {"rv": rv, "av": rv}, float(rng.uniform(20, 60)), nframes=n, echo=echo)
    return st, A.PARAMS[int(rng.integers(0, 3))], dict(colormap_rad=COLORMAPS[a], colormap_long=COLORMAPS[b]), cent
