"""Frames made to break a tiled connected-component labeller (the device's tile is 64 x 16), shared by the GPU tests of
tf_av_centroids (tests/test_gpu_study_stats.py) and of the labelling scratch that it shares with the masks (tests/test_gpu_masks.py).
A helper module: nothing here is collected."""
import numpy as np


def stress_frames():
    """name -> bool [H, W]; the frames and their order are those the centroid stress test has always walked"""
    out = {}
    out["full"] = np.ones((40, 130), bool)                                      # full-frame foreground
    one = np.zeros((37, 70), bool); one[20, 66] = True; out["single_pixel"] = one   # a single pixel in a ragged tile
    yy, xx = np.mgrid[:50, :140]
    out["checkerboard"] = (yy + xx) % 2 == 0                                   # checkerboard: one component
    snake = np.zeros((61, 200), bool)                                         # a one-pixel-wide snake through many tiles
    for r in range(0, 61, 4):
        snake[r, 1:199] = True
        snake[r:r + 4, 198 if (r // 4) % 2 == 0 else 1] = True
    snake[60:, :] = False
    snake[59, :] = False
    out["snake"] = snake
    stair = np.zeros((70, 200), bool)                                         # diagonal staircases across tile corners
    for k in range(70):
        stair[k, 64 - 16 + k] = True
        stair[69 - k, 150 - k] = True
    out["staircase"] = stair
    anti = np.zeros((48, 192), bool)                                          # pixels that meet only at tile corners
    for ty in range(1, 3):
        for tx in range(1, 3):
            anti[16 * ty - 1, 64 * tx - 1] = anti[16 * ty, 64 * tx] = True
            anti[16 * ty - 1, 64 * tx] = anti[16 * ty, 64 * tx - 1] = True
    anti[15, 63] = anti[16, 64] = anti[16, 63] = False
    out["tile_corners"] = anti
    rng = np.random.default_rng(3)
    for H, W in ((1, 300), (300, 1), (1, 1), (17, 65), (129, 63), (100, 257)):
        out[f"random_{H}x{W}"] = rng.random((H, W)) < 0.45
    out["empty"] = np.zeros((20, 20), bool)
    return out
