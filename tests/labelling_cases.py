"""Frames made to break a tiled connected-component labeller (the device's tile is 64 x 16), shared by the GPU tests of
tf_av_centroids (tests/test_gpu_study_stats.py) and of the labelling scratch that it shares with the masks (tests/test_gpu_masks.py):
the fixed stress_frames(), and the seeded families of adversarial() that tools/fuzz_labelling.py draws its cases from.
A helper module: nothing here is collected."""
import importlib.util
import os

import numpy as np
from scipy import ndimage

S8 = np.ones((3, 3), bool)


def load_fuzzer():
    """tools/fuzz_labelling.py as a module: its scipy references (ref_clean, ref_otsu, ref_centroid, ...) and its draw"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_labelling.py")
    spec = importlib.util.spec_from_file_location("fuzz_labelling", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def corner_diagonals():
    """bool [48, 192]: at each of the four inner tile corners two pixels that meet only diagonally across it, in both orientations:
    four components 8-connected, eight 4-connected (stress_frames()'s tile_corners keeps 2 x 2 blocks there, which both rules join)"""
    m = np.zeros((48, 192), bool)
    for ty in (1, 2):
        for tx in (1, 2):
            if (ty + tx) % 2:
                m[16 * ty - 1, 64 * tx - 1] = m[16 * ty, 64 * tx] = True
            else:
                m[16 * ty - 1, 64 * tx] = m[16 * ty, 64 * tx - 1] = True
    return m


FAMILIES = ("noise", "percolation", "maze", "maze_inv", "rings", "blocks", "lattice", "twins", "nested")


def _maze(rng, H, W):
    """a random spanning tree of the odd lattice (cells at odd rows and columns; at even ones where a side is shorter than 3), one pixel
    wide: one 4-connected component.  The tree is the minimum spanning tree of the lattice under random edge weights."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    oy, ox = (1 if H >= 3 else 0), (1 if W >= 3 else 0)
    ny, nx = (H - oy + 1) // 2, (W - ox + 1) // 2
    if oy and 2 * (ny - 1) + oy > H - 2:
        ny -= 1                                                               # the last row stays wall
    if ox and 2 * (nx - 1) + ox > W - 2:
        nx -= 1
    m = np.zeros((H, W), bool)
    idx = np.arange(ny * nx).reshape(ny, nx)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    m[oy:oy + 2 * ny:2, ox:ox + 2 * nx:2] = True
    if len(a):
        t = minimum_spanning_tree(coo_matrix((rng.random(len(a)) + 0.01, (a, b)), shape=(ny * nx, ny * nx))).tocoo()
        ya, xa = np.divmod(t.row, nx)
        yb, xb = np.divmod(t.col, nx)
        m[oy + ya + yb, ox + xa + xb] = True                                  # the pixel between two joined cells
    return m


def _rings(rng, H, W):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for _ in range(int(rng.integers(1, 8))):
        cy, cx = rng.uniform(-0.3 * H, 1.3 * H), rng.uniform(-0.3 * W, 1.3 * W)
        r, t = rng.uniform(1.0, max(H, W, 4) / 2.0), rng.uniform(0.8, 3.0)
        m |= np.abs(np.hypot(yy - cy, xx - cx) - r) < t / 2.0
    return m


def _lattice(rng, H, W):
    """lines with random breaks on the rows and columns beside the 64 x 16 tile edges, a gap line next to some of them, and pixel pairs
    that meet only diagonally across a tile corner; where the frame holds no tile edge, sparse noise"""
    m = rng.random((H, W)) < 0.04
    for r in (15, 16, 31, 32):
        if r < H and rng.random() < 0.8:
            m[r] = rng.random(W) < 0.9
            if rng.random() < 0.5 and r + 1 < H:
                m[r + 1 if r % 2 else r - 1] = False                          # the row across the edge: a gap
    for c in (63, 64, 127, 128):
        if c < W and rng.random() < 0.8:
            m[:, c] = rng.random(H) < 0.9
            if rng.random() < 0.5 and c + 1 < W:
                m[:, c + 1 if c % 2 else c - 1] = False
    for y in range(16, H, 16):
        for x in range(64, W, 64):
            if rng.random() < 0.6:
                m[y - 2:y + 2, x - 2:x + 2] = False
                if rng.random() < 0.5:
                    m[y - 1, x - 1] = m[y, x] = True
                else:
                    m[y - 1, x] = m[y, x - 1] = True
    return m


def twins(rng, H, W, down_left=False):
    """One random 8-connected blob stamped twice, the copies apart under 8-connectivity (checked with scipy, redrawn otherwise), plus
    debris of smaller area away from both: the largest area is tied.  `down_left`: the second copy lies lower and further left, so the
    copy whose first pixel comes later in raster order has the smaller column centroid.  Needs a side of at least 3."""
    if max(H, W) < 3:
        raise ValueError("twins needs a side of at least 3 pixels")
    if down_left and min(H, W) < 3:
        raise ValueError("twins(down_left) needs both sides of at least 3 pixels")
    for _ in range(200):
        along_x = W >= 3 and (H < 3 or rng.random() < 0.7) if not down_left else bool(rng.random() < 0.5)
        bh = int(rng.integers(1, (H if along_x and not down_left else (H - 1) // 2) + 1))
        bw = int(rng.integers(1, ((W - 1) // 2 if along_x or down_left else W) + 1))
        blob = rng.random((bh, bw)) < rng.uniform(0.45, 0.95)
        lab, n = ndimage.label(blob, structure=S8)
        if n == 0:
            continue
        blob = lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:]))
        ys, xs = np.nonzero(blob)
        blob = blob[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
        bh, bw = blob.shape
        if down_left:
            if H - bh < 1 or W - bw < 1:
                continue
            dy, dx = int(rng.integers(1, H - bh + 1)), -int(rng.integers(1, W - bw + 1))
        elif along_x:
            if W - bw < bw + 1:
                continue
            dy, dx = int(rng.integers(-(H - bh), H - bh + 1)), int(rng.integers(bw + 1, W - bw + 1))
        else:
            if H - bh < bh + 1:
                continue
            dy, dx = int(rng.integers(bh + 1, H - bh + 1)), int(rng.integers(-(W - bw), W - bw + 1))
        y0 = int(rng.integers(max(0, -dy), H - bh - max(0, dy) + 1))
        x0 = int(rng.integers(max(0, -dx), W - bw - max(0, dx) + 1))
        m = np.zeros((H, W), bool)
        m[y0:y0 + bh, x0:x0 + bw] |= blob
        m[y0 + dy:y0 + dy + bh, x0 + dx:x0 + dx + bw] |= blob
        lab, n = ndimage.label(m, structure=S8)
        area = int(blob.sum())
        if n != 2 or not np.array_equal(np.bincount(lab.ravel())[1:], [area, area]):
            continue
        debris = (rng.random((H, W)) < 0.03) & ~ndimage.binary_dilation(m, structure=S8)
        lab, n = ndimage.label(debris, structure=S8)
        big = np.bincount(lab.ravel(), minlength=n + 1) >= area
        big[0] = False
        return m | (debris & ~big[lab])
    raise ValueError(f"no twins found in {H} x {W}")


def _nested(rng, H, W):
    """concentric rectangles alternating foreground and background, random thickness, optionally with a one-pixel breach through one
    foreground ring on its top or left side (to the border, where that ring is the outermost)"""
    m = np.zeros((H, W), bool)
    o = int(rng.integers(0, 3))
    rings = []
    fg = True
    while H - 2 * o > 0 and W - 2 * o > 0:
        t = int(rng.integers(1, 5))
        if fg:
            m[o:H - o, o:W - o] = True
            rings.append((o, t))
        else:
            m[o:H - o, o:W - o] = False
        o += t
        fg = not fg
    if rings and rng.random() < 0.5:
        o, t = rings[int(rng.integers(0, min(2, len(rings))))]
        if rng.random() < 0.5:
            m[o:min(o + t, H - o), int(rng.integers(o, W - o))] = False
        else:
            m[int(rng.integers(o, H - o)), o:min(o + t, W - o)] = False
    return m


def adversarial(rng, H, W, family):
    """bool [H, W] of one of FAMILIES, drawn from rng"""
    if family == "noise":
        return rng.random((H, W)) < rng.uniform(0.05, 0.95)
    if family == "percolation":                          # the site-percolation thresholds of 4- and 8-connectivity
        return rng.random((H, W)) < (0.593 if rng.random() < 0.5 else 0.407)
    if family == "maze":
        return _maze(rng, H, W)
    if family == "maze_inv":                             # the walls; some passages walled up: sealed one-pixel holes and corridors
        m = _maze(rng, H, W)
        return ~(m & (rng.random((H, W)) >= rng.choice([0.0, 0.05, 0.3])))
    if family == "rings":
        return _rings(rng, H, W)
    if family == "blocks":
        b = rng.random(((H + 7) // 8, (W + 7) // 8)) < 0.5
        return np.repeat(np.repeat(b, 8, axis=0), 8, axis=1)[:H, :W] ^ (rng.random((H, W)) < 0.03)
    if family == "lattice":
        return _lattice(rng, H, W)
    if family == "twins":
        return twins(rng, H, W)
    if family == "nested":
        return _nested(rng, H, W)
    raise ValueError(f"unknown family {family!r}")
