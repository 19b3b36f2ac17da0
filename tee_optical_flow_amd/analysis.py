"""radial / longitudinal projection of the flow and the per-frame percentile / histogram curves.

Mirrors /root/reference/optical_flow/analysis.py:
  :122-134  calc_proj_mag,  :137-163 calculate_comp_magnitude (with radial_vecgrid :89-119)   -> calculate_comp_magnitude
  :166-212  calc_bidirectional_hist                                                          -> calc_bidirectional_hist
Two implementations with identical results: a vectorised numpy one (host) and a device one that keeps the projections in
HBM and gets the histogram and the exact order statistics np.percentile interpolates between from HIP kernels
(include/teeflow.h: tf_radlong_project / _hist / _select, as DenseFlow.radlong_project / radlong_hist / radlong_select: every device
call here is a method of the engine).  Pinned by tests/golden/reference_analysis.npz, which the reference's own functions produced.

The steps before the projection are here too, so that the consumer's call runs whole (/root/reference/optical_flow/analyze_optical_flow.py):
  :202-244  calc_AV_centroid (8-connected labelling, largest region, Savitzky-Golay)                  -> av_centroids
  :320-343  calculate_3dhist_radlong(ds, param) with OpticalFlowDataset's param field
            (optical_flow_dataset.py:57, 100-101, 182-228: velocity, np.gradient acceleration, PWR, x rv mask) -> calculate_3dhist_radlong
With engine= the labelling (tf_av_centroids) and the param field fused into the projection (tf_radlong_project_param) run on the device;
without, a numpy/scipy twin gives the same bits.  Pinned by tests/golden/reference_study_stats.npz (the reference's own functions on a
study file opened by its own OpticalFlowDataset).

And the polar steps of the same consumer:
  analyze_optical_flow.py:909-966  calculate_3dhist(ds, param, label)                                 -> calculate_3dhist
  cardiac_cycle_detection.py:100-120  AngleDetector.detect's per-frame mode of np.round(ang, 2)        -> angle_mode_series
both on cv2.cartToPolar, restated here as cart_to_polar (OpenCV 4.x's AVX2 / NEON arithmetic; parity with cv2 unpinned, DESIGN.md
section 2).  With engine= the field, the transform, the angle histogram and mode run fused on the device (tf_polar_project_param) and
the magnitude / angle statistics come from tf_radlong_hist / tf_radlong_select; without, numpy.  Pinned by
tests/golden/reference_polar.npz (the reference's own calculate_3dhist and AngleDetector.detect, with cart_to_polar as cv2).

And the other cardiac-cycle detector's per-frame series:
  cardiac_cycle_detection.py:159-172  AreaDetector.detect's skimage label + regionprops, props[0].area  -> area_series
With engine= the labelling runs on the device (tf_first_region_areas); without, a scipy twin that needs no skimage.  Pinned by
tests/golden/reference_area_series.npz (the area_list the reference's own AreaDetector.detect handed to its smoother).

And the overlay video of the rad/long projections:
  analyze_optical_flow.py:488-560  overlay3, visualize_radlong(ds, param, save_dir)                   -> radlong_overlay, visualize_radlong
  visualization.py:241-297, 1045-1051  VisualizationManager.visualize_radlong (other colormaps)       -> the colormap_rad / colormap_long keywords
With engine= the frames are rendered on the device from the planes tf_radlong_project_param left resident (tf_radlong_overlay), 6 bytes
per pixel downloaded; without, a numpy twin that keeps index planes instead of RGBA float64 arrays.  Pinned by
tests/golden/reference_overlay.npz (the frames the reference's own functions handed to their video writer).

And the reference's other video, the single-component magnitude overlay:
  example_peak_plots.py:459-513  mag of get_masked_arr(param, label) through 'hot', blended with the echo -> magnitude_overlay, visualize_magnitude
With engine= the field, the study-wide norm, the indices, the per-frame maxima and the frames are made on the device
(tf_magnitude_overlay), 3 bytes per pixel downloaded; without, a numpy twin that works frame by frame (magnitude_overlay_host).  Pinned by
tests/golden/reference_single_overlay.npz (the frames the reference's own example handed to its video writer).

A study held on the device (DenseFlow.hold_study, or a study call with hold=True) is analysed through a HeldStudy: the `ds` of the
functions above whose arrays are not on the host.  With it and its own engine they take the held calls (tf_held_*), which read the
flow, the masks and the echo where they are; the results are the bits of the same functions on a FlowStudy of the same arrays.
Where the arrays are is _Tail's business alone; each function's device path is written once, over either kind.

A study file reaches the device as arrays (HeldStudy.from_hdf5, inflate="h5py": h5py inflates every gzip chunk on one thread) or as the
chunks the file stores: study_chunks reads them without inflating them (save_chunks / load_chunks carry the record to an interpreter
without h5py), and HeldStudy.from_chunks has them inflated by zlib in a thread pool (unchunk_host, inflate="host") or uploaded
compressed and inflated on the device (DenseFlow.hold_study_chunks / hold_mask_chunks, inflate="device").  The held bytes are the same.
"""
import logging
import os
from types import SimpleNamespace

import numpy as np

from . import _lib

log = logging.getLogger(__name__)

PARAMS = ("velocity", "acceleration", "PWR")       # OpticalFlowDataset.accepted_params; the index is the ABI's TF_PARAM_* code


# ---- host (numpy) -------------------------------------------------------------------------------------------------------
def calculate_comp_magnitude(OF_arr, centroid_list):
    """(rad_arr, long_arr), float64 [N,H,W].  Reference quirk kept: unitvec[...,0] is the ROW direction and multiplies
    OF[...,0], the x (column) displacement."""
    n = len(centroid_list)
    OF = np.asarray(OF_arr)[:n]
    H, W = OF.shape[1:3]
    c = np.asarray(centroid_list, dtype=np.float64)
    dh = c[:, 0, None, None] - np.arange(H)[None, :, None]
    dw = c[:, 1, None, None] - np.arange(W)[None, None, :]
    dh = np.broadcast_to(dh, (n, H, W))
    dw = np.broadcast_to(dw, (n, H, W))
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = np.sqrt(dh * dh + dw * dw)
        u0 = np.nan_to_num(dh / norm, nan=0)
        u1 = np.nan_to_num(dw / norm, nan=0)
    rad = OF[..., 0] * u0 + OF[..., 1] * u1
    lon = OF[..., 0] * u1 + OF[..., 1] * (-1 * u0)
    return rad, lon


def _finish_hist(n_frames, nbins, mag_min, mag_max, counts, per_frame):
    """The reference's per-frame loop (:188-212) given, for every frame, either None (no non-zero data) or (hi, lo, freq)."""
    hi_l, lo_l, fr_l = [], [], []
    edges = []
    for i in range(n_frames):
        if per_frame[i] is None:
            if hi_l:
                hi_l.append(hi_l[-1]); lo_l.append(lo_l[-1]); fr_l.append(fr_l[-1])
            else:
                hi_l.append(mag_max); lo_l.append(mag_min); fr_l.append(np.ones(nbins))
        else:
            hi, lo, freq = per_frame[i]
            hi_l.append(hi); lo_l.append(lo); fr_l.append(freq + 1)
            edges = np.linspace(mag_min, mag_max, nbins + 1) if mag_min != mag_max else np.linspace(mag_min - 0.5, mag_max + 0.5, nbins + 1)
    return np.stack(fr_l), edges, np.asarray(hi_l), np.asarray(lo_l)


def calc_bidirectional_hist(mag_arr, nframes, perc_lo=1, perc_hi=99, nbins=1000):
    mag_arr = np.asarray(mag_arr)
    mag_max, mag_min = np.max(mag_arr), np.min(mag_arr)
    per = []
    for i in range(nframes):
        flat = np.ravel(mag_arr[i])
        nz = flat[flat != 0]
        if len(nz) == 0:
            per.append(None)
        else:
            freq, _ = np.histogram(nz, bins=nbins, range=(mag_min, mag_max))
            per.append((np.percentile(nz, perc_hi), np.percentile(nz, perc_lo), freq))
    return _finish_hist(nframes, nbins, mag_min, mag_max, None, per)


# ---- device ---------------------------------------------------------------------------------------------------------------
def _lerp(a, b, t):
    """numpy's percentile interpolation (numpy/lib/_function_base_impl.py::_lerp) for scalars, in their own dtype: a + (b - a) * t, or
    b - (b - a) * (1 - t) for t >= 0.5"""
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def percentile_rank64(count, q):
    """(prev, next, frac) of np.percentile(a, q) for `count` float64 values: method 'linear', the virtual index (count - 1) * (q / 100)
    in float64, the next index clipped at count - 1.  The result is _lerp(sorted(a)[prev], sorted(a)[next], frac)."""
    vi = (count - 1) * np.true_divide(q, 100)
    prev = int(np.floor(vi))
    return prev, min(prev + 1, count - 1), vi - prev


def _check_finite_range(mn, mx):
    """np.histogram's refusal of a non-finite range, raised before any device histogram runs.  f64_key orders a positive NaN above
    +inf and a negative NaN below -inf, so the min/max a projection returns are finite exactly when every plane value is."""
    if not (np.isfinite(mn) and np.isfinite(mx)):
        raise ValueError(f"supplied range of [{mn}, {mx}] is not finite")


def _check_bins(edges, nbins):
    """np.histogram's refusal of edges that do not increase (a range too narrow for nbins bins)"""
    if np.any(edges[:-1] >= edges[1:]):
        raise ValueError(f"Too many bins for data range. Cannot create {nbins} finite-sized bins.")


def radlong_stats_device(engine, OF_arr, centroid_list, perc_lo=1, perc_hi=99, nbins=1000, return_arrays=False):
    """{'radial': (freq, edges[:-1], hi, lo), 'longitudinal': (...)} as calculate_3dhist_radlong (:289-327) returns after its
    centroid step, computed on the device behind `engine` (a DenseFlow).  return_arrays adds 'rad_arr' / 'long_arr'.  A NaN or
    inf in a plane raises ValueError, as np.histogram does for the host twin."""
    mm, nz, rad, lon = engine.radlong_project(OF_arr, centroid_list, return_arrays=return_arrays)
    return _radlong_stats_resident(engine, len(centroid_list), mm, nz, perc_lo, perc_hi, nbins, rad, lon)


def _radlong_stats_resident(engine, N, mm, nz, perc_lo, perc_hi, nbins, rad=None, lon=None):
    """The statistics of the projections resident on the device after tf_radlong_project(_param): per frame histogram, the exact
    order statistics np.percentile interpolates between, and the reference's per-frame loop.  mm / nz as the projection returned.
    Raises the ValueError np.histogram raises in the host twin (a non-finite range, or one too narrow for nbins bins) before the
    device histogram of that component runs."""
    nz = np.asarray(nz).reshape(-1)
    out = {}
    for which, name in ((0, "radial"), (1, "longitudinal")):
        mn, mx = mm[2 * which], mm[2 * which + 1]
        cnt = nz[which::2]
        if cnt.any():                                                         # the host calls np.histogram for a non-empty frame only
            _check_finite_range(mn, mx)
        first, last = (mn, mx) if mn != mx else (mn - 0.5, mx + 0.5)          # np.histogram's degenerate-range rule
        edges = np.linspace(first, last, nbins + 1)
        if cnt.any():
            _check_bins(edges, nbins)
        freq = engine.radlong_hist(which, edges, N)
        ranks = np.full((N, 4), -1, np.int64)
        frac = np.zeros((N, 2))
        for i in range(N):
            if cnt[i] > 0:
                for j, q in enumerate((perc_hi, perc_lo)):
                    ranks[i, 2 * j], ranks[i, 2 * j + 1], frac[i, j] = percentile_rank64(cnt[i], q)
        vals = engine.radlong_select(which, ranks)
        per = [None if cnt[i] == 0 else (_lerp(vals[i, 0], vals[i, 1], frac[i, 0]), _lerp(vals[i, 2], vals[i, 3], frac[i, 1]), freq[i])
               for i in range(N)]
        f, e, hi, lo = _finish_hist(N, nbins, mn, mx, cnt, per)
        out[name] = (f, np.asarray(e)[:-1], hi, lo)
    if rad is not None:
        out["rad_arr"], out["long_arr"] = rad, lon
    return out


# ---- the whole consumer call: AV centroids, the param field, then the statistics -------------------------------------------
def _largest_component(frame):
    """(centroid (row, col), area) of the largest 8-connected component of frame != 0 (first label on a tie), or None: skimage's
    label + regionprops + find_correct_centroid.  Sums of integer coordinates in float64 are exact, so sum / area is the float64
    coords.mean(axis=0) of regionprops."""
    from scipy import ndimage
    lab, n = ndimage.label(np.asarray(frame) != 0, structure=np.ones((3, 3), bool))
    if n == 0:
        return None
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    lbl = flat[idx]
    rows, cols = np.divmod(idx, lab.shape[1])
    area = np.bincount(lbl, minlength=n + 1)
    k = 1 + int(np.argmax(area[1:]))
    sr = np.bincount(lbl, weights=rows, minlength=n + 1)
    sc = np.bincount(lbl, weights=cols, minlength=n + 1)
    return (sr[k] / area[k], sc[k] / area[k]), int(area[k])


def av_centroids(mask_arr, nframes, filter=True, savgol_window=10, savgol_poly=4, *, engine=None):
    """calc_AV_centroid (analyze_optical_flow.py:213-244): per frame the centroid (row, col) of the largest 8-connected region of
    mask_arr[i, :, :, 0]; an empty frame copies the previous centroid ((H/2, W/2) on frame 0) with a warning; then, with `filter`,
    scipy.signal.savgol_filter over the frames (an ndarray), unless the list is shorter than the window (logged; the list is
    returned unfiltered).  With `engine` (a DenseFlow) the labelling runs on the device (tf_av_centroids), with the same bits.
    mask_arr may be a HeldStudy (its 'av' mask) or what its get_mask returned: the labelling then reads the held mask."""
    nframes = int(nframes)
    if isinstance(mask_arr, HeldStudy):
        mask_arr = mask_arr.get_mask("av")
    tail = _tail(mask_arr, engine)
    shape = np.shape(mask_arr)                                # (a HeldMask has the shape of the mask it names)
    if len(shape) != 4:
        raise ValueError(f"mask_arr must be [N,H,W,C], got shape {shape}")
    if nframes > shape[0]:
        raise IndexError(f"nframes {nframes} > {shape[0]} mask frames")
    if tail is not None and nframes > 0:
        cent, area = tail.centroids(mask_arr, nframes)
        found = [((float(cent[i, 0]), float(cent[i, 1])), int(area[i])) if area[i] > 0 else None for i in range(nframes)]
    else:
        found = [_largest_component(np.asarray(mask_arr[i, :, :, 0])) for i in range(nframes)]
    centroid_list = []
    for i in range(nframes):
        if found[i] is not None:
            centroid_list.append(found[i][0])
        else:
            centroid_list.append(centroid_list[i - 1] if centroid_list else (shape[1] / 2, shape[2] / 2))
            log.warning("empty AV mask at frame %d: centroid carried over", i)
    if filter:
        if len(centroid_list) < savgol_window:
            log.error("cannot apply the Savitzky-Golay filter: %d centroids, window %d", len(centroid_list), savgol_window)
        else:
            from scipy.signal import savgol_filter
            centroid_list = savgol_filter(centroid_list, savgol_window, savgol_poly, axis=0)
    return centroid_list


def gradient_is_f64(frame_rate):
    """Whether numpy, in this process, divides np.gradient(float32 field, 1 / frame_rate) in float64: NEP 50 (numpy >= 2) with a
    np.float64 frame_rate (as h5py returns the attribute) does; a Python float, or numpy 1.x, divides in float32.  The output is
    float32 either way; only its rounding differs."""
    h = 1 / frame_rate
    return (np.zeros(1, np.float32) / (2.0 * h)).dtype == np.float64


def param_field(flow, mask, param, frame_rate, n_used):
    """OpticalFlowDataset's get_masked_arr(param, label) for frames [0, n_used), numpy as the reference runs it: vel =
    flow.astype(float32); accel = np.gradient(vel, 1 / frame_rate, axis=0); pwr = vel * accel; times the mask.  The gradient sees
    frame n_used too (when it exists), as it does over the whole study."""
    if param not in PARAMS:
        raise ValueError(f"param must be one of {PARAMS}, got {param!r}")
    flow = np.asarray(flow)
    N = flow.shape[0]
    n_used = int(n_used)
    if param == "velocity":
        field = flow[:n_used].astype(np.float32)
    else:
        vel = flow[:min(N, n_used + 1)].astype(np.float32)
        accel = np.gradient(vel, 1 / frame_rate, axis=0)[:n_used]
        field = accel if param == "acceleration" else vel[:n_used] * accel
    return field * np.asarray(mask)[:n_used]


def param_radlong_stats(flow, mask, param, frame_rate, n_used, centroid_list, perc_lo=1, perc_hi=99, nbins=1000, return_arrays=False, *,
                        engine=None):
    """calculate_3dhist_radlong (analyze_optical_flow.py:320-343) after its centroid step, for the param field of a study: flow
    [N,H,W,2] (float16 as the study file holds it, or float32), mask [N,H,W,C] (the 'rv' mask), n_used = ds.nframes frames
    projected, centroid_list of n_used (row, col).  Returns the dict of radlong_stats_device.  With `engine` the field, projection,
    histogram and order statistics run on the device (tf_radlong_project_param, tf_radlong_hist, tf_radlong_select); without, numpy."""
    if param not in PARAMS:
        raise ValueError(f"param must be one of {PARAMS}, got {param!r}")
    n_used = int(n_used)
    centroid_list = _frame_centroids(n_used, centroid_list)
    if engine is None:
        rad, lon = calculate_comp_magnitude(param_field(flow, mask, param, frame_rate, n_used), centroid_list)
        out = {}
        for name, arr in (("radial", rad), ("longitudinal", lon)):
            f, e, hi, lo = calc_bidirectional_hist(arr, n_used, perc_lo=perc_lo, perc_hi=perc_hi, nbins=nbins)
            out[name] = (f, np.asarray(e)[:-1], hi, lo)
        if return_arrays:
            out["rad_arr"], out["long_arr"] = rad, lon
        return out
    ds = SimpleNamespace(flow=flow, vel_array=flow, frame_rate=frame_rate, get_mask=lambda label: mask)      # what _Tail reads of a study
    return _Tail(ds, engine).radlong_stats(param, n_used, centroid_list, perc_lo, perc_hi, nbins, return_arrays)


def _frame_centroids(n, centroids, ds=None, engine=None, **av):
    """`centroids`, or (None) the centroid step of `ds` with av_centroids' keywords `av`: one centroid per frame, or ValueError"""
    if centroids is None:
        centroids = av_centroids(ds.get_mask("av"), n, engine=engine, **av)
    if len(centroids) != n:
        raise ValueError(f"{len(centroids)} centroids for {n} frames")
    return centroids


def calculate_3dhist_radlong(ds, param, nbins=1000, perc_lo=1, perc_hi=99, av_filter_flag=True, av_savgol_window=10, av_savgol_poly=4, *,
                             engine=None, centroids=None):
    """The reference's calculate_3dhist_radlong(ds, param) (analyze_optical_flow.py:320-343): {'radial': (freq, edges[:-1], hi, lo),
    'longitudinal': (...)}, or None (logged) for an unknown param or a mode without 'RVIO'.  `ds` is the reference's
    OpticalFlowDataset or a FlowStudy: .flow (or .vel_array), .frame_rate, .nframes, .mode, .get_mask(label).  `centroids` (what
    av_centroids returned) skips the centroid step, so that the three params of a study share it.  With `engine` (a DenseFlow) every
    per-pixel step runs on the device."""
    if param not in PARAMS:
        log.error("%r is not a valid optical flow parameter, choose from %s", param, list(PARAMS))
        return None
    if "RVIO" not in ds.mode:
        log.error("only mode=RVIO_2class is supported for radlong functions, got mode=%s", ds.mode)
        return None
    tail = _tail(ds, engine)
    n = int(ds.nframes)
    centroids = _frame_centroids(n, centroids, ds, engine, filter=av_filter_flag, savgol_window=av_savgol_window, savgol_poly=av_savgol_poly)
    if tail is None:
        flow, mask = _study_arrays(ds, "rv")
        return param_radlong_stats(flow, mask, param, ds.frame_rate, n, centroids, perc_lo=perc_lo, perc_hi=perc_hi, nbins=nbins)
    return tail.radlong_stats(param, n, centroids, perc_lo, perc_hi, nbins)


class FlowStudy:
    """What calculate_3dhist_radlong reads of a study, built from arrays: flow [N,H,W,2] as given (float16 as the study file holds
    it: the device upload is then 2 bytes per component), masks {label: [N,H,W,C]}, frame_rate, nframes (default N - 2, as
    OpticalFlowDataset reads attrs['nframes'] - 2 of a file whose flow has attrs['nframes'] frames), mode; and, for the overlay
    video, echo [>= nframes,H,W] as the study file holds it (float16) and filename (the stem of the video's name)."""

    def __init__(self, flow, masks, frame_rate, nframes=None, mode="RVIO_2class", echo=None, filename="study"):
        self.echo = None if echo is None else np.asarray(echo)
        self.filename = filename
        self.flow = np.asarray(flow)
        if self.flow.ndim != 4 or self.flow.shape[3] != 2:
            raise ValueError(f"flow must be [N,H,W,2], got {self.flow.shape}")
        self.masks = dict(masks)
        self.frame_rate = frame_rate
        self.nframes = int(self.flow.shape[0] - 2 if nframes is None else nframes)
        self.mode = mode
        self.accepted_labels = list(self.masks)

    @property
    def vel_array(self):
        return self.flow.astype(np.float32)

    def get_mask(self, label):
        if label not in self.masks:
            log.error("%s not a valid key, choose from %s", label, self.accepted_labels)
            return None
        return self.masks[label]

    def get_echo(self):
        return self.echo

    @classmethod
    def from_hdf5(cls, path):
        """A study file in the reference's layout (hdf5_out.py), read as OpticalFlowDataset reads it, the flow kept float16.
        Needs h5py."""
        import h5py
        with h5py.File(path, "r") as f:
            d = f["flow"]
            flow = d[()]
            a = d.attrs
            frame_rate = a["frame_rate"] if a["units_converted"] else 1
            masks = {str(k): f[k][()] for k in a["labels"]}
            echo = f["echo"][()] if "echo" in f else None
            # (OpticalFlowDataset's filename: the base name less its last four characters, whatever the extension)
            return cls(flow, masks, frame_rate, nframes=a["nframes"] - 2, mode=a["mode"], echo=echo, filename=os.path.basename(path)[:-4])


class HeldMask:
    """What HeldStudy.get_mask returns: the name of a mask held on the device, for the functions that take a mask array."""

    def __init__(self, study, label, shape):
        self.study, self.label, self.shape = study, label, tuple(shape)


class HeldStudy:
    """The `ds` of the analysis functions for the study held on `engine` (a DenseFlow): what FlowStudy is for arrays on the host.
    Made after the study and its masks are on the device -- DenseFlow.hold_study / hold_mask, or a study call with hold=True and
    hold_mask -- or by from_study / from_hdf5, which upload the flow, the echo and every mask once.  nframes defaults to N - 2, as
    FlowStudy's.  calculate_3dhist_radlong, calculate_3dhist, angle_mode_series, area_series, av_centroids, radlong_overlay,
    visualize_radlong, magnitude_overlay and visualize_magnitude then read the held arrays when they are given this engine as `engine`; with engine=None or another engine
    they raise, since the arrays are not on the host and nothing falls back to a host path.  The object belongs to the generation of
    the held study it was made at: once the engine's held study has been replaced or released, using it raises."""

    def __init__(self, engine, frame_rate, nframes=None, mode="RVIO_2class", filename="study"):
        held = engine.held
        if held is None:
            raise ValueError("the engine holds no study (hold_study, or a study call with hold=True)")
        self.engine = engine
        self.generation = held.generation
        self.shape = (held.N, held.H, held.W)
        self.n_echo = held.n_echo
        self.frame_rate = frame_rate
        self.nframes = int(held.N - 2 if nframes is None else nframes)
        self.mode = mode
        self.filename = filename

    def check(self, engine):
        """raises unless `engine` is the one that holds this study, and still holds it"""
        if engine is None:
            raise ValueError("a HeldStudy's arrays are on the device: pass engine=<the DenseFlow that holds it> (there is no host path)")
        if engine is not self.engine:
            raise ValueError("this HeldStudy is held on another engine; its arrays are not on the host and not on this engine")
        held = engine.held
        if held is None or held.generation != self.generation:
            raise RuntimeError("stale HeldStudy: the engine's held study has been replaced or released since it was made")
        return held

    @property
    def accepted_labels(self):
        held = self.engine.held
        return list(held.masks) if held is not None and held.generation == self.generation else []

    def get_mask(self, label):
        held = self.check(self.engine)
        if label not in held.masks:
            log.error("%s not a valid key, choose from %s", label, list(held.masks))
            return None
        n, Cm = held.masks[label]
        return HeldMask(self, label, (n, held.H, held.W, Cm))

    @classmethod
    def from_study(cls, engine, study):
        """Upload a FlowStudy's flow (float16, as the study file holds it), its echo (float16, or None) and every mask (bool or uint8,
        1 or 2 channels), once."""
        flow = np.asarray(study.flow)
        if flow.dtype != np.float16:
            raise ValueError(f"a held study's flow is the study file's float16, got {flow.dtype}")
        echo = study.get_echo()
        if echo is not None and np.asarray(echo).dtype != np.float16:
            raise ValueError(f"a held study's echo is the study file's float16, got {np.asarray(echo).dtype}")
        engine.hold_study(flow, echo)
        for label, mask in study.masks.items():
            engine.hold_mask(label, mask)
        return cls(engine, study.frame_rate, nframes=study.nframes, mode=study.mode, filename=study.filename)

    @classmethod
    def from_hdf5(cls, engine, path, inflate="h5py"):
        """A study file in the reference's layout, held on `engine`.  Needs h5py.  `inflate` says who inflates the file's gzip chunks:
          "h5py"    h5py does, chunk after chunk on this thread (FlowStudy.from_hdf5), and the arrays are uploaded: the default
          "host"    the chunks are read as they are stored (study_chunks), inflated by zlib in a thread pool (unchunk_host), uploaded
          "device"  the chunks are read as they are stored and uploaded compressed; the device inflates and assembles them
                    (DenseFlow.hold_study_chunks / hold_mask_chunks)
        The held study is the same bytes whichever way.  A file whose datasets are not plain gzip chunks (contiguous, another filter
        in the pipeline), or an h5py without the direct-chunk calls, is read the "h5py" way, with one logged reason."""
        if inflate not in INFLATE_WAYS:
            raise ValueError(f"inflate must be one of {INFLATE_WAYS}, got {inflate!r}")
        if inflate != "h5py":
            try:
                return cls.from_chunks(engine, study_chunks(path), inflate=inflate)
            except ChunksUnavailable as e:
                log.warning("%s: read through h5py instead of inflate=%r: %s", path, inflate, e)
        return cls.from_study(engine, FlowStudy.from_hdf5(path))

    @classmethod
    def from_chunks(cls, engine, record, inflate="device"):
        """A study_chunks / load_chunks record held on `engine`: inflate = "device" (the compressed chunks go up) or "host"
        (unchunk_host, then the arrays).  Each array is held whole or not at all, but the study is held array by array, the flow and
        echo first: a flow or echo chunk that does not decode raises and leaves the study held before; a mask chunk that does not
        decode raises with the new study held and the masks before it (the way "host" inflates everything before it holds anything)."""
        if inflate not in INFLATE_WAYS[1:]:
            raise ValueError(f"inflate must be one of {INFLATE_WAYS[1:]}, got {inflate!r}")
        a, ds = record["attrs"], record["datasets"]
        frame_rate = a["frame_rate"] if a["units_converted"] else 1
        labels = [str(k) for k in a["labels"]]
        kw = dict(nframes=int(a["nframes"]) - 2, mode=str(a["mode"]), filename=str(record["filename"]))
        if inflate == "host":
            return cls.from_study(engine, FlowStudy(unchunk_host(ds["flow"]), {k: unchunk_host(ds[k]) for k in labels}, frame_rate,
                                                    echo=unchunk_host(ds["echo"]) if "echo" in ds else None, **kw))
        engine.hold_study_chunks(ds["flow"], ds.get("echo"))
        for k in labels:
            engine.hold_mask_chunks(k, ds[k])
        return cls(engine, frame_rate, **kw)


# ---- a study file's chunks as they are stored -----------------------------------------------------------------------------------
INFLATE_WAYS = ("h5py", "host", "device")
_DS_FIELDS = ("shape", "dtype", "chunks", "coord", "filter_mask", "off", "len", "blob")
_ATTRS = ("frame_rate", "units_converted", "nframes", "mode", "labels")


class ChunksUnavailable(ValueError):
    """study_chunks cannot hand over a file's chunks as they are stored; the message says why"""


def chunks_record(shape, dtype, chunks, stored):
    """A dataset record from its parts: stored = [(coord, filter_mask, bytes)] of the chunks the file wrote, coord the element offset
    of the chunk's first element, filter_mask HDF5's (bit 0 set: the bytes are the chunk itself, no filter was applied), bytes a
    zlib stream of the whole chunk (edge chunks are stored whole).  Plain data: tuples, a string and numpy arrays; the chunks' bytes
    lie end to end in `blob`, chunk i at [off[i], off[i] + len[i])."""
    ndim = len(shape)
    lens = np.array([len(b) for _, _, b in stored], np.uint32)
    off = np.zeros(len(stored), np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return {"shape": tuple(int(v) for v in shape), "dtype": str(np.dtype(dtype)), "chunks": tuple(int(v) for v in chunks),
            "coord": np.array([c for c, _, _ in stored], np.int64).reshape(len(stored), ndim),
            "filter_mask": np.array([m for _, m, _ in stored], np.uint32), "off": off, "len": lens,
            "blob": np.frombuffer(b"".join(bytes(b) for _, _, b in stored), np.uint8)}


def _dataset_chunks(ds, name):
    import h5py
    if ds.chunks is None:
        raise ChunksUnavailable(f"dataset {name!r} is contiguous, not chunked")
    if not all(hasattr(ds.id, f) for f in ("get_num_chunks", "get_chunk_info", "read_direct_chunk")):
        raise ChunksUnavailable("this h5py has no get_num_chunks / get_chunk_info / read_direct_chunk")
    plist = ds.id.get_create_plist()
    filters = [plist.get_filter(i)[0] for i in range(plist.get_nfilters())]
    if filters not in ([], [h5py.h5z.FILTER_DEFLATE]):
        raise ChunksUnavailable(f"dataset {name!r} has the filter pipeline {filters}, not gzip alone")
    stored = []
    for i in range(ds.id.get_num_chunks()):
        info = ds.id.get_chunk_info(i)
        mask, data = ds.id.read_direct_chunk(info.chunk_offset)
        stored.append((info.chunk_offset, mask if filters else 1, data))       # (no filter at all: every chunk is its own bytes)
    return chunks_record(ds.shape, ds.dtype, ds.chunks, stored)


def study_chunks(path):
    """What HeldStudy.from_hdf5 needs of a study file, with the chunks of `flow`, `echo` and every mask in attrs['labels'] as the
    file stores them, not inflated: {'filename', 'attrs': {frame_rate, units_converted, nframes, mode, labels}, 'datasets': {name:
    chunks_record}}.  h5py and numpy only, no engine.  Raises ChunksUnavailable where a dataset is not plain gzip chunks."""
    import h5py
    with h5py.File(path, "r") as f:
        a = f["flow"].attrs
        labels = [str(k) for k in a["labels"]]
        rec = {"filename": os.path.basename(path)[:-4],
               "attrs": {"frame_rate": float(a["frame_rate"]), "units_converted": bool(a["units_converted"]), "nframes": int(a["nframes"]),
                         "mode": a["mode"].decode() if isinstance(a["mode"], bytes) else str(a["mode"]), "labels": labels},
               "datasets": {}}
        for name in ["flow"] + (["echo"] if "echo" in f else []) + labels:
            rec["datasets"][name] = _dataset_chunks(f[name], name)
    return rec


def save_chunks(record, npz_path):
    """a study_chunks record as an .npz of plain arrays (no pickle): one interpreter reads the file, another holds the study"""
    flat = {"filename": np.array(record["filename"]), "names": np.array(list(record["datasets"]))}
    for k in _ATTRS:
        flat[f"attrs/{k}"] = np.array(record["attrs"][k])
    for name, ds in record["datasets"].items():
        for k in _DS_FIELDS:
            flat[f"ds/{name}/{k}"] = np.array(ds[k])
    np.savez(npz_path, **flat)


def load_chunks(npz_path):
    with np.load(npz_path, allow_pickle=False) as z:
        a = {k: z[f"attrs/{k}"] for k in _ATTRS}
        rec = {"filename": str(z["filename"]),
               "attrs": {"frame_rate": float(a["frame_rate"]), "units_converted": bool(a["units_converted"]), "nframes": int(a["nframes"]),
                         "mode": str(a["mode"]), "labels": [str(k) for k in a["labels"]]},
               "datasets": {}}
        for name in (str(n) for n in z["names"]):
            ds = {k: z[f"ds/{name}/{k}"] for k in _DS_FIELDS}
            ds["shape"], ds["chunks"], ds["dtype"] = tuple(int(v) for v in ds["shape"]), tuple(int(v) for v in ds["chunks"]), str(ds["dtype"])
            rec["datasets"][name] = ds
    return rec


def unchunk_host(ds, workers=None):
    """A dataset record -> its array, on the host: zlib.decompress of every chunk in a thread pool (zlib releases the GIL; sized like
    the writer's, hdf5_out._workers; workers=1: no pool, this thread), then assembly; where the file wrote no chunk the array is 0, HDF5's fill value.  The numpy
    twin of DenseFlow.hold_study_chunks / hold_mask_chunks."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    from .hdf5_out import _workers
    shape, chunks, dt = tuple(ds["shape"]), tuple(ds["chunks"]), np.dtype(str(ds["dtype"]))
    blob, off, ln, mask = np.asarray(ds["blob"], np.uint8), ds["off"], ds["len"], ds["filter_mask"]
    out = np.zeros(shape, dt)
    want = int(np.prod(chunks, dtype=np.int64)) * dt.itemsize

    def one(i):
        b = blob[int(off[i]):int(off[i]) + int(ln[i])]
        raw = b.tobytes() if int(mask[i]) & 1 else zlib.decompress(b)
        if len(raw) != want:
            raise ValueError(f"chunk {i} inflates to {len(raw)} bytes, a chunk has {want}")
        at = [int(v) for v in ds["coord"][i]]
        keep = tuple(slice(0, min(c, s - o)) for o, c, s in zip(at, chunks, shape))
        out[tuple(slice(o, o + k.stop) for o, k in zip(at, keep))] = np.frombuffer(raw, dt).reshape(chunks)[keep]

    n = len(ln)
    if workers == 1:                                          # on the calling thread
        for i in range(n):
            one(i)
        return out
    with ThreadPoolExecutor(workers or _workers()) as pool:
        list(pool.map(lambda lo: [one(i) for i in range(lo, min(lo + 16, n))], range(0, n, 16)))
    return out


# ---- where a study's arrays are: the one place that knows ------------------------------------------------------------------------
def _study_arrays(ds, label):
    flow = getattr(ds, "flow", None)
    if flow is None:
        flow = ds.vel_array
    return flow, ds.get_mask(label)


class _Tail:
    """The device steps of the analysis functions behind `engine` (a DenseFlow), each in two implementations: for a `ds` whose arrays are on
    the host, which the engine uploads with every call, and (`held`) for the study the engine holds, through the held calls, which upload
    nothing.  A mask argument is what get_mask returned; the results are the engine's."""

    def __init__(self, ds, engine, held=False):
        self.ds, self.engine, self.held = ds, engine, held

    def _param(self, param):
        return PARAMS.index(param), 1 / self.ds.frame_rate, gradient_is_f64(self.ds.frame_rate)

    def centroids(self, mask, n):
        if self.held:
            return self.engine.held_av_centroids(mask.label, n)
        masks = np.asarray(mask)[:n]
        if masks.dtype not in (np.bool_, np.uint8) or masks.shape[3] not in (1, 2):
            masks = np.ascontiguousarray(masks[..., :1] != 0)
        return self.engine.av_centroids(masks)

    def first_region_areas(self, mask, n):
        """None for a host mask the engine does not take (another dtype or channel count, or empty): that one runs on the host"""
        if self.held:
            return self.engine.held_first_region_areas(mask.label, n)
        masks = np.asarray(mask)[:n]
        ok = masks.size > 0 and masks.dtype in (np.bool_, np.uint8) and masks.shape[3] in (1, 2)
        return self.engine.first_region_areas(masks) if ok else None

    def radlong_project(self, param, n, centroids, return_arrays=False):
        if self.held:
            return self.engine.held_radlong_project_param("rv", *self._param(param), n, centroids, return_arrays=return_arrays)
        flow, mask = _study_arrays(self.ds, "rv")
        mask = np.asarray(mask)
        if mask.dtype not in (np.bool_, np.uint8):
            raise ValueError(f"the device path takes a bool or uint8 mask (the study file's), got {mask.dtype}")
        return self.engine.radlong_project_param(flow, mask, *self._param(param), n, centroids, return_arrays=return_arrays)

    def radlong_stats(self, param, n, centroids, perc_lo, perc_hi, nbins, return_arrays=False):
        """the device part of param_radlong_stats and calculate_3dhist_radlong: the projection, then the statistics of its planes"""
        mm, nz, rad, lon = self.radlong_project(param, n, centroids, return_arrays)
        return _radlong_stats_resident(self.engine, n, mm, nz, perc_lo, perc_hi, nbins, rad, lon)

    def polar_project(self, param, label, n):
        if self.held:
            return self.engine.held_polar_project_param(label, *self._param(param), n)
        flow, mask = _study_arrays(self.ds, label)
        return self.engine.polar_project_param(flow, mask, *self._param(param), n)

    def echo(self, n):
        """the echo the overlay takes, known to cover n frames: the host array, or None for the held one, which stays where it is"""
        if not self.held:
            return _host_echo(self.ds, n)
        if self.ds.n_echo < 1:
            raise ValueError("the study has no echo frames")
        if self.ds.n_echo < n:
            raise ValueError(f"echo must be [>= {n},{self.ds.shape[1]},{self.ds.shape[2]}], the held one has {self.ds.n_echo} frames")

    def overlay(self, echo, lut_rad, lut_long):
        return self.engine.held_radlong_overlay(lut_rad, lut_long) if self.held else self.engine.radlong_overlay(echo, lut_rad, lut_long)

    def magnitude_overlay(self, param, label, n, echo, lut, norm_f64):
        if self.held:
            return self.engine.held_magnitude_overlay(label, *self._param(param), norm_f64, n, lut)
        flow, mask = _study_arrays(self.ds, label)
        mask = np.asarray(mask)
        if mask.dtype not in (np.bool_, np.uint8):
            raise ValueError(f"the device path takes a bool or uint8 mask (the study file's), got {mask.dtype}")
        return self.engine.magnitude_overlay(flow, mask, *self._param(param), norm_f64, n, echo, lut)


def _tail(src, engine):
    """The device side of `src` (a ds, or the mask av_centroids was given): the held one for what is held on the device (it raises unless
    `engine` holds it: there is no host path), the uploading one for host arrays and an engine, None for host arrays and no engine."""
    if isinstance(src, (HeldStudy, HeldMask)):
        ds = src.study if isinstance(src, HeldMask) else src
        ds.check(engine)
        return _Tail(ds, engine, held=True)
    return None if engine is None else _Tail(src, engine)


# ---- the polar steps: cv2.cartToPolar, calculate_3dhist, the angle detector's per-frame mode --------------------------------
_DEG = 180 / np.pi                                            # 180 / CV_PI (CV_PI is the double nearest pi, as np.pi)
_P1, _P3 = np.float32(0.9997878412794807) * np.float32(_DEG), np.float32(-0.3258083974640975) * np.float32(_DEG)
_P5, _P7 = np.float32(0.1555786518463281) * np.float32(_DEG), np.float32(-0.04432655554792128) * np.float32(_DEG)
_EPS32 = np.float32(np.finfo(np.float64).eps)                 # (float)DBL_EPSILON
_RAD32 = np.float32(np.pi / 180)                              # (float)(CV_PI / 180)


def fma32(a, b, c):
    """float32 fma(a, b, c) with one rounding, in numpy (which has no fma): a*b is exact in float64; s = p + c in float64 with its
    TwoSum error; s is made round-to-odd (stepped one ulp toward zero if it overshot the exact sum, then its lowest bit set, when
    the error is not zero), so that the final cast to float32 rounds the exact sum once (53 >= 24 + 2 bits)."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    inexact = err != 0
    if np.any(inexact):
        s = np.array(s, np.float64, copy=True)
        over = inexact & ((err < 0) == (s > 0))                 # |s| > |exact sum|: truncate toward zero first
        s[over] = np.nextafter(s[over], 0.0)
        v = s.view(np.int64)
        v[inexact] |= 1
    return s.astype(np.float32)


def cart_to_polar(x, y):
    """cv2.cartToPolar(x, y) for float32 in radians, as OpenCV 4.x's SIMD body computes it on an AVX2 (FMA3) or NEON build
    (modules/core/src/mathfuncs_core.simd.hpp: magnitude32f, fastAtan32f / v_atan_f32): (mag, ang), float32.  The same formula
    runs on the device (teeflow_polar.hip.h).  A restatement, not cv2: parity with cv2 is unpinned."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mag = np.sqrt(fma32(x, x, y * y))                          # v_muladd(x, x, y*y): y*y rounded first
        ax, ay = np.abs(x), np.abs(y)
        c = np.minimum(ax, ay) / (np.maximum(ax, ay) + _EPS32)
        cc = c * c
        a = fma32(fma32(fma32(cc, _P7, _P5), cc, _P3), cc, _P1) * c
        a = np.where(ax >= ay, a, np.float32(90) - a)
        a = np.where(x < 0, np.float32(180) - a, a)                # -0.0 is not < 0
        a = np.where(y < 0, np.float32(360) - a, a)
        ang = (a * _RAD32).astype(np.float32)
    return mag.astype(np.float32), ang


def polar_field(flow, mask, param, frame_rate, n_used):
    """cv2.cartToPolar of every frame of get_masked_arr(param, label): (mag, ang) float32 [n_used,H,W]"""
    field = param_field(flow, mask, param, frame_rate, n_used)
    return cart_to_polar(field[..., 0], field[..., 1])


def percentile_index(n, q, dtype=np.float32):
    """(prev, next, gamma) of np.percentile(a, q) for n values of float dtype: method 'linear' as numpy >= 2 computes it, q / 100
    and the virtual index (n - 1) * q in the data's dtype (numpy 1.x computes both in float64).  The result is
    _lerp(sorted(a)[prev], sorted(a)[next], gamma) in that dtype."""
    qq = np.asarray(np.true_divide(q, np.dtype(dtype).type(100)))
    vi = np.asarray((n - 1) * qq)
    prev = int(np.floor(vi))
    nxt = prev + 1
    if vi >= n - 1:                                            # above the last index: both are the maximum
        prev = nxt = -1
    gamma = np.asarray(vi - prev, dtype=vi.dtype)              # numpy's _get_gamma: from the clipped previous index
    return (prev % n, nxt % n, gamma[()])


def _polar_edges(mn, mx, nbins):
    """np.histogram's bin edges for range=(mn, mx) (np.float32 scalars, as np.min / np.max return them) of float32 data, from the
    numpy of this process (numpy 2 runs linspace in float32)"""
    return np.histogram_bin_edges(np.empty(0, np.float32), bins=nbins, range=(mn, mx))


def _valid(ds, param, label):
    if param not in PARAMS:
        log.error("%r is not a valid optical flow parameter, choose from %s", param, list(PARAMS))
        return False
    if label not in list(ds.accepted_labels):
        log.error("%r not a valid key, choose from %s", label, list(ds.accepted_labels))
        return False
    return True


def _hist_host(mag, ang, n, nbins, percentile):
    """the reference's two loops (analyze_optical_flow.py:927-961) on float32 planes, numpy as it runs them"""
    mag_freq, hi, mag_edges = [], [], []
    mag_max, mag_min = np.max(mag), np.min(mag)
    for i in range(n):
        flat = np.ravel(mag[i])
        nz = flat[flat != 0]
        if len(nz) == 0:
            hi.append(hi[-1])                                  # IndexError on an empty first frame, as the reference
            mag_freq.append(mag_freq[-1])
        else:
            hi.append(np.percentile(nz, percentile))
            freq, mag_edges = np.histogram(nz, bins=nbins, range=(mag_min, mag_max))
            mag_freq.append(freq + 1)
    ang_freq, ang_edges = [], []
    ang_max, ang_min = np.max(ang), np.min(ang)
    for i in range(n):
        flat = np.ravel(ang[i])
        nz = flat[flat != 0]
        if len(nz) == 0:
            ang_freq.append(mag_freq[-1])                      # the reference's quirk: the LAST frame's magnitude row
        else:
            freq, ang_edges = np.histogram(nz, bins=nbins, range=(ang_min, ang_max))
            ang_freq.append(freq + 1)
    return np.stack(mag_freq), np.stack(ang_freq), mag_edges[:-1], ang_edges[:-1], np.asarray(hi)


def _hist_device(engine, n, mm, nz, nbins, percentile):
    """the same from the planes tf_polar_project_param left resident: tf_radlong_hist over numpy's float32 edges (passed as float64,
    exactly) and tf_radlong_select for the order statistics np.percentile interpolates between"""
    mn, mx, amn, amx = (np.float32(v) for v in mm)
    cnt, acnt = nz[:, 0], nz[:, 1]
    if cnt[0] == 0:
        raise IndexError("list index out of range")           # the reference's perc_hi[-1] on an empty first frame
    _check_finite_range(mn, mx)                                # np.histogram's ValueError, before tf_radlong_hist runs
    mag_edges = _polar_edges(mn, mx, nbins)
    # k_radlong_hist estimates the bin in float64 and fixes it up by one against these edges, as numpy fixes up its float32
    # estimate: both estimates lie within one bin of the edge-defined one, so both end in the same bin
    freq = engine.radlong_hist(0, mag_edges.astype(np.float64), n)       # (exact)
    ranks = np.full((n, 4), -1, np.int64)
    gam = [None] * n
    for i in range(n):
        if cnt[i] > 0:
            ranks[i, 0], ranks[i, 1], gam[i] = percentile_index(int(cnt[i]), percentile)
    vals = engine.radlong_select(0, ranks)
    mag_freq, hi = [], []
    for i in range(n):
        if cnt[i] == 0:
            hi.append(hi[-1]); mag_freq.append(mag_freq[-1])
        else:
            hi.append(_lerp(np.float32(vals[i, 0]), np.float32(vals[i, 1]), gam[i]))
            mag_freq.append(freq[i] + 1)
    ang_edges = []
    if acnt.any():
        _check_finite_range(amn, amx)
        ang_edges = _polar_edges(amn, amx, nbins)
        afreq = engine.radlong_hist(1, ang_edges.astype(np.float64), n)
    ang_freq = [afreq[i] + 1 if acnt[i] > 0 else mag_freq[-1] for i in range(n)]
    return np.stack(mag_freq), np.stack(ang_freq), mag_edges[:-1], ang_edges[:-1], np.asarray(hi)


def calculate_3dhist(ds, param, label, nbins=1000, percentile=99, *, engine=None):
    """The reference's calculate_3dhist(ds, param, label) (analyze_optical_flow.py:909-966): (mag_freq, ang_freq, mag_edges[:-1],
    ang_edges[:-1], hi_arr) for frames [0, ds.nframes) of cv2.cartToPolar(get_masked_arr(param, label)), quirks kept: freq + 1; an
    empty frame copies the previous row and hi; an empty angle frame takes the magnitude row of the study's last frame; an empty
    first frame raises IndexError; an unknown param or label is logged and gives None; a NaN or inf in the field (or a magnitude that
    overflows float32) raises np.histogram's ValueError.  float32 statistics as numpy >= 2 computes them.
    `ds` is the reference's OpticalFlowDataset or a FlowStudy.  With `engine` (a DenseFlow) every per-pixel step runs on the
    device, with the same bits."""
    tail = _tail(ds, engine)
    if not _valid(ds, param, label):
        return None
    n = int(ds.nframes)
    if tail is None:
        flow, mask = _study_arrays(ds, label)
        mag, ang = polar_field(flow, mask, param, ds.frame_rate, n)
        return _hist_host(mag, ang, n, nbins, percentile)
    mm, nz, _, _, _ = tail.polar_project(param, label, n)
    return _hist_device(engine, n, mm, nz, nbins, percentile)


def _mode_of_rounded(ang):
    """scipy.stats.mode of np.round(ang, 2)'s non-zero values: the smallest of the most frequent, np.float32(nan) if none"""
    flat = np.ravel(np.round(ang, decimals=2))
    nz = flat[flat != 0]
    if len(nz) == 0:
        return np.float32(np.nan)
    vals, counts = np.unique(nz, return_counts=True)
    return vals[np.argmax(counts)]


def angle_mode_series(ds, param, label, *, engine=None):
    """The per-frame series AngleDetector.detect (cardiac_cycle_detection.py:100-120) hands to its SpectralSmoother: for frames
    [0, ds.nframes), scipy.stats.mode of the non-zero np.round(ang, 2) of cv2.cartToPolar(get_masked_arr(param, label)), float32,
    NaN for a frame without any.  With `engine` (a DenseFlow) it runs on the device (tf_polar_project_param), with the same bits.
    Non-finite input: the host twin lets np.unique count NaN angles; the device path does not imitate that (its bins drop a NaN
    angle, and fminf / fmaxf in its cart_to_polar drop a NaN operand where numpy propagates it) and raises ValueError instead
    whenever a magnitude or an angle of the field is NaN or inf, so it never returns a mode where the twin's differs."""
    tail = _tail(ds, engine)
    if param not in PARAMS:
        raise ValueError(f"param must be one of {PARAMS}, got {param!r}")
    if label not in list(ds.accepted_labels):
        raise ValueError(f"{label!r} not a valid key, choose from {list(ds.accepted_labels)}")
    n = int(ds.nframes)
    if tail is None:
        flow, mask = _study_arrays(ds, label)
        _, ang = polar_field(flow, mask, param, ds.frame_rate, n)
        return np.asarray([_mode_of_rounded(ang[i]) for i in range(n)], np.float32)
    mm, _, mode, _, _ = tail.polar_project(param, label, n)
    if not np.isfinite(mm).all():
        raise ValueError(f"the field holds NaN or inf (magnitude range [{mm[0]}, {mm[1]}], angle range [{mm[2]}, {mm[3]}])")
    return mode


# ---- the area detector's per-frame region area ---------------------------------------------------------------------------------
def _first_region_area(frame):
    """props[0].area of skimage.measure.regionprops(skimage.measure.label(frame)), or None for a frame of zeros.  label joins
    8-connected pixels of equal value and numbers the regions by their first pixel in raster order, so region 1 is the region of
    {frame == v0} that holds the first non-zero pixel, v0 that pixel's value (checked against skimage 0.18.3 on bool, integer and
    float masks of one to three non-zero values)."""
    from scipy import ndimage
    frame = np.asarray(frame)
    flat = frame.ravel()
    nz = np.flatnonzero(flat != 0)
    if len(nz) == 0:
        return None
    lab, _ = ndimage.label(frame == flat[nz[0]], structure=np.ones((3, 3)))
    return int((lab == lab.ravel()[nz[0]]).sum())


def area_series(ds, label, *, engine=None):
    """The per-frame series AreaDetector.detect (cardiac_cycle_detection.py:159-172) hands to its SpectralSmoother, its area_list:
    for frames [0, ds.nframes) the area of the first region of ds.get_mask(label)[i, :, :, 0] (skimage label + regionprops,
    props[0].area), int64; a frame without a region takes the previous frame's value (0 on frame 0) with a warning.  ds: an
    OpticalFlowDataset, a FlowStudy or anything with get_mask(label) and nframes.  With `engine` (a DenseFlow) the labelling runs on
    the device (tf_first_region_areas), with the same values; a mask that is neither bool nor uint8, or has other than 1 or 2
    channels, runs on the host whatever the engine.  The smoother, the baseline and the peak search stay with the caller."""
    tail = _tail(ds, engine)
    mask_arr = ds.get_mask(label)
    n = int(ds.nframes)
    shape = np.shape(mask_arr)                                # (a HeldMask has the shape of the mask it names)
    if len(shape) != 4:
        raise ValueError(f"the {label!r} mask must be [N,H,W,C], got shape {shape}")
    if n > shape[0]:
        raise IndexError(f"nframes {n} > {shape[0]} mask frames")
    areas = tail.first_region_areas(mask_arr, n) if tail is not None and n > 0 else None
    if areas is not None:
        found = [int(a) if a > 0 else None for a in areas]
    else:
        masks = np.asarray(mask_arr) if n > 0 else ()
        found = [_first_region_area(masks[i, :, :, 0]) for i in range(n)]
    out = np.zeros(max(n, 0), np.int64)
    for i in range(n):
        if found[i] is not None:
            out[i] = found[i]
        else:
            out[i] = out[i - 1] if i > 0 else 0
            log.warning("no %s mask at frame %d: area carried over", label, i)
    return out


# ---- the rad/long overlay video: visualize_radlong ---------------------------------------------------------------------------
COLORMAP_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormap_luts.json")  # tools/make_colormap_luts.py writes it


def committed_colormap_luts():
    """{name: float64 [256,3]} from colormap_luts.json: text, each float64 written with the shortest decimal string that reads back as the
    same bits (Python's repr), so the tables are matplotlib's exactly.  (Text rather than an .npz: package data that can be read and
    diffed; the repository's binary files are the test vectors under tests/golden/ alone.)"""
    import json
    with open(COLORMAP_FILE) as f:
        return {name: np.array(rows, np.float64).reshape(256, 3) for name, rows in json.load(f)["luts"].items()}


def colormap_lut(name):
    """The 256-entry RGB table of matplotlib's colormap `name`, float64 [256,3]: from matplotlib when it is importable (a colormap
    with N != 256 is refused), else from the committed colormap_luts.json (bwr, BrBG, PiYG, viridis: matplotlib's own tables).  An
    unknown name raises ValueError."""
    try:
        import matplotlib
        from matplotlib import cm
    except ImportError:
        matplotlib = None
    if matplotlib is None:
        luts = committed_colormap_luts()
        if name not in luts:
            raise ValueError(f"{name!r} is not among the committed colormaps {sorted(luts)} and matplotlib is not importable")
        return luts[name]
    try:
        cmap = matplotlib.colormaps[name] if hasattr(matplotlib, "colormaps") else cm.get_cmap(name)
    except (KeyError, ValueError) as e:
        raise ValueError(f"{name!r} is not a matplotlib colormap") from e
    if cmap.N != 256:
        raise ValueError(f"colormap {name!r} has {cmap.N} entries; the overlay takes 256-entry colormaps")
    return np.array(cmap(np.arange(256))[:, :3], np.float64)      # integer input indexes the table itself


def _check_lut(lut, name):
    lut = np.ascontiguousarray(lut, dtype=np.float64)
    if lut.shape != (256, 3):
        raise ValueError(f"{name} must be [256,3], got shape {lut.shape}")
    if not (np.isfinite(lut).all() and (lut >= 0).all()):
        raise ValueError(f"{name} holds a negative or non-finite entry")
    return lut


def overlay_host(rad, lon, echo, lut_rad, lut_long):
    """The per-pixel part of visualize_radlong in numpy, as the reference computes it but without its RGBA float64 arrays:
    (out uint8 [n,H,2W,3], info float64 [3] = (half, echo max, m2)) from the float64 planes rad / lon [n,H,W], the echo [>= n,H,W]
    (float16 or uint8) and two [256,3] tables.
      half = max|rad[0]|: the reference makes ONE CenteredNorm, which autoscales on its first call only (frame 0, radial) and then
             serves every frame of both components; t = (a + half) / (2 half), 0 everywhere when half == 0, not clipped;
      index = clip(floor(t * 256), 0, 255): matplotlib's lookup, under = entry 0, over = entry 255;
      overlay3: ((0.5 * (echo / max echo)) + (0.5 * (colour / m2))) * 255, cast to uint8 (truncation); m2 = the largest channel among
             the colours actually produced; a float16 echo keeps float16 through its quotient and the product with 0.5.
    ValueError where the reference's cast is undefined: NaN or inf in a plane, a negative or non-finite echo value, an echo maximum
    of 0, 2 * half overflowing, m2 == 0."""
    rad, lon = np.asarray(rad, np.float64), np.asarray(lon, np.float64)
    n, H, W = rad.shape
    lut_rad, lut_long = _check_lut(lut_rad, "lut_rad"), _check_lut(lut_long, "lut_long")
    echo = np.asarray(echo)
    if echo.dtype not in (np.float16, np.uint8):
        raise ValueError(f"echo must be float16 or uint8, got {echo.dtype}")
    if echo.ndim != 3 or echo.shape[0] < n or echo.shape[1:] != (H, W):
        raise ValueError(f"echo must be [>= {n},{H},{W}], got shape {echo.shape}")
    echo = echo[:n]
    if not (np.isfinite(rad).all() and np.isfinite(lon).all()):
        raise ValueError("the rad/long planes hold NaN or inf")
    if echo.dtype == np.float16 and not (np.isfinite(echo).all() and (echo >= 0).all()):
        raise ValueError("the echo holds a negative or non-finite value")
    emax = np.max(echo)
    if emax == 0:
        raise ValueError("the echo's maximum is 0")
    half = np.max(np.abs(rad[0]))
    with np.errstate(over="ignore"):
        two_half = half - (-half)                                   # vmax - vmin
    if not np.isfinite(two_half):
        raise ValueError(f"the norm's range 2 * {half} overflows")

    def index(a):
        if half == 0:
            return np.zeros(a.shape, np.uint8)
        idx = np.empty(a.shape, np.uint8)
        with np.errstate(over="ignore"):
            for i in range(a.shape[0]):                             # frame by frame: the float64 temporaries stay one frame large
                idx[i] = np.clip(((a[i] + half) / two_half) * 256, 0, 255).astype(np.uint8)
        return idx
    ir, il = index(rad), index(lon)
    used_r = np.bincount(ir.ravel(), minlength=256) > 0
    used_l = np.bincount(il.ravel(), minlength=256) > 0
    m2 = max(lut_rad[used_r].max(), lut_long[used_l].max())
    if m2 == 0:
        raise ValueError("every colour used is black (the colour maximum is 0)")
    col_r, col_l = 0.5 * (lut_rad / m2), 0.5 * (lut_long / m2)
    out = np.empty((n, H, 2 * W, 3), np.uint8)
    for i in range(n):
        e = (0.5 * (echo[i] / emax)).astype(np.float64)[..., None]  # float16 / float16 and 0.5 * float16 stay float16; uint8 / uint8 is float64
        out[i, :, :W] = ((e + col_r[ir[i]]) * 255).astype(np.uint8)
        out[i, :, W:] = ((e + col_l[il[i]]) * 255).astype(np.uint8)
    return out, np.array([half, emax, m2], np.float64)


def radlong_overlay(ds, param, av_filter_flag=True, av_savgol_window=10, av_savgol_poly=4, colormap_rad="bwr", colormap_long="BrBG", *,
                    engine=None, centroids=None, return_info=False):
    """The frames visualize_radlong (analyze_optical_flow.py:496-560) hands to its video writer: uint8 [ds.nframes,H,2W,3], the radial
    projection of get_masked_arr(param, 'rv') through `colormap_rad` on the left, the longitudinal one through `colormap_long` on the
    right, each blended half-and-half with the echo image; or None (logged) for an unknown param or a mode without 'RVIO', the
    reference's own refusals.  The colormaps are names (colormap_lut) or [256,3] tables; the defaults are the reference's, and
    VisualizationManager.visualize_radlong (visualization.py:241-297) is the same with other names.  `ds` is the reference's
    OpticalFlowDataset or a FlowStudy with an echo; `centroids` (what av_centroids returned) skips the centroid step.
    Without `engine`, numpy (overlay_host); with `engine` (a DenseFlow) the projection and the rendering run on the device
    (tf_radlong_project_param, tf_radlong_overlay) and only the frames come back.  Both give the same bytes.  Both raise ValueError for
    NaN or inf in the projections, a negative or non-finite echo value, an echo maximum of 0, a norm range that overflows and a colour
    maximum of 0: the reference casts NaN or out-of-range values to uint8 there, which is undefined and differs between machines.
    return_info adds (half, echo max, m2) as a second result."""
    if param not in PARAMS:
        log.error("%r is not a valid optical flow parameter, choose from %s", param, list(PARAMS))
        return None
    if "RVIO" not in ds.mode:
        log.error("only RVIO modes are supported for radlong visualization, got mode=%s", ds.mode)
        return None
    lut_rad = colormap_lut(colormap_rad) if isinstance(colormap_rad, str) else colormap_rad
    lut_long = colormap_lut(colormap_long) if isinstance(colormap_long, str) else colormap_long
    lut_rad, lut_long = _check_lut(lut_rad, "colormap_rad"), _check_lut(lut_long, "colormap_long")
    tail = _tail(ds, engine)
    n = int(ds.nframes)
    echo = _host_echo(ds, n) if tail is None else tail.echo(n)
    centroids = _frame_centroids(n, centroids, ds, engine, filter=av_filter_flag, savgol_window=av_savgol_window, savgol_poly=av_savgol_poly)
    if tail is None:
        flow, mask = _study_arrays(ds, "rv")
        rad, lon = calculate_comp_magnitude(param_field(flow, mask, param, ds.frame_rate, n), centroids)
        out, info = overlay_host(rad, lon, echo, lut_rad, lut_long)
    else:
        tail.radlong_project(param, n, centroids)
        out, info = _device_overlay(lambda: tail.overlay(echo, lut_rad, lut_long))
    return (out, info) if return_info else out


def _host_echo(ds, n):
    """the echo of a study on the host, float16 or uint8 and covering n frames of the flow's size, or ValueError"""
    echo = ds.get_echo()
    if echo is None:
        raise ValueError("the study has no echo frames")
    echo = np.asarray(echo)
    if echo.dtype not in (np.float16, np.uint8):
        raise ValueError(f"echo must be float16 (the study file's) or uint8, got {echo.dtype}")
    H, W = np.shape(_study_arrays(ds, "rv")[0])[1:3]
    if echo.ndim != 3 or echo.shape[0] < n or echo.shape[1:] != (H, W):
        raise ValueError(f"echo must be [>= {n},{H},{W}], got shape {echo.shape}")
    return echo


def _device_overlay(render):
    """render(), the library's refusals of the data raised as the host twin's ValueErrors"""
    from .exceptions import OpticalFlowCalculationError
    try:
        return render()
    except OpticalFlowCalculationError as e:
        if getattr(e, "code", None) == _lib.TF_ERR_INVALID_ARG:
            raise ValueError(str(e)) from e
        raise


def visualize_radlong(ds, param, save_dir, fps=30, av_filter_flag=True, av_savgol_window=10, av_savgol_poly=4, colormap_rad="bwr",
                      colormap_long="BrBG", *, engine=None, centroids=None, writer_factory=None):
    """The reference's visualize_radlong(ds, param, save_dir) (analyze_optical_flow.py:496-560): renders radlong_overlay's frames and
    writes them to <save_dir>/<ds.filename>_<param>_radlong_overlay.mp4, one append_data call per frame, then close.  Returns the
    path, or None under radlong_overlay's refusals (nothing is written then).  writer_factory(path, fps=) makes the writer; the default
    is imageio.v2.get_writer, imported when needed.  The encoding itself is the writer's."""
    frames = radlong_overlay(ds, param, av_filter_flag=av_filter_flag, av_savgol_window=av_savgol_window, av_savgol_poly=av_savgol_poly,
                             colormap_rad=colormap_rad, colormap_long=colormap_long, engine=engine, centroids=centroids)
    if frames is None:
        return None
    if writer_factory is None:
        import imageio.v2 as iio
        writer_factory = iio.get_writer
    os.makedirs(save_dir, exist_ok=True)
    save_path = os.path.join(save_dir, f"{ds.filename}_{param}_radlong_overlay.mp4")
    writer = writer_factory(save_path, fps=fps)
    for i in range(frames.shape[0]):
        writer.append_data(frames[i])
    writer.close()
    return save_path


# ---- the single-component video: the magnitude overlay of example_peak_plots.py:459-513 -----------------------------------------
MAGNITUDE_COLORMAP_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormap_luts_magnitude.json")  # tools/make_magnitude_colormap_luts.py writes it


def committed_magnitude_luts():
    """{name: float64 [256,3]} from colormap_luts_magnitude.json, the second table file, in colormap_luts.json's format: 'hot', the
    reference's colormap for the magnitude overlay (matplotlib's own table; its row 0 is (0.0416, 0, 0), not black)."""
    import json
    with open(MAGNITUDE_COLORMAP_FILE) as f:
        return {name: np.array(rows, np.float64).reshape(256, 3) for name, rows in json.load(f)["luts"].items()}


def magnitude_colormap_lut(name):
    """colormap_lut for the magnitude overlay: from matplotlib when it is importable, else from the committed files, the magnitude
    overlay's own ('hot') before the rad/long overlay's four.  An unknown name raises ValueError."""
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        luts = {**committed_colormap_luts(), **committed_magnitude_luts()}
        if name not in luts:
            raise ValueError(f"{name!r} is not among the committed colormaps {sorted(luts)} and matplotlib is not importable") from None
        return luts[name]
    return colormap_lut(name)


def norm_is_f64():
    """Whether numpy, in this process, divides a float32 array in place by a np.float64 scalar in float64 (NEP 50, numpy >= 2: the
    quotient is formed in float64 and rounded to float32 once) or rounds the scalar to float32 first (numpy 1.x's value-based
    casting).  That is matplotlib's Normalize on a float32 frame: `resdat /= (vmax - vmin)` with vmin and vmax float64 scalars.
    Probed by value: (1 + 2^-22) / (1 + 2^-24) is 1 + 2^-23 by the first rule and 1 + 2^-22 by the second."""
    a = np.array([1 + 2.0 ** -22], np.float32)
    a /= np.float64(1 + 2.0 ** -24)
    return bool(a[0] == np.float32(1 + 2.0 ** -23))


def magnitude_norm_index(mag, vmin, vmax, norm_f64):
    """(t float32, idx uint8) of one float32 magnitude frame under Normalize(vmin, vmax) and a 256-entry colormap's lookup, as the
    reference's numpy / matplotlib run them: t = (mag - vmin) / (vmax - vmin) with the float32 difference in the numerator and the
    float64 difference of the extrema as divisor -- the quotient formed in float64 and rounded once (norm_f64) or the divisor rounded
    to float32 first; t = 0 if vmin == vmax; idx = min(trunc(t * 256), 255) (t is in [0, 1] for a frame within the extrema)."""
    mag = np.asarray(mag, np.float32)
    vmin, vmax = np.float32(vmin), np.float32(vmax)
    if vmin == vmax:
        return np.zeros(mag.shape, np.float32), np.zeros(mag.shape, np.uint8)
    d64 = np.float64(vmax) - np.float64(vmin)
    s = mag - vmin
    t = (s.astype(np.float64) / d64).astype(np.float32) if norm_f64 else s / np.float32(d64)
    return t, np.minimum((t * np.float32(256)).astype(np.int64), 255).astype(np.uint8)


def _magnitude(frame):
    """np.sqrt(x**2 + y**2) of one float32 [H,W,2] frame: two rounded squares, a rounded sum, a rounded root"""
    return np.sqrt(frame[..., 0] ** 2 + frame[..., 1] ** 2)


def magnitude_overlay_host(field, n_used, echo, lut, norm_f64=None):
    """The per-pixel part of the reference's single-component video in numpy, as the reference computes it but frame by frame, without
    its [N,H,W,4] float64 colour array: (out uint8 [n_used,H,W,3], info float64 [2] = (vmin, vmax), frame_info float64 [n_used,2] =
    each frame's (echo max, colour max)) from the float32 field [N,H,W,2] = get_masked_arr(param, label) over ALL the frames the
    file stores, the echo [>= n_used,H,W] (float16 or uint8) and a [256,3] table.
      mag = sqrt(x**2 + y**2) in float32; ONE Normalize(min mag, max mag) over all N frames, zeros outside the mask included;
      frames [0, n_used) are rendered: magnitude_norm_index (norm_f64=None: norm_is_f64(), this process's numpy), then per frame
      ((0.5 * (echo / max echo)) + (0.5 * (colour / max colour))) * 255 with the frame's own maxima, a maximum of 0 leaving its term
      undivided; a float16 echo keeps float16 through its quotient and the product with 0.5, and the result is stored into a float16
      array before uint8 truncates it (the reference's output array is np.zeros_like(gray2rgb(echo))); a uint8 echo divides in
      float64 and truncates directly.
    ValueError where the reference's cast is undefined: NaN or inf in the magnitude, a negative or non-finite echo value."""
    field = np.asarray(field)
    if field.dtype != np.float32 or field.ndim != 4 or field.shape[3] != 2 or min(field.shape) < 1:
        raise ValueError(f"field must be float32 [N,H,W,2] with no empty side, got {field.dtype} {field.shape}")
    N, H, W, _ = field.shape
    n = int(n_used)
    if not 1 <= n <= N:
        raise ValueError(f"n_used must be in [1, {N}], got {n_used}")
    lut = _check_lut(lut, "lut")
    echo = np.asarray(echo)
    if echo.dtype not in (np.float16, np.uint8):
        raise ValueError(f"echo must be float16 or uint8, got {echo.dtype}")
    if echo.ndim != 3 or echo.shape[0] < n or echo.shape[1:] != (H, W):
        raise ValueError(f"echo must be [>= {n},{H},{W}], got shape {echo.shape}")
    echo = echo[:n]
    if echo.dtype == np.float16 and not (np.isfinite(echo).all() and (echo >= 0).all()):
        raise ValueError("the echo holds a negative or non-finite value")
    if norm_f64 is None:
        norm_f64 = norm_is_f64()
    vmin, vmax = np.float32(np.inf), np.float32(-np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(N):                                          # frame by frame: the float32 temporaries stay one frame large
            m = _magnitude(field[i])
            if not np.isfinite(m).all():
                raise ValueError("the magnitude holds NaN or inf")
            vmin, vmax = min(vmin, m.min()), max(vmax, m.max())
    out = np.empty((n, H, W, 3), np.uint8)
    frame_info = np.zeros((n, 2), np.float64)
    for i in range(n):
        _, idx = magnitude_norm_index(_magnitude(field[i]), vmin, vmax, norm_f64)
        cmax = lut[np.bincount(idx.ravel(), minlength=256) > 0].max()
        col = 0.5 * (lut / cmax if cmax > 0 else lut)
        emax = np.max(echo[i])
        pn = echo[i] / emax if emax > 0 else echo[i]                 # float16 / float16 stays float16; uint8 / uint8 is float64
        v = ((0.5 * pn).astype(np.float64)[..., None] + col[idx]) * 255   # 0.5 * float16 stays float16
        out[i] = (v.astype(np.float16) if echo.dtype == np.float16 else v).astype(np.uint8)
        frame_info[i] = emax, cmax
    return out, np.array([vmin, vmax], np.float64), frame_info


def magnitude_overlay(ds, param, label, colormap="hot", *, engine=None, norm_f64=None, return_info=False):
    """The frames the reference's example hands to the writer of its single-component video (example_peak_plots.py:459-513): uint8
    [ds.nframes,H,W,3], the magnitude of get_masked_arr(param, label) through `colormap`, blended half and half with the echo image;
    or None (logged) for an unknown param or label, mode 'otsu' or a study without echo, the reference's own refusals.  `colormap` is
    a name (magnitude_colormap_lut; the reference's is 'hot') or a [256,3] table.  `ds` is the reference's OpticalFlowDataset, a
    FlowStudy or a HeldStudy; the field and the norm's range are over all the frames the file stores (nframes + 2), the frames
    rendered are the first ds.nframes.  norm_f64 chooses the norm's division rule (magnitude_norm_index); None takes this process's
    numpy's (norm_is_f64).  Without `engine`, numpy (magnitude_overlay_host); with `engine` (a DenseFlow) everything per pixel runs on
    the device (tf_magnitude_overlay) and only the frames come back; the resident planes of the engine's last projection stay as they
    are.  Both give the same bytes, and both raise ValueError for NaN or inf in the magnitude and for a negative or non-finite echo
    value.  return_info adds (vmin, vmax) and the per-frame (echo max, colour max) as second and third results."""
    if not _valid(ds, param, label):
        return None
    if ds.mode == "otsu":
        log.error("the magnitude overlay is not supported for mode='otsu'")
        return None
    tail = _tail(ds, engine)
    n = int(ds.nframes)
    if tail is not None and tail.held:
        echo = None
        if ds.n_echo < 1:
            log.error("the study has no echo frames: no magnitude overlay")
            return None
        if ds.n_echo < n:
            raise ValueError(f"echo must be [>= {n},{ds.shape[1]},{ds.shape[2]}], the held one has {ds.n_echo} frames")
    else:
        echo = ds.get_echo()
        if echo is None:
            log.error("the study has no echo frames: no magnitude overlay")
            return None
        echo = np.asarray(echo)
        if echo.dtype not in (np.float16, np.uint8):
            raise ValueError(f"echo must be float16 (the study file's) or uint8, got {echo.dtype}")
    lut = _check_lut(magnitude_colormap_lut(colormap) if isinstance(colormap, str) else colormap, "colormap")
    if norm_f64 is None:
        norm_f64 = norm_is_f64()
    if tail is None:
        flow, mask = _study_arrays(ds, label)
        N = np.shape(flow)[0]
        if np.shape(mask)[0] < N:
            raise ValueError(f"the {label!r} mask has {np.shape(mask)[0]} frames, fewer than the flow's {N} (the norm's range is over every frame)")
        res = magnitude_overlay_host(param_field(flow, mask, param, ds.frame_rate, N), n, echo, lut, norm_f64)
    else:
        res = _device_overlay(lambda: tail.magnitude_overlay(param, label, n, echo, lut, norm_f64))
    return res if return_info else res[0]


def visualize_magnitude(ds, param, label, save_dir, fps=30, colormap="hot", *, engine=None, norm_f64=None, writer_factory=None):
    """The single-component video of the reference's example (example_peak_plots.py:469-513): renders magnitude_overlay's frames and
    writes them to <save_dir>/<stem>_<label>_<param>_single_overlay.mp4, one append_data call per frame, then close.  <stem> is
    ds.filename less one trailing dot: OpticalFlowDataset's filename of an .hdf5 file keeps the dot of the extension, the example's
    name does not.  Returns the path, or None under magnitude_overlay's refusals (nothing is written then).  writer_factory(path,
    fps=) makes the writer; the default is imageio.v2.get_writer, imported when needed.  The encoding itself is the writer's."""
    frames = magnitude_overlay(ds, param, label, colormap, engine=engine, norm_f64=norm_f64)
    if frames is None:
        return None
    if writer_factory is None:
        import imageio.v2 as iio
        writer_factory = iio.get_writer
    os.makedirs(save_dir, exist_ok=True)
    stem = ds.filename[:-1] if ds.filename.endswith(".") else ds.filename
    save_path = os.path.join(save_dir, f"{stem}_{label}_{param}_single_overlay.mp4")
    writer = writer_factory(save_path, fps=fps)
    for i in range(frames.shape[0]):
        writer.append_data(frames[i])
    writer.close()
    return save_path
