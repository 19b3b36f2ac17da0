"""radial / longitudinal projection of the flow and the per-frame percentile / histogram curves.

Mirrors /root/reference/optical_flow/analysis.py:
  :122-134  calc_proj_mag,  :137-163 calculate_comp_magnitude (with radial_vecgrid :89-119)   -> calculate_comp_magnitude
  :166-212  calc_bidirectional_hist                                                          -> calc_bidirectional_hist
Two implementations with identical results: a vectorised numpy one (host) and a device one that keeps the projections in
HBM and gets the histogram and the exact order statistics np.percentile interpolates between from HIP kernels
(include/teeflow.h: tf_radlong_project / _hist / _select).  Pinned by tests/golden/reference_analysis.npz, which the
reference's own functions produced.

The steps before the projection are here too, so that the consumer's call runs whole (/root/reference/optical_flow/analyze_optical_flow.py):
  :202-244  calc_AV_centroid (8-connected labelling, largest region, Savitzky-Golay)                  -> av_centroids
  :320-343  calculate_3dhist_radlong(ds, param) with OpticalFlowDataset's param field
            (optical_flow_dataset.py:57, 100-101, 182-228: velocity, np.gradient acceleration, PWR, x rv mask) -> calculate_3dhist_radlong
With engine= the labelling (tf_av_centroids) and the param field fused into the projection (tf_radlong_project_param) run on the device;
without, a numpy/scipy twin gives the same bits.  Pinned by tests/golden/reference_study_stats.npz (the reference's own functions on a
study file opened by its own OpticalFlowDataset).
"""
import ctypes as C
import logging

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
    """numpy's percentile interpolation (numpy/lib/_function_base_impl.py::_lerp) for scalars."""
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def radlong_stats_device(engine, OF_arr, centroid_list, perc_lo=1, perc_hi=99, nbins=1000, return_arrays=False):
    """{'radial': (freq, edges[:-1], hi, lo), 'longitudinal': (...)} as calculate_3dhist_radlong (:289-327) returns after its
    centroid step, computed on the device behind `engine` (a DenseFlow).  return_arrays adds 'rad_arr' / 'long_arr'."""
    L = engine._L
    n = len(centroid_list)
    OF = np.ascontiguousarray(np.asarray(OF_arr)[:n], dtype=np.float32)
    N, H, W, _ = OF.shape
    cent = np.ascontiguousarray(centroid_list, dtype=np.float64).reshape(N, 2)
    rad = np.empty((N, H, W), np.float64) if return_arrays else None
    lon = np.empty((N, H, W), np.float64) if return_arrays else None
    mm = np.zeros(4, np.float64)
    nz = np.zeros(2 * N, np.int64)
    _lib.check(L.tf_radlong_project(engine._h, OF.ctypes.data, cent.ctypes.data, N, H, W, rad.ctypes.data if return_arrays else None,
                                    lon.ctypes.data if return_arrays else None, mm.ctypes.data, nz.ctypes.data), engine._h, "tf_radlong_project")
    return _radlong_stats_resident(engine, N, mm, nz, perc_lo, perc_hi, nbins, rad, lon)


def _radlong_stats_resident(engine, N, mm, nz, perc_lo, perc_hi, nbins, rad=None, lon=None):
    """The statistics of the projections resident on the device after tf_radlong_project(_param): per frame histogram, the exact
    order statistics np.percentile interpolates between, and the reference's per-frame loop.  mm / nz as the projection returned."""
    L = engine._L
    nz = np.asarray(nz).reshape(-1)
    out = {}
    for which, name in ((0, "radial"), (1, "longitudinal")):
        mn, mx = mm[2 * which], mm[2 * which + 1]
        cnt = nz[which::2]
        first, last = (mn, mx) if mn != mx else (mn - 0.5, mx + 0.5)          # np.histogram's degenerate-range rule
        edges = np.linspace(first, last, nbins + 1)
        freq = np.zeros((N, nbins), np.int64)
        _lib.check(L.tf_radlong_hist(engine._h, which, edges.ctypes.data, nbins, freq.ctypes.data), engine._h, "tf_radlong_hist")
        ranks = np.full((N, 4), -1, np.int64)
        frac = np.zeros((N, 2))
        for i in range(N):
            if cnt[i] > 0:
                for j, q in enumerate((perc_hi, perc_lo)):
                    vi = (cnt[i] - 1) * np.true_divide(q, 100)
                    lo_i = int(np.floor(vi))
                    ranks[i, 2 * j] = lo_i
                    ranks[i, 2 * j + 1] = min(lo_i + 1, cnt[i] - 1)
                    frac[i, j] = vi - lo_i
        vals = np.zeros((N, 4), np.float64)
        _lib.check(L.tf_radlong_select(engine._h, which, ranks.ctypes.data, vals.ctypes.data), engine._h, "tf_radlong_select")
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
    returned unfiltered).  With `engine` (a DenseFlow) the labelling runs on the device (tf_av_centroids), with the same bits."""
    nframes = int(nframes)
    shape = np.shape(mask_arr)
    if len(shape) != 4:
        raise ValueError(f"mask_arr must be [N,H,W,C], got shape {shape}")
    if nframes > shape[0]:
        raise IndexError(f"nframes {nframes} > {shape[0]} mask frames")
    if nframes > 0 and engine is not None:
        masks = np.asarray(mask_arr)[:nframes]
        if masks.dtype not in (np.bool_, np.uint8) or masks.shape[3] not in (1, 2):
            masks = np.ascontiguousarray(masks[..., :1] != 0)
        cent, area = engine.av_centroids(masks)
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
    if len(centroid_list) != n_used:
        raise ValueError(f"{len(centroid_list)} centroids for {n_used} frames")
    if engine is None:
        rad, lon = calculate_comp_magnitude(param_field(flow, mask, param, frame_rate, n_used), centroid_list)
        out = {}
        for name, arr in (("radial", rad), ("longitudinal", lon)):
            f, e, hi, lo = calc_bidirectional_hist(arr, n_used, perc_lo=perc_lo, perc_hi=perc_hi, nbins=nbins)
            out[name] = (f, np.asarray(e)[:-1], hi, lo)
        if return_arrays:
            out["rad_arr"], out["long_arr"] = rad, lon
        return out
    mask = np.asarray(mask)
    if mask.dtype not in (np.bool_, np.uint8):
        raise ValueError(f"the device path takes a bool or uint8 mask (the study file's), got {mask.dtype}")
    mm, nz, rad, lon = engine.radlong_project_param(flow, mask, PARAMS.index(param), 1 / frame_rate, gradient_is_f64(frame_rate), n_used,
                                                    centroid_list, return_arrays=return_arrays)
    return _radlong_stats_resident(engine, n_used, mm, nz, perc_lo, perc_hi, nbins, rad, lon)


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
    flow = getattr(ds, "flow", None)
    if flow is None:
        flow = ds.vel_array
    if centroids is None:
        centroids = av_centroids(ds.get_mask("av"), ds.nframes, filter=av_filter_flag, savgol_window=av_savgol_window,
                                 savgol_poly=av_savgol_poly, engine=engine)
    return param_radlong_stats(flow, ds.get_mask("rv"), param, ds.frame_rate, ds.nframes, centroids, perc_lo=perc_lo, perc_hi=perc_hi,
                               nbins=nbins, engine=engine)


class FlowStudy:
    """What calculate_3dhist_radlong reads of a study, built from arrays: flow [N,H,W,2] as given (float16 as the study file holds
    it: the device upload is then 2 bytes per component), masks {label: [N,H,W,C]}, frame_rate, nframes (default N - 2, as
    OpticalFlowDataset reads attrs['nframes'] - 2 of a file whose flow has attrs['nframes'] frames), mode."""

    def __init__(self, flow, masks, frame_rate, nframes=None, mode="RVIO_2class"):
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
            return cls(flow, masks, frame_rate, nframes=a["nframes"] - 2, mode=a["mode"])
