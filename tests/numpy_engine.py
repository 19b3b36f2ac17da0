"""A DenseFlow's tail protocol in numpy, for the CPU tests of analysis.py's engine glue (tests/test_analysis_glue_cpu.py): the five
host-pointer calls, their held_* forms, hold_study / hold_mask / held, and radlong_project / radlong_hist / radlong_select.  Every step is
one of the package's own host twins, so an analysis function given this engine can differ from the same function without an engine
only through its glue: percentile ranks, _lerp, the edge rules, the refusals, the carry-over quirks.  The histogram is the device's rule
(stats_cases.device_hist_rule) and the select the device's radix walk (stats_cases.select_model), over the planes the last projection
left.  A helper module: nothing here is collected."""
import numpy as np

from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.dense_flow import HeldShape

from tests.stats_cases import device_hist_rule, select_model


class _Rate:
    """the frame rate of a spacing: 1 / _Rate(spacing) is `spacing` itself, its type and bits, as param_field divides"""

    def __init__(self, spacing):
        self.spacing = spacing

    def __rtruediv__(self, one):
        return self.spacing


class NumpyEngine:
    def __init__(self):
        self.calls = []                                       # the names of the public calls taken, in order
        self.planes = None                                    # the last projection's two planes, float64 [n,H,W]
        self.flow = self.echo = None                          # the held study
        self.masks, self.generation = {}, 0

    # ---- the steps, shared by both forms ---------------------------------------------------------------------------------------------
    @staticmethod
    def _centroids(masks):
        found = [A._largest_component(m[:, :, 0]) for m in np.asarray(masks)]
        cent = np.array([f[0] if f else (0.0, 0.0) for f in found], np.float64).reshape(len(found), 2)
        return cent, np.array([f[1] if f else 0 for f in found], np.int64)

    @staticmethod
    def _areas(masks):
        return np.array([A._first_region_area(m[:, :, 0]) or 0 for m in np.asarray(masks)], np.int64)

    @staticmethod
    def _rate(spacing, grad_f64):
        """numpy divides the gradient in float64 for a np.float64 spacing and in float32 for a Python float: grad_f64 says which"""
        return _Rate(np.float64(spacing) if grad_f64 else float(spacing))

    def _radlong(self, flow, mask, param, spacing, grad_f64, n_used, centroids, return_arrays):
        field = A.param_field(flow, mask, A.PARAMS[param], self._rate(spacing, grad_f64), n_used)
        return self._project(field, centroids, return_arrays)

    def _project(self, field, centroids, return_arrays):
        rad, lon = A.calculate_comp_magnitude(field, np.asarray(centroids, np.float64).reshape(-1, 2))
        self.planes = (rad, lon)
        mm = np.array([rad.min(), rad.max(), lon.min(), lon.max()], np.float64)
        nz = np.stack([(rad != 0).sum((1, 2)), (lon != 0).sum((1, 2))], 1).astype(np.int64)
        return (mm, nz, rad, lon) if return_arrays else (mm, nz, None, None)

    def _polar(self, flow, mask, param, spacing, grad_f64, n_used, return_arrays):
        mag, ang = A.polar_field(flow, mask, A.PARAMS[param], self._rate(spacing, grad_f64), n_used)
        self.planes = (mag.astype(np.float64), ang.astype(np.float64))
        mm = np.array([mag.min(), mag.max(), ang.min(), ang.max()], np.float32)
        nz = np.stack([(mag != 0).sum((1, 2)), (ang != 0).sum((1, 2))], 1).astype(np.int64)
        mode = np.asarray([A._mode_of_rounded(a) for a in ang], np.float32)
        return (mm, nz, mode, mag, ang) if return_arrays else (mm, nz, mode, None, None)

    def _overlay(self, echo, lut_rad, lut_long):
        return A.overlay_host(self.planes[0], self.planes[1], echo, lut_rad, lut_long)

    # ---- the host-pointer calls ------------------------------------------------------------------------------------------------------
    def av_centroids(self, masks):
        self.calls.append("av_centroids")
        return self._centroids(masks)

    def first_region_areas(self, masks):
        self.calls.append("first_region_areas")
        return self._areas(masks)

    def radlong_project_param(self, flow, mask, param, spacing, grad_f64, n_used, centroids, return_arrays=False):
        self.calls.append("radlong_project_param")
        return self._radlong(flow, mask, param, spacing, grad_f64, n_used, centroids, return_arrays)

    def polar_project_param(self, flow, mask, param, spacing, grad_f64, n_used, return_arrays=False):
        self.calls.append("polar_project_param")
        return self._polar(flow, mask, param, spacing, grad_f64, n_used, return_arrays)

    def radlong_overlay(self, echo, lut_rad, lut_long):
        self.calls.append("radlong_overlay")
        return self._overlay(echo, lut_rad, lut_long)

    # ---- the held study: the arrays kept here ----------------------------------------------------------------------------------------
    def hold_study(self, flow16, echo16=None):
        self.calls.append("hold_study")
        self.flow, self.echo = np.asarray(flow16), None if echo16 is None else np.asarray(echo16)
        self.masks, self.generation = {}, self.generation + 1
        return self.held

    def hold_mask(self, label, mask):
        self.calls.append("hold_mask")
        self.masks[label] = np.asarray(mask)

    @property
    def held(self):
        if self.flow is None:
            return None
        N, H, W, _ = self.flow.shape
        return HeldShape(N, H, W, 0 if self.echo is None else len(self.echo), self.generation,
                         {k: (m.shape[0], m.shape[3]) for k, m in self.masks.items()})

    def held_av_centroids(self, label, n):
        self.calls.append("held_av_centroids")
        return self._centroids(self.masks[label][:n])

    def held_first_region_areas(self, label, n):
        self.calls.append("held_first_region_areas")
        return self._areas(self.masks[label][:n])

    def held_radlong_project_param(self, label, param, spacing, grad_f64, n_used, centroids, return_arrays=False):
        self.calls.append("held_radlong_project_param")
        return self._radlong(self.flow, self.masks[label], param, spacing, grad_f64, n_used, centroids, return_arrays)

    def held_polar_project_param(self, label, param, spacing, grad_f64, n_used, return_arrays=False):
        self.calls.append("held_polar_project_param")
        return self._polar(self.flow, self.masks[label], param, spacing, grad_f64, n_used, return_arrays)

    def held_radlong_overlay(self, lut_rad, lut_long):
        self.calls.append("held_radlong_overlay")
        return self._overlay(self.echo, lut_rad, lut_long)

    # ---- the statistics of the resident planes ---------------------------------------------------------------------------------------
    def radlong_project(self, flow, centroids, return_arrays=False):
        self.calls.append("radlong_project")
        return self._project(np.asarray(flow, np.float32)[:len(centroids)], centroids, return_arrays)

    def radlong_hist(self, which, edges, n_frames):
        self.calls.append("radlong_hist")
        assert n_frames == len(self.planes[which]) and np.asarray(edges).dtype == np.float64
        return np.stack([device_hist_rule(p.ravel(), edges) for p in self.planes[which]]).astype(np.int64)

    def radlong_select(self, which, ranks):
        self.calls.append("radlong_select")
        ranks = np.asarray(ranks)
        assert ranks.shape == (len(self.planes[which]), 4) and ranks.dtype == np.int64
        vals = np.zeros(ranks.shape, np.float64)
        for i, j in zip(*np.nonzero(ranks >= 0)):
            vals[i, j] = select_model(self.planes[which][i], ranks[i, j])
        return vals
