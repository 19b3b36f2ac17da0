"""tests/numpy_engine.NumpyEngine with the magnitude overlay's two protocol methods, on the package's host twin: an analysis function given
this engine can differ from the same function without an engine only through its glue.  A helper module: nothing here is collected."""
import numpy as np

from tee_optical_flow_amd import analysis as A

from tests.numpy_engine import NumpyEngine


class MagnitudeNumpyEngine(NumpyEngine):
    def _magnitude(self, flow, mask, param, spacing, grad_f64, norm_f64, n_used, echo, lut):
        N = np.shape(flow)[0]
        field = A.param_field(flow, mask, A.PARAMS[param], self._rate(spacing, grad_f64), N)
        return A.magnitude_overlay_host(field, n_used, echo, lut, bool(norm_f64))

    def magnitude_overlay(self, flow, mask, param, spacing, grad_f64, norm_f64, n_used, echo, lut):
        self.calls.append("magnitude_overlay")
        return self._magnitude(flow, mask, param, spacing, grad_f64, norm_f64, n_used, echo, lut)

    def held_magnitude_overlay(self, label, param, spacing, grad_f64, norm_f64, n_used, lut):
        self.calls.append("held_magnitude_overlay")
        return self._magnitude(self.flow, self.masks[label], param, spacing, grad_f64, norm_f64, n_used, self.echo, lut)
