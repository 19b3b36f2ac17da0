"""The four kernel forms of DualTVL1's inner iteration and the tuning knobs that select each, for the GPU tests that run a case in a
chosen form.  A form is named, or given by its index in FORMS (the tests' `variant` / `form` parameters 0..3)."""
import contextlib

FORMS = ("tiles", "strips", "strips2", "tiles2")
KNOBS = {
    "tiles": {"iter_variant": 0, "min_rows_work": 0},            # k_iter: 64x16 tiles, one iteration per launch
    "strips": {"iter_variant": 1, "min_rows_work": 0},           # k_iter_rows: full-width row strips, however small the launch
    "strips2": {"iter_variant": 2, "min_rows_work": 0},          # k_iter2_rows: strips, two iterations per launch
    "tiles2": {"iter_variant": 2, "min_rows_work": 1 << 30},     # k_iter2_tile: no launch is large enough for the strips
}
DEFAULT_ITER_KNOBS = {"iter_variant": 2, "min_rows_work": 8192}


@contextlib.contextmanager
def iter_form(engine, form):
    """Run the block with `engine` set to `form`; the engine has its default knobs again afterwards.  (An odd iteration count takes
    the two-per-launch forms' one-per-launch kernels, as in a solve.)"""
    for name, v in KNOBS[FORMS[form] if isinstance(form, int) else form].items():
        engine.set_tuning(name, v)
    try:
        yield engine
    finally:
        for name, v in DEFAULT_ITER_KNOBS.items():
            engine.set_tuning(name, v)
