from .hat_model import HATModel  # noqa: F401

# `model_type` of an option file -> the test-time harness.  ESC's ESRModel.test (ESC/esc/models/esr_model.py:269-310) is HATModel's:
# reflect-pad to network_g.window_size, run, crop — the test branch is all that is built (training is out of scope).
# ESRGANModel / SRGANModel / RealESRGANModel validate as SRModel does (esrgan_model.py, realesrgan_model.py): their own parts are training.
MODEL_TYPES = {"HATModel": HATModel, "ESRModel": HATModel, "SRModel": HATModel, "RealESRNetModel": HATModel,
               "ESRGANModel": HATModel, "SRGANModel": HATModel, "RealESRGANModel": HATModel}


def model_class(model_type):
    """The harness class of an option file's `model_type` (None: HATModel); KeyError for a model type that is not built."""
    if model_type is None:
        return HATModel
    try:
        return MODEL_TYPES[model_type]
    except KeyError:
        raise KeyError(f"model_type {model_type!r} is not built: {', '.join(sorted(MODEL_TYPES))}") from None
