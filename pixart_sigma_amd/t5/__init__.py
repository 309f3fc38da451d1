"""The T5 v1.1 text encoder on HIP: prompts to the (B, L, 4096) caption features the denoiser consumes (reference diffusion/model/t5.py)."""
from .embedder import T5Embedder  # noqa: F401
from .encoder import MAX_LENGTH, T5Config, T5Encoder, key_lengths, relative_position_bucket  # noqa: F401


def __getattr__(name):
    """CaptionEncoder on first use: captions.py is also the program of its worker process (python -m pixart_sigma_amd.t5.captions), which this package
    must not have imported before it runs."""
    if name in ("CaptionEncoder", "CaptionWorkerError"):
        from . import captions
        return getattr(captions, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
