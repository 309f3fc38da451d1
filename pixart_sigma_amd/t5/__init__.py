"""The T5 v1.1 text encoder on HIP: prompts to the (B, L, 4096) caption features the denoiser consumes (reference diffusion/model/t5.py)."""
from .embedder import T5Embedder  # noqa: F401
from .encoder import MAX_LENGTH, T5Config, T5Encoder, key_lengths, relative_position_bucket  # noqa: F401
