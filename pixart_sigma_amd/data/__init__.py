"""Callers' side of the hot path: batch formation for multi-aspect training."""
from .sampler import AspectRatioBatchSampler, closest_ratio  # noqa: F401
from .features import FeatureDatasetMS, vae_feat_loader  # noqa: F401,E402
from .images import ImagePreprocessor, resample_tables, save_png, transform_geometry  # noqa: F401,E402
from .pictures import PictureCaptionDataset, PictureCaptionDatasetMS, load_ratio_table  # noqa: F401,E402
from .pipeline import PictureBatches  # noqa: F401,E402
