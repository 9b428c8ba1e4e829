"""Data path (reference: data/dataset.py:15-62 `BaseDataset`); DeviceLoader feeds its batches from HBM;
CutMix / CutOut (reference: data/augmentations.py, data/__init__.py) on the box-mix kernel; the similarity transforms (flip /
rotation, same file of the reference) on the affine-warp kernel; the photometric strong augmentation (colour jitter, grayscale, blur:
no reference counterpart) on the photometric kernel; SyntheticCropWeed: seeded blobs where no dataset is at hand."""
from .dataset import BaseDataset, write_synthetic_dataset  # noqa: F401
from .device_loader import DeviceLoader, f32_table, label_table  # noqa: F401
from .augmentations import CutMix, CutOut, aug_dict, augmentation, draw_box, make_aug, make_cutout_mask  # noqa: F401
from .augmentations import (inverse_similarity_transform, similarity_matrices, similarity_transform, step_transforms,  # noqa: F401
                            warp_batch)
from .augmentations import (IDENTITY_PHOTOMETRIC, StrongPhotometric, draw_photometric, photometric, photometric_taps,  # noqa: F401
                            step_photometric)
from .synthetic import SyntheticCropWeed  # noqa: F401
