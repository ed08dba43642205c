from .augment import PairAugment
from .datasets import (ImagePairDataset, PFPascalDataset, SingleImageDataset, SyntheticCorrespondenceDataset,
                       SyntheticImageDataset, SyntheticPairDataset, synthetic_batch)
from .transforms import AffineTnf, NormalizeImageDict, normalize_image, resize_bilinear

__all__ = ["PairAugment", "ImagePairDataset", "PFPascalDataset", "SingleImageDataset", "SyntheticCorrespondenceDataset",
           "SyntheticImageDataset", "SyntheticPairDataset", "synthetic_batch", "AffineTnf", "NormalizeImageDict",
           "normalize_image", "resize_bilinear"]
