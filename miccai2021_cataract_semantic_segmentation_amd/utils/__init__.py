from .classes import CADIS_PALETTE, CATEGORIES, CLASS_REMAP, IGNORE_LABEL, NUM_CLASSES, ce_ignore_index, num_classes  # noqa: F401
from .augment import (GpuAugment, check_randaugment, gaussian_box_params, pseudo_jitter_ranges, pseudo_jitter_strength,  # noqa: F401
                      randaugment_from_transforms, randaugment_space, sample_blur, sample_color_jitter, sample_randaugment)
from .ingest import GpuIngest, check_label_tables, label_tables_of, remap_lut, sample_flips  # noqa: F401
from .semi import BalancedConcatDataset  # noqa: F401
from .geometry import (affine_inverse, class_frequencies, crop_freq_region, crop_px, freq_weight_table, geometry_from_transforms,  # noqa: F401
                       sample_affine, sample_crops, sample_freq_u)
from .egress import (GpuEgress, clipped_argmax, get_cadis_colormap, get_remapped_colormap, mask_from_network, mask_to_colormap,  # noqa: F401
                     network_lut, palette_table, to_comb_image)
from .lr_functions import LRFcts  # noqa: F401
from .sampling import RepeatFactorSampler, class_repeat_factors, image_repeat_factors  # noqa: F401
from .census import IoUTracker, class_info, class_sums_of, label_census, presence_of  # noqa: F401
from .class_sampling import (OVERSAMPLING_PRESETS, AdaptiveBatchSampler, ShuffledIndexList, oversampled_indices, train_schedule,  # noqa: F401
                             weighted_random_weights)


def __getattr__(name):  # metrics need the HIP library: import lazily so CPU-only tooling can use the rest
    if name in ("t_get_confusion_matrix", "t_get_pixel_accuracy", "t_get_miou", "t_get_mean_iou", "t_normalise_confusion_matrix"):
        from . import metrics
        return getattr(metrics, name)
    if name == "PinnedFrameLoader":
        from .loader import PinnedFrameLoader
        return PinnedFrameLoader
    raise AttributeError(name)
