"""Instance-level validation metrics on the MI355X (reference: skoots/validate/lib.py)."""
from .lib import (accuracies_from_iou, f1_score, get_segmentation_errors, label_soft_skeleton, mask_dice,  # noqa: F401
                  mask_iou, mask_metrics, mask_soft_cldice, mask_to_bbox)
