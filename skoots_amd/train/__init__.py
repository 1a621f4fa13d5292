"""Config-5 training step on the HIP kernels (reference: skoots/train/)."""
from .engine import TrainUNet, TrainStep, fused_loss, sync_gradients, train_step  # noqa: F401
from .generate_skeletons import calculate_skeletons, create_gt_skeletons  # noqa: F401
from .loss import LOSS_FUNCTIONS, loss_from_cfg, soft_dice_cldice, soft_skeletonize, tversky  # noqa: F401
from .sigma import Sigma, init_sigma  # noqa: F401
from .transforms import AugmentPlan, TransformFromCfg, draw_plan, skeleton_colate  # noqa: F401
from .dataloader import MultiDataset, dataset  # noqa: F401
from .schedule import cosine_annealing_warm_restarts  # noqa: F401
from .trainer import Batches, run_training, train  # noqa: F401
