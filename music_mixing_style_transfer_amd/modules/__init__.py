"""Scoring and training objectives with the reference's module path and names (modules/front_back_end.py, modules/loss.py), on
libmst_hip.so's kernels: the fused multi-scale spectral kernels (csrc/mss_kernels.h) and the contrastive / gain losses
(csrc/contrast_kernels.h).  Forward only by default; an instance built with differentiable=True carries its gradient
(mst_mss_backward, mst_ntxent_backward, mst_rms_loss_backward), and `Loss` - the trainer's container - builds its members that way."""
from .front_back_end import BackEnd, FrontEnd  # noqa: F401
from .loss import Loss, MultiScale_Spectral_Loss_MidSide_DDSP, NT_Xent, RMSLoss, infoNCE  # noqa: F401
