"""Scoring modules with the reference's module path and names (modules/front_back_end.py, modules/loss.py), on libmst_hip.so's fused
multi-scale spectral kernels (csrc/mss_kernels.h): forward only, except MultiScale_Spectral_Loss_MidSide_DDSP(differentiable=True), whose value
carries its gradient with respect to the estimate (mst_mss_backward)."""
from .front_back_end import BackEnd, FrontEnd  # noqa: F401
from .loss import MultiScale_Spectral_Loss_MidSide_DDSP  # noqa: F401
