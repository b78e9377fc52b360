"""Scoring modules with the reference's module path and names (modules/front_back_end.py, modules/loss.py), forward only, on
libmst_hip.so's fused multi-scale spectral kernel (csrc/mss_kernels.h)."""
from .front_back_end import BackEnd, FrontEnd  # noqa: F401
from .loss import MultiScale_Spectral_Loss_MidSide_DDSP  # noqa: F401
