from .joint import radiation_step
from .longwave import RRTMGLongwave
from .shortwave import RRTMGShortwave, band_albedo

__all__ = ("RRTMGShortwave", "RRTMGLongwave", "band_albedo", "radiation_step")
