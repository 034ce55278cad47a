from .longwave import RRTMGLongwave
from .shortwave import RRTMGShortwave, band_albedo

__all__ = ("RRTMGShortwave", "RRTMGLongwave", "band_albedo")
