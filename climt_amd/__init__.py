"""climt_amd -- MI355X-native RRTMG longwave + shortwave radiation, drop-in for
climt.RRTMGLongwave / climt.RRTMGShortwave (climt/_components/rrtmg/__init__.py:1-4), plus the zenith-angle producer
upstream of the shortwave, climt.Instellation and climt.BergerSolarInsolation, and the consumer of the surface
fluxes downstream, climt.SlabSurface, and climt.DryConvectiveAdjustment, climt.SimpleBoundaryLayer and climt.EmanuelConvection behind them; the gray radiation path beside the RRTMG one
(climt.GrayLongwaveRadiation, climt.Frierson06LongwaveOpticalDepth, climt.GridScaleCondensation); and what a model script needs to set the path up: get_grid / get_default_state
(climt/_core/initialization.py), UpdateFrequencyWrapper and the AdamsBashforth tendency stepper."""
import os as _os

# The shortwave and the longwave run on two HIP streams of one context, and a communicator adds a third.  The HIP runtime
# deals streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); with another library's streams in the process (torch's
# RCCL process group creates several) the two can land on ONE queue and run back to back: measured 2.00 instead of 1.76 ms
# per step.  Eight queues keep them apart.  Read by the runtime when it initialises, so it has to be in the
# environment before the first HIP call of the process; a value the user set is left alone.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from ._lib import Context, RRTMGError  # noqa: F401,E402
from .berger import BergerSolarInsolation  # noqa: F401,E402
from .device_state import DeviceAdamsBashforth, DeviceQuantity, DeviceState  # noqa: F401,E402
from .dry_convection import DryConvectiveAdjustment  # noqa: F401,E402
from .initialization import get_default_state, get_grid  # noqa: F401,E402
from .instellation import Instellation  # noqa: F401,E402
from .rrtmg import RRTMGLongwave, RRTMGShortwave, radiation_step  # noqa: F401,E402
from .simple_boundary_layer import SimpleBoundaryLayer  # noqa: F401,E402
from .simple_physics import SimplePhysics  # noqa: F401,E402
from .gray_radiation import Frierson06LongwaveOpticalDepth, GrayLongwaveRadiation  # noqa: F401,E402
from .cork import CorkLongwaveRadiation, CorkShortwaveRadiation  # noqa: F401,E402
from .grid_scale_condensation import GridScaleCondensation  # noqa: F401,E402
from .surface_ice import LandIce, SeaIce  # noqa: F401,E402
from .bucket_hydrology import BucketHydrology  # noqa: F401,E402
from .second_best import (BestSoilProperties, BestSubsurfaceTransport, BestSurfaceAlbedo, BestSurfaceFluxes, BestSurfaceLayer,  # noqa: F401,E402
                          SecondBEST)
from .emanuel import EmanuelConvection  # noqa: F401,E402
from .slab_surface import SlabSurface  # noqa: F401,E402
from .timestepping import AdamsBashforth  # noqa: F401,E402
from .wrappers import UpdateFrequencyWrapper  # noqa: F401,E402
from .intermittent import IntermittentLongwave, IntermittentShortwave  # noqa: F401,E402

__all__ = ["RRTMGLongwave", "RRTMGShortwave", "Instellation", "BergerSolarInsolation", "SlabSurface", "DryConvectiveAdjustment", "SimpleBoundaryLayer", "EmanuelConvection", "SimplePhysics", "GrayLongwaveRadiation", "Frierson06LongwaveOpticalDepth", "GridScaleCondensation", "CorkLongwaveRadiation", "CorkShortwaveRadiation", "SeaIce", "LandIce", "BucketHydrology", "SecondBEST", "BestSoilProperties", "BestSurfaceAlbedo", "BestSurfaceLayer", "BestSurfaceFluxes", "BestSubsurfaceTransport", "get_grid", "get_default_state", "UpdateFrequencyWrapper", "IntermittentShortwave", "IntermittentLongwave", "AdamsBashforth",
           "Context", "RRTMGError", "DeviceState", "DeviceQuantity", "DeviceAdamsBashforth", "radiation_step"]
