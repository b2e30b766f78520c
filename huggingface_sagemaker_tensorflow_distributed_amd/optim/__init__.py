from .adam import FusedAdam
from .lamb import FusedLamb

__all__ = ["FusedAdam", "FusedLamb"]
