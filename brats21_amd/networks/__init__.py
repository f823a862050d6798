from .cbam import CBAM  # noqa: F401
from .equiunet import EquiUnet  # noqa: F401
