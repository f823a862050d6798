from .att_equiunet import AttEquiUnet  # noqa: F401
from .attgate import AttentionBlock  # noqa: F401
from .attunet import AttUnet, R2AttUnet  # noqa: F401
from .cbam import CBAM  # noqa: F401
from .equiunet import EquiUnet  # noqa: F401
from .r2unet import R2Unet  # noqa: F401
from .rrcnn import RRCNNblock  # noqa: F401
from .unet import Unet  # noqa: F401
