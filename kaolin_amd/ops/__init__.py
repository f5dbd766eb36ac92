from . import mesh  # noqa: F401
from . import conversions  # noqa: F401
from . import voxelgrid  # noqa: F401
from . import spc  # noqa: F401
from . import random  # noqa: F401
from . import gaussians  # noqa: F401
from . import gaussian  # noqa: F401
