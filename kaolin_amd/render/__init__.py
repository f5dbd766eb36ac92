from . import camera  # noqa: F401
from . import mesh  # noqa: F401
from . import lighting  # noqa: F401
from . import spc  # noqa: F401
