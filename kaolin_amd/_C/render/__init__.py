from . import mesh  # noqa: F401
from . import sg  # noqa: F401
from . import spc  # noqa: F401
