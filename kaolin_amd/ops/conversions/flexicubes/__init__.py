from .flexicubes import *  # noqa: F401,F403
from .flexicubes import __all__  # noqa: F401
