"""``kaolin.rep``: data classes.  Only ``Spc``, the structured point cloud, is part of this package."""
from .spc import Spc  # noqa: F401

__all__ = ['Spc']
