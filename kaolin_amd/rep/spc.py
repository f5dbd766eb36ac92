"""``kaolin.rep.Spc``: a batch of structured point clouds -- the packed octrees, their byte counts and, computed on first use, what
``ops.spc.scan_octrees`` and ``ops.spc.generate_points`` derive from them (reference: kaolin/rep/spc.py).  Unlike the reference's,
the octrees may live on the CPU: ``ops.spc`` takes them there."""
import torch

__all__ = ['Spc']


def _require(cond, message):
    if not cond:
        raise AssertionError(message)       # the reference's checks are asserts: the same exception, also under python -O


class Spc(object):
    """octrees (num_bytes) uint8: the octrees of the batch one after the other, a byte per node, bit ``x << 2 | y << 1 | z`` set where
    the node has that child, levels root first; lengths (B) int32: bytes per octree; features: optional, one row per point of
    the deepest level.

    ``max_level``, ``pyramids`` ((B, 2, max_level + 2) int32, CPU) and ``exsum`` (current layout: num_bytes entries) come from one
    ``scan_octrees`` call the first time any of them is read, ``point_hierarchies`` from ``generate_points``; values passed to the
    constructor are kept instead.  ``to_dict()`` gives the keyword arguments the ``ops.spc`` operators take (``KEYS``)."""

    KEYS = {'octrees', 'lengths', 'max_level', 'pyramids', 'exsum', 'point_hierarchies'}

    def __init__(self, octrees, lengths, max_level=None, pyramids=None, exsum=None, point_hierarchies=None, features=None):
        _require(isinstance(octrees, torch.Tensor) and octrees.dtype == torch.uint8 and octrees.dim() == 1,
                 'octrees must be a 1D ByteTensor.')
        _require(isinstance(lengths, torch.Tensor) and lengths.dtype == torch.int32 and lengths.dim() == 1,
                 'lengths must be a 1D IntTensor.')
        _require(max_level is None or isinstance(max_level, int), 'max_level must an int.')
        if pyramids is not None:
            _require(isinstance(pyramids, torch.Tensor) and pyramids.dtype == torch.int32, 'pyramids must be an IntTensor.')
            _require(pyramids.dim() == 3 and pyramids.shape[0] == lengths.shape[0] and pyramids.shape[1] == 2 and
                     (max_level is None or pyramids.shape[2] == max_level + 2),
                     'pyramids must be of shape (batch_size, 2, max_level + 2).')
            _require(not pyramids.is_cuda, 'pyramids must be on cpu.')
        if exsum is not None:
            _require(isinstance(exsum, torch.Tensor) and exsum.dtype == torch.int32, 'exsum must be an IntTensor.')
            _require(exsum.dim() == 1, 'exsum must be a 1D tensor.')
            _require(exsum.device == octrees.device, 'exsum must be on the same device than octrees.')
            if exsum.numel() != octrees.numel():
                raise ValueError(f'Spc: exsum has {exsum.numel()} entries for {octrees.numel()} octree bytes; only the current '
                                 'layout (num_bytes entries, inclusive sums) is accepted')
        if point_hierarchies is not None:
            _require(isinstance(point_hierarchies, torch.Tensor) and point_hierarchies.dtype == torch.int16,
                     'point_hierarchies must be a ShortTensor.')
            _require(point_hierarchies.dim() == 2 and point_hierarchies.shape[1] == 3,
                     'point_hierarchies must be of shape (num_nodes, 3).')
            _require(point_hierarchies.device == octrees.device, 'point_hierarchies must be on the same device than octrees.')
        if features is not None:
            _require(isinstance(features, torch.Tensor), 'features must be a torch.Tensor')
            _require(features.device == octrees.device, 'features must be on the same device as octrees.')
        self.octrees = octrees
        self.lengths = lengths
        self.features = features
        self._max_level = max_level
        self._pyramids = pyramids
        self._exsum = exsum
        self._point_hierarchies = point_hierarchies

    # ---- constructors ---------------------------------------------------------------------------------------------------------
    @classmethod
    def make_dense(cls, level, device='cuda'):
        """The fully occupied octree of ``level`` levels, as a batch of one."""
        from ..ops.spc import create_dense_spc              # ops.spc imports this module
        octree, lengths = create_dense_spc(level, device)
        return cls(octrees=octree, lengths=lengths)

    @classmethod
    def from_features(cls, feature_grids, masks=None):
        """feature_grids (B, C, X, Y, Z), masks (B, X, Y, Z) bool (default: a cell is occupied where any channel is non-zero) -> the
        Spc of the occupied cells, ``features`` (num_points, C) in the points' order."""
        from ..ops.spc import feature_grids_to_spc
        octrees, lengths, features = feature_grids_to_spc(feature_grids, masks=masks)
        return cls(octrees=octrees, lengths=lengths, features=features)

    @classmethod
    def from_list(cls, octrees_list):
        """A list of single octrees (1D uint8 tensors) -> their batch."""
        octrees = [o.reshape(-1) for o in octrees_list]
        return cls(torch.cat(octrees).contiguous(), torch.tensor([o.numel() for o in octrees], dtype=torch.int32))

    # ---- what the scan and the point generation derive ----------------------------------------------------------------------------
    def _scan(self):
        from ..ops.spc import scan_octrees
        self._max_level, self._pyramids, self._exsum = scan_octrees(self.octrees, self.lengths)

    @property
    def max_level(self):
        if self._max_level is None:
            self._scan()
        return self._max_level

    @property
    def pyramids(self):
        if self._pyramids is None:
            self._scan()
        return self._pyramids

    @property
    def exsum(self):
        if self._exsum is None:
            self._scan()
        return self._exsum

    @property
    def point_hierarchies(self):
        if self._point_hierarchies is None:
            from ..ops.spc import generate_points
            self._point_hierarchies = generate_points(self.octrees, self.pyramids, self.exsum)
        return self._point_hierarchies

    # ---- devices ------------------------------------------------------------------------------------------------------------------------
    def to(self, device, non_blocking=False, memory_format=torch.preserve_format):
        """The Spc on ``device``: itself when the octrees already are there; otherwise a new one with the octrees and whatever
        has been computed so far moved (lengths and pyramids stay on the CPU; features are not carried over, as in the
        reference)."""
        def move(x):
            return None if x is None else x.to(device=device, non_blocking=non_blocking, memory_format=memory_format)
        octrees = move(self.octrees)
        if octrees.data_ptr() == self.octrees.data_ptr():
            return self
        return Spc(octrees, self.lengths, self._max_level, self._pyramids, move(self._exsum), move(self._point_hierarchies))

    def cuda(self, device='cuda', non_blocking=False, memory_format=torch.preserve_format):
        return self.to(device=device, non_blocking=non_blocking, memory_format=memory_format)

    def cpu(self, memory_format=torch.preserve_format):
        return self.to(device='cpu', memory_format=memory_format)

    # ---- views ------------------------------------------------------------------------------------------------------------------------------
    @property
    def batch_size(self):
        return self.lengths.shape[0]

    def to_dict(self, keys=None):
        """{key: member} for ``keys`` (default: all of ``KEYS``): ``conv3d(**spc.to_dict(), level=..., input=...)``"""
        return {k: getattr(self, k) for k in (self.KEYS if keys is None else keys)}

    def num_points(self, lod):
        """(B) int32: the points every octree of the batch has at level ``lod`` (level 0 is the root: 1)."""
        return self.pyramids[:, 0, lod]
