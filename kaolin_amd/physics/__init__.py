"""Physics on torch tensors behind the names of kaolin/physics: the Neo-Hookean material and the reduced (Simplicits) energy,
gradient and Hessian, fused in HIP on a GPU (kaolin_amd/csrc/physics.hip), the Simplicits skinning network with its Jacobian in
one HIP launch (kaolin_amd/csrc/skinning_mlp.hip), and contacts between points: detection, the barrier and friction terms and
their reduced form (kaolin_amd/csrc/collisions.hip).  Scenes, the Newton driver, training and linear elasticity are not here."""
from . import collisions, materials, simplicits  # noqa: F401
from .collisions import Collision  # noqa: F401
