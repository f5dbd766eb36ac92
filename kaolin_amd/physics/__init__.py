"""Physics on torch tensors behind the names of kaolin/physics: the Neo-Hookean material and the reduced (Simplicits) energy,
gradient and Hessian, fused in HIP on a GPU (kaolin_amd/csrc/physics.hip), and the Simplicits skinning network with its Jacobian in
one HIP launch (kaolin_amd/csrc/skinning_mlp.hip).  Scenes, collisions, the Newton driver, training and linear elasticity are not
here."""
from . import materials, simplicits  # noqa: F401
