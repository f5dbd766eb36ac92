"""Physics on torch tensors behind the names of kaolin/physics: the Neo-Hookean material and the reduced (Simplicits) energy,
gradient and Hessian, fused in HIP on a GPU (kaolin_amd/csrc/physics.hip), the Simplicits skinning network with its Jacobian in
one HIP launch (kaolin_amd/csrc/skinning_mlp.hip), and contacts between points: detection, the barrier and friction terms and
their reduced form (kaolin_amd/csrc/collisions.hip), and the training of that network: the losses of
kaolin/physics/simplicits/losses.py with their gradient (kaolin_amd/csrc/simplicits_loss.hip) and the network's reverse pass
(kaolin_amd/csrc/skinning_mlp_backward.hip).  Scenes, the Newton driver, SimplicitsObject and its create_with_mlp driver, and a
linear elastic material class are not here."""
from . import collisions, materials, simplicits  # noqa: F401
from .collisions import Collision  # noqa: F401
