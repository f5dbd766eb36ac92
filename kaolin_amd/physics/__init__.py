"""Physics on torch tensors behind the names of kaolin/physics: the Neo-Hookean material and the reduced (Simplicits) energy,
gradient and Hessian, fused in HIP on a GPU (kaolin_amd/csrc/physics.hip), the Simplicits skinning network with its Jacobian in
one HIP launch (kaolin_amd/csrc/skinning_mlp.hip), contacts between points: detection, the barrier and friction terms and
their reduced form (kaolin_amd/csrc/collisions.hip), the training of that network: the losses of
kaolin/physics/simplicits/losses.py with their gradient (kaolin_amd/csrc/simplicits_loss.hip) and the network's reverse pass
(kaolin_amd/csrc/skinning_mlp_backward.hip), and the scene forces: gravity, a floor, pinned points and the inertia term of a
Newton step, per point and in reduced form (kaolin_amd/csrc/scene_forces.hip).  With these every term of the Newton objective
has a matrix-free reduced (E, g, K), and optimization takes the step: Newton's method with the reference's line search on a
Cholesky factorisation and solve of the reduced Hessian (kaolin_amd/csrc/spd_solve.hip).  SimplicitsScene, the conjugate-gradient
solve, SimplicitsObject and its create_with_mlp driver, and a linear elastic material class are not here."""
from . import collisions, materials, optimization, scene_forces, simplicits  # noqa: F401
from .collisions import Collision  # noqa: F401
from .optimization import cholesky_spd, newtons_method, solve_spd  # noqa: F401
from .scene_forces import Boundary, Floor, Gravity, lbs_matrix, reduced_scene_terms  # noqa: F401
