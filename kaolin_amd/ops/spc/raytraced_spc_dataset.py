"""``kaolin.ops.spc.raytraced_spc_dataset``: depth maps of an SPC ray traced from given viewpoints, the input of ``bf_recon``
(reference: kaolin/ops/spc/raytraced_spc_dataset.py).  The reference builds its views with the ``Camera`` class, which is out of
scope here; ``_pinhole`` below produces what ``Camera.from_args(eye, at, up, fov, width, height)`` and
``generate_rays`` produce for one square pinhole view."""
import math

import torch
from torch.utils.data import Dataset

from .points import morton_to_points
from .spc import generate_points, scan_octrees

__all__ = ['RayTracedSPCDataset']


def _normalize(v):
    return v / torch.linalg.norm(v)


def _pinhole(eye, at, up, fov, res, device):
    """A look-at pinhole camera of ``res`` x ``res`` pixels with vertical field of view ``fov`` (radians) -> (world-to-camera
    view matrix (4, 4), fx, fy, cx, cy, ray origins (res * res, 3), ray directions (res * res, 3), row major from the top left).

    forward = normalize(at - eye), right = normalize(forward x up), up' = right x forward; the rotation rows are (right, up',
    -forward) and the translation is -R eye: the camera looks down -z.  Pixel centres at +0.5, NDC 2 p / res - 1; the
    camera-space direction (x tan(fov / 2), -y tan(fov / 2), -1) is rotated to the world and normalised."""
    eye, at, up = (torch.as_tensor(v, dtype=torch.float32).cpu() for v in (eye, at, up))
    forward = _normalize(at - eye)
    right = _normalize(torch.linalg.cross(forward, up))
    up2 = torch.linalg.cross(right, forward)
    R = torch.stack([right, up2, -forward])
    view = torch.eye(4)
    view[:3, :3] = R
    view[:3, 3] = -(R @ eye)
    tan_half = math.tan(fov / 2.0)
    focal = res / (2.0 * tan_half)
    centres = (torch.arange(res, dtype=torch.float32, device=device) + 0.5) * (2.0 / res) - 1.0
    ndc_y, ndc_x = torch.meshgrid(centres, centres, indexing='ij')
    cam_dirs = torch.stack([ndc_x * tan_half, -ndc_y * tan_half, -torch.ones_like(ndc_x)], dim=-1).reshape(-1, 3)
    dirs = cam_dirs @ R.to(device)                         # R^T applied to every direction: camera -> world
    dirs = dirs / torch.linalg.norm(dirs, dim=-1, keepdim=True)
    origins = eye.to(device).expand_as(dirs).contiguous()
    return view, focal, focal, res / 2.0, res / 2.0, origins, dirs.contiguous()


def _camera_matrices(view, fx, fy, cx, cy):
    """-> (Cam, In) (4, 4) CPU: the world-to-pixel matrix for row vectors with perspective division by z (the computer-vision
    convention: the view matrix transposed, y and z flipped, times the intrinsics), and the intrinsics"""
    In = torch.tensor([[fx, 0, 0, 0], [0, fy, 0, 0], [cx, cy, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)
    G = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
    return torch.mm(torch.mm(view.T.contiguous(), G), In), In


class RayTracedSPCDataset(Dataset):
    """Ray intersections of an SPC (octree) from predefined viewpoints that look at the origin: the frames ``bf_recon`` carves with.

    Item ``i`` is the ten-tuple (image (res, res, 3) float: 1 where a ray hit; depth map (res, res) float: the ray length to the
    first hit, ``max_depth`` where there is none; Cam (4, 4) CPU: world to pixel space, for row vectors and division by z; In
    (4, 4) CPU: the intrinsics; max_depth; mip_levels; true_depth (True: the map holds ray lengths, which bf_recon converts); start
    level of the carving; the dense points of that level (8^start_level, 3) short; whether any ray hit).  When no ray hits, the
    first nine entries are None."""

    # the reference's constants
    FOV = 0.644             # vertical field of view of the carving cameras, in radians
    MIP_LEVELS = 6
    START_LEVEL = 4

    def __init__(self, viewpoints, gs_octree, res=8):
        self.viewpoints, self.gs_octree, self.res = viewpoints, gs_octree, res
        self.device = gs_octree.device
        # the hierarchy the rays are traced against
        self.level, self.pyramid, self.exsum = scan_octrees(gs_octree, torch.tensor([gs_octree.numel()], dtype=torch.int32))
        self.point_hierarchy = generate_points(gs_octree, self.pyramid, self.exsum)
        self.carve_camera_fov, self.mip_levels, self.start_level = self.FOV, self.MIP_LEVELS, self.START_LEVEL
        self.max_depth = torch.finfo(torch.float32).max         # the depth of a ray that hits nothing

    def __len__(self):
        return len(self.viewpoints)

    def __getitem__(self, index):
        from ...render.spc import mark_pack_boundaries, unbatched_raytrace
        res = 2 ** self.res
        eye = torch.as_tensor(self.viewpoints[index], dtype=torch.float32).cpu()
        up = torch.tensor([0.0, 0.0, 1.0])
        at = torch.zeros(3)
        if torch.allclose(torch.linalg.cross(up, at - eye), torch.zeros(3)):    # up parallel to the view direction
            up = torch.tensor([0.0, 1.0, 0.0])
        view, fx, fy, cx, cy, origins, dirs = _pinhole(eye, at, up, self.carve_camera_fov, res, self.device)
        ridx, pidx, depths = unbatched_raytrace(self.gs_octree, self.point_hierarchy, self.pyramid[0], self.exsum, origins, dirs,
                                                self.level, return_depth=True, with_exit=False)
        is_any_ray_hit = len(ridx) > 0
        if not is_any_ray_hit:
            return None, None, None, None, None, None, None, None, None, is_any_ray_hit
        first = mark_pack_boundaries(ridx)                 # the closest hit of every ray
        first_ray = ridx[first].long()
        image = torch.zeros((res * res, 3), dtype=torch.float32, device=self.device)
        image[first_ray, :] = 1.0
        depthmap = torch.full((res * res, 1), self.max_depth, dtype=torch.float32, device=self.device)
        depthmap[first_ray, :] = depths[first]
        Cam, In = _camera_matrices(view, fx, fy, cx, cy)
        points = morton_to_points(torch.arange(8 ** self.start_level, device=self.device))
        return (image.reshape(res, res, 3), depthmap.reshape(res, res), Cam, In, self.max_depth, self.mip_levels, True,
                self.start_level, points, is_any_ray_hit)
