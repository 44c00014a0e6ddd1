"""`roiaware_pool3d_cuda` (VR/pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp): the entry point the point heads use,
points_in_boxes_gpu(boxes, pts, box_idx_of_points), in the pybind argument order with the output allocated by the caller
(roiaware_pool3d_utils.py:28-41 fills it with -1 first; every element is written here).  The other entry points of that module
(the RoI-aware pooling forward / backward, points_in_boxes_cpu) are not provided."""
import torch

from .. import ops as _ops
from ._common import need_cuda_contiguous, runtime_errors


@runtime_errors
def points_in_boxes_gpu(boxes_tensor, pts_tensor, box_idx_of_points_tensor):
    """boxes [B, N, 7] (x, y, z, dx, dy, dz, heading), pts [B, npts, 3] float32; box_idx_of_points int32 [B, npts] receives the
    index of the first box that holds the point, else -1."""
    for t, nm in ((boxes_tensor, "boxes"), (pts_tensor, "pts"), (box_idx_of_points_tensor, "box_idx_of_points")):
        need_cuda_contiguous(t, nm)
    if box_idx_of_points_tensor.dtype != torch.int32:
        raise RuntimeError("box_idx_of_points must be int32 (got %s)" % box_idx_of_points_tensor.dtype)
    _ops.points_in_boxes(boxes_tensor, pts_tensor, out=box_idx_of_points_tensor)
    return 1
