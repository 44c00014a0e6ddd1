"""`pointnet2_stack_cuda` (VR/pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp:12-31): the entry points the voxel
RoI pooling and the PV-RCNN point branch use -- voxel query, stack grouping with its gradient, and the stacked ball query --
in the argument order of voxel_query.cpp:28-30, group_points.cpp:31-54 and ball_query.cpp, outputs allocated by the caller;
and the two samplers of sampling.cpp, `farthest_point_sampling_wrapper` and `stack_farthest_point_sampling_wrapper`.
The other entry points of that module (three_nn / interpolate, vector pool) are not provided."""
import torch

from .. import _lib
from ..ops import _ptr, _stream
from ._common import need_cuda_contiguous, runtime_errors


def _need_dtype(t, dtype, name):
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s (got %s)" % (name, dtype, t.dtype))


@runtime_errors
def voxel_query_wrapper(M, R1, R2, R3, nsample, radius, z_range, y_range, x_range, new_xyz_tensor, xyz_tensor,
                        new_coords_tensor, point_indices_tensor, idx_tensor):
    """point_indices int32 [B, R1, R2, R3] (-1 = empty cell); new_coords int32 [M, 4] (batch, z, y, x); idx int32
    [M, nsample] (zeroed by the caller, as voxel_query_utils.py:33 does): idx[m, 0] = -1 for an empty ball."""
    for t, nm in ((new_xyz_tensor, "new_xyz"), (xyz_tensor, "xyz"), (new_coords_tensor, "new_coords"),
                  (point_indices_tensor, "point_indices"), (idx_tensor, "idx")):
        need_cuda_contiguous(t, nm)
    _need_dtype(new_xyz_tensor, torch.float32, "new_xyz")
    _need_dtype(xyz_tensor, torch.float32, "xyz")
    for t, nm in ((new_coords_tensor, "new_coords"), (point_indices_tensor, "point_indices"), (idx_tensor, "idx")):
        _need_dtype(t, torch.int32, nm)
    if point_indices_tensor.dim() != 4 or tuple(point_indices_tensor.shape[1:]) != (R1, R2, R3):
        raise RuntimeError("voxel_query: point_indices must be [B, %d, %d, %d]" % (R1, R2, R3))
    if tuple(new_coords_tensor.shape) != (M, 4) or tuple(new_xyz_tensor.shape) != (M, 3) or tuple(idx_tensor.shape) != (M, nsample):
        raise RuntimeError("voxel_query: new_coords [M, 4], new_xyz [M, 3], idx [M, nsample]")
    shp_p, k1 = _lib.int3((R1, R2, R3))
    rng_p, k2 = _lib.int3((z_range, y_range, x_range))
    _lib.load().df3d_voxel_query_dense(
        _ptr(point_indices_tensor), point_indices_tensor.shape[0], shp_p, _ptr(xyz_tensor), xyz_tensor.shape[0],
        _ptr(new_xyz_tensor), _ptr(new_coords_tensor), int(M), rng_p, float(radius), int(nsample), _ptr(idx_tensor), _stream())
    return 1


@runtime_errors
def ball_query_wrapper(B, M, radius, nsample, new_xyz_tensor, new_xyz_batch_cnt_tensor, xyz_tensor, xyz_batch_cnt_tensor,
                       idx_tensor):
    """ball_query.cpp:31-47.  idx int32 [M, nsample] (zeroed by the caller, as pointnet2_utils.py:33 does), local to the
    frame: idx[m, 0] = -1 for an empty ball, whose other slots stay as they are."""
    for t, nm in ((new_xyz_tensor, "new_xyz"), (new_xyz_batch_cnt_tensor, "new_xyz_batch_cnt"), (xyz_tensor, "xyz"),
                  (xyz_batch_cnt_tensor, "xyz_batch_cnt"), (idx_tensor, "idx")):
        need_cuda_contiguous(t, nm)
    if tuple(new_xyz_tensor.shape) != (M, 3) or tuple(idx_tensor.shape) != (M, nsample) \
            or tuple(xyz_batch_cnt_tensor.shape) != (B,) or tuple(new_xyz_batch_cnt_tensor.shape) != (B,):
        raise RuntimeError("ball_query: new_xyz [M, 3], idx [M, nsample], counts [B]")
    from .. import ops
    ops.ball_query_stack(float(radius), int(nsample), xyz_tensor, xyz_batch_cnt_tensor, new_xyz_tensor,
                         new_xyz_batch_cnt_tensor, out=idx_tensor)
    return 1


def _stack_check(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, grouped, what):
    for t, nm in ((features, "features"), (features_batch_cnt, "features_batch_cnt"), (idx, "idx"),
                  (idx_batch_cnt, "idx_batch_cnt"), (grouped, what)):
        need_cuda_contiguous(t, nm)
    _need_dtype(features, torch.float32, "features")
    _need_dtype(grouped, torch.float32, what)
    for t, nm in ((features_batch_cnt, "features_batch_cnt"), (idx, "idx"), (idx_batch_cnt, "idx_batch_cnt")):
        _need_dtype(t, torch.int32, nm)
    if features.dim() != 2 or features.shape[1] != C or tuple(idx.shape) != (M, nsample) or tuple(grouped.shape) != (M, C, nsample) \
            or tuple(features_batch_cnt.shape) != (B,) or tuple(idx_batch_cnt.shape) != (B,):
        raise RuntimeError("group_points: features [N, C], idx [M, nsample], %s [M, C, nsample], counts [B]" % what)


@runtime_errors
def group_points_wrapper(B, M, C, nsample, features_tensor, features_batch_cnt_tensor, idx_tensor, idx_batch_cnt_tensor,
                         out_tensor):
    _stack_check(B, M, C, nsample, features_tensor, features_batch_cnt_tensor, idx_tensor, idx_batch_cnt_tensor, out_tensor,
                 "out")
    _lib.load().df3d_group_points_stack(
        _ptr(features_tensor), _ptr(features_batch_cnt_tensor), _ptr(idx_tensor), _ptr(idx_batch_cnt_tensor), int(B), int(M),
        int(C), int(nsample), features_tensor.shape[0], _ptr(out_tensor), _stream())
    return 1


@runtime_errors
def group_points_grad_wrapper(B, M, C, N, nsample, grad_out_tensor, idx_tensor, idx_batch_cnt_tensor,
                              features_batch_cnt_tensor, grad_features_tensor):
    """grad_features [N, C] is OVERWRITTEN with the ordered sums (the reference adds onto the zeros its caller allocates)."""
    _stack_check(B, M, C, nsample, grad_features_tensor, features_batch_cnt_tensor, idx_tensor, idx_batch_cnt_tensor,
                 grad_out_tensor, "grad_out")
    if grad_features_tensor.shape[0] != N:
        raise RuntimeError("group_points_grad: grad_features must be [N, C]")
    from .. import ops
    ops.group_points_stack_backward(grad_out_tensor, idx_tensor, idx_batch_cnt_tensor, features_batch_cnt_tensor, int(N),
                                    out=grad_features_tensor)
    return 1


@runtime_errors
def farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output):
    """sampling.cpp:24-37: xyz float32 [B, N, 3] -> output int32 [B, npoint] (first pick = row 0).  `temp` [B, N] is taken
    as holding 1e10, as the reference's callers fill it (it is initialised here); its contents afterwards are unspecified."""
    for t, nm in ((xyz, "xyz"), (temp, "temp"), (output, "output")):
        need_cuda_contiguous(t, nm)
    _need_dtype(xyz, torch.float32, "xyz")
    _need_dtype(temp, torch.float32, "temp")
    _need_dtype(output, torch.int32, "output")
    if tuple(xyz.shape) != (B, N, 3) or temp.numel() < B * N or output.numel() < B * npoint:
        raise RuntimeError("farthest_point_sampling: xyz [B, N, 3], temp [B, N], output [B, npoint]")
    _lib.load().df3d_furthest_point_sample(_ptr(xyz), int(B), int(N), int(npoint), _ptr(temp), _ptr(output), _stream())
    return 1


@runtime_errors
def stack_farthest_point_sampling_wrapper(xyz, temp, xyz_batch_cnt, idx, num_sampled_points):
    """sampling.cpp:40-60: xyz float32 [N1 + N2 .., 3], xyz_batch_cnt / num_sampled_points int32 [B] -> idx int32
    [sum(num_sampled_points)] of global rows, every segment in one launch.  `temp` [N] as above.  The counts are not read:
    a segment is clipped to the rows of xyz and the slots of idx."""
    for t, nm in ((xyz, "xyz"), (temp, "temp"), (xyz_batch_cnt, "xyz_batch_cnt"), (idx, "idx"),
                  (num_sampled_points, "num_sampled_points")):
        need_cuda_contiguous(t, nm)
    _need_dtype(temp, torch.float32, "temp")
    if temp.numel() < xyz.shape[0] or idx.dim() != 1:
        raise RuntimeError("stack_farthest_point_sampling: temp [N], idx [M]")
    from .. import ops
    ops.stack_furthest_point_sample(xyz, xyz_batch_cnt, num_sampled_points, total=idx.shape[0], mode="stack", out=idx)
    return 1
