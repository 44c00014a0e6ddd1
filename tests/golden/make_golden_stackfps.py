#!/usr/bin/env python3
"""Generate tests/golden/stack_fps.npz FROM THE REFERENCE ITSELF: stacked furthest point sampling.

Runs only where the reference checkout exists.  The reference's own `sector_fps` (voxel_set_abstraction.py:78-121) and
`StackFarthestPointSampling` (pointnet2_stack/pointnet2_utils.py:187-221) run on the CPU with their packages stubbed the way
make_golden_vsa.py does it; the compiled `pointnet2_stack_cuda.stack_farthest_point_sampling_wrapper` is replaced by the host
restatement of its kernel (tests/stackfps_reference.py).  The fixture stores inputs and the reference's outputs only.

The sector case keeps every point's (angle / sector size) at least 1e-3 away from an integer, so that the sector of a point
does not depend on the last bit of atan2; the random segments keep every pick's margin at MARGIN_ULPS or more."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import make_golden_vsa as mgv  # noqa: E402
import stackfps_reference as fr  # noqa: E402


def stack_farthest_point_sampling_wrapper(xyz, temp, xyz_batch_cnt, idx, num_sampled_points):
    assert float(temp.min()) == 1e10 and temp.numel() == xyz.shape[0]
    out = fr.stack_fps(xyz.numpy().astype(np.float32), xyz_batch_cnt.tolist(), num_sampled_points.tolist(), fr.STACK)
    assert len(out) == idx.numel()
    idx.copy_(torch.from_numpy(out))
    return 1


def stack_cases():
    """name -> (xyz, counts, npoint as the caller passes it)"""
    a = np.concatenate([fr.random_cloud(n, 70 + i) for i, n in enumerate((120, 7, 300))])
    return {"list": (a, [120, 7, 300], [16, 7, 33]),
            "int": (a, [120, 7, 300], 5),
            "tensor": (a, [120, 7, 300], torch.tensor([1, 3, 40]).int()),
            "lattice": (fr.lattice_cloud(600, 5), [600], [64])}


def main():
    if not os.path.isdir(mgv.R):
        raise SystemExit("the reference checkout is needed to generate stack_fps.npz")
    ref = mgv.import_reference()
    sys.modules["pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda"].stack_farthest_point_sampling_wrapper = \
        stack_farthest_point_sampling_wrapper
    import importlib
    utils = importlib.import_module("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils")
    out = {}
    for name, (xyz, cnt, npoint) in stack_cases().items():
        got = utils.stack_farthest_point_sample(torch.from_numpy(xyz), torch.tensor(cnt).int(), npoint)
        per = npoint.tolist() if isinstance(npoint, torch.Tensor) else (npoint if isinstance(npoint, list) else [npoint] * len(cnt))
        if name != "lattice":
            s = 0
            for n, m in zip(cnt, per):
                assert fr.pick_margins(xyz[s:s + n], m, 1024).min() >= fr.MARGIN_ULPS, "pick another seed"
                s += n
        out["stack__%s__xyz" % name], out["stack__%s__cnt" % name] = xyz, np.asarray(cnt, np.int32)
        out["stack__%s__num" % name], out["stack__%s__idx" % name] = np.asarray(per, np.int32), got.numpy().astype(np.int32)
    points, K, sectors = fr.sector_case()
    _, q = fr.sector_of(points, sectors)
    assert np.abs(q - np.round(q)).min() > 1e-3, "pick another seed"
    got = ref["vsa"].sector_fps(torch.from_numpy(points), K, sectors)
    want, xyz, cnt, num = fr.sector_fps(points, K, sectors)
    assert 0 in cnt and np.array_equal(got.numpy(), want)
    s = 0
    for n, m in zip(cnt, num):
        assert n == 0 or fr.pick_margins(xyz[s:s + n], m, 1024).min() >= fr.MARGIN_ULPS, "pick another seed"
        s += n
    out["sector__points"], out["sector__args"], out["sector__sampled"] = points, np.asarray([K, sectors], np.int32), got.numpy()
    mg.save("stack_fps.npz", **out)
    print("stack_fps.npz:", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
